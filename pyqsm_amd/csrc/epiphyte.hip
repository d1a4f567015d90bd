// epiphyte.hip — the two stages between the contraction and the batched alpha-shape area in pyQSM's
// canopy_metrics.identify_epiphytes:
//
//   selection   pyqsm_select_values: elements of given ranks of the sorted keys of n rows, the key a
//               component of the row or its norm sqrt(((x*x) + (y*y)) + (z*z)). A radix selection in
//               the manner of pdist.hip: keys recomputed from the rows in each of eight 8-bit passes,
//               integer histograms, a one-wave kernel between passes (reduce.hpp), nothing read back
//               until the end. Keys may be negative: the usual monotone map of fp64 to u64, -0.0
//               keyed as +0.0. pyqsm_split_above_dev partitions by a threshold through
//               compact_flagged; pyqsm_shift_components labels wood / leaf / epiphyte by the two
//               percentiles of viz.color.split_on_percentile, NumPy's linear rule applied on the host.
//   k-means++   pyqsm_kmeans_pp: scikit-learn's KMeans(init="k-means++", n_init=1, algorithm="lloyd")
//               on n points of d <= 3 dimensions and k <= 64 centres, as the header states it: many
//               workgroups, a wave per chunk of 256 points, four consecutive points per lane, centres
//               broadcast from LDS. Iterations are queued in bursts behind a device-side "done" word.
//
// No float atomics: every floating-point sum is a chunk sum (reduce.hpp), the chunk totals added one
// at a time in chunk order by a wave that loads 64 of them at once. Integer atomics count histogram
// bins, labelled rows and "some label changed": the same bits on every run.
#include "reduce.hpp"

#include <algorithm>
#include <cmath>

namespace pyqsm {

using u64 = unsigned long long;

// ---------------------------------------------------------------- selection

constexpr int kSelBins = 256;  // eight bits per pass
constexpr int kSelPasses = 8;
constexpr int kSelMaxRanks = PYQSM_PDIST_MAX_RANKS;
constexpr int kSelThreads = 256;

// key >= 0: that component of the row; PYQSM_KEY_NORM: the row's norm (width 3)
__device__ __forceinline__ double row_key(const double* __restrict__ v, int64_t i, int width, int key) {
  if (key >= 0) return v[i * width + key];
  const double x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
  return sqrt(((x * x) + (y * y)) + (z * z));
}

// fp64 -> u64 that orders as the doubles do; both zeros map to +0.0's image
__host__ __device__ __forceinline__ u64 order_bits(u64 b) {
  if ((b << 1) == 0) b = 0;
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
static double from_order_bits(u64 m) {
  const u64 b = (m >> 63) ? (m ^ (1ull << 63)) : ~m;
  double d;
  std::memcpy(&d, &b, sizeof d);
  return d;
}

// One pass: every row whose key carries a group's prefix is counted by its next digit in the group's
// LDS histogram, which goes to the global one at the end. The lanes of a wave that share the first
// active lane's bin (nearly all of them in the passes over the exponent) are counted by one add.
// Pass 0 also looks for a NaN anywhere in the rows.
__global__ __launch_bounds__(kSelThreads) void k_sel_hist(const double* __restrict__ v, int64_t n, int width, int key,
                                                          int n_ranks, int pass, const int32_t* __restrict__ gcount,
                                                          const u64* __restrict__ gprefix, u64* __restrict__ hist,
                                                          int32_t* __restrict__ nan_flag) {
  extern __shared__ uint32_t s_hist[];  // [n_ranks][256]
  __shared__ u64 s_gp[kSelMaxRanks];
  const int tid = threadIdx.x;
  const int groups = gcount[0];
  if (tid < groups) s_gp[tid] = gprefix[tid];
  for (int k = tid; k < groups * kSelBins; k += kSelThreads) s_hist[k] = 0;
  __syncthreads();
  const int pre_shift = 63 - 8 * pass;  // prefix = (key >> 1) >> pre_shift: the top 8 * pass bits
  const int dig_shift = 56 - 8 * pass;
  bool bad = false;
  const int64_t stride = int64_t(gridDim.x) * kSelThreads;
  const int64_t rounds = (n + stride - 1) / stride;  // the same for every lane: the ballots below see whole waves
  for (int64_t rd = 0; rd < rounds; ++rd) {
    const int64_t i = rd * stride + int64_t(blockIdx.x) * kSelThreads + tid;
    int bin = -1;
    if (i < n) {
      if (pass == 0)
        for (int j = 0; j < width; ++j) {
          const double a = v[i * width + j];
          bad |= a != a;
        }
      const u64 kb = order_bits(u64(__double_as_longlong(row_key(v, i, width, key))));
      const u64 pre = (kb >> 1) >> pre_shift;
      for (int g = 0; g < groups; ++g)
        if (pre == s_gp[g]) bin = g * kSelBins + int((kb >> dig_shift) & 255);
    }
    const u64 active = __ballot(bin >= 0);
    if (active) {
      const int lead = __ffsll((long long)active) - 1;
      const int b0 = __shfl(bin, lead, 64);
      const u64 same = __ballot(bin == b0);
      if ((threadIdx.x & 63) == lead) atomicAdd(&s_hist[b0], uint32_t(__popcll(same)));
      else if (bin >= 0 && bin != b0) atomicAdd(&s_hist[bin], 1u);
    }
  }
  if (bad) atomicOr(nan_flag, 1);
  __syncthreads();
  for (int k = tid; k < groups * kSelBins; k += kSelThreads) {
    const uint32_t c = s_hist[k];
    if (c) atomicAdd(&hist[k], u64(c));
  }
}

enum { kCmpGt = 0, kCmpGe = 1, kCmpLt = 2, kCmpLe = 3 };

// flags[i] = cmp(key(row i), thr) for i < n, flags[n] = 0: what compact_flagged takes
__global__ __launch_bounds__(256) void k_split_flags(const double* __restrict__ v, int64_t n, int width, int key,
                                                     int cmp, double thr, int32_t* __restrict__ flags) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i > n) return;
  int32_t f = 0;
  if (i < n) {
    const double a = row_key(v, i, width, key);
    f = cmp == kCmpGt ? a > thr : cmp == kCmpGe ? a >= thr : cmp == kCmpLt ? a < thr : a <= thr;
  }
  flags[i] = f;
}

// label 0: norm not above thr_mag; 1: above, and z above thr_z; 2: the other rows above thr_mag.
// counts[0] += rows above thr_mag, counts[1] += label 1 (integer atomics, one per wave).
__global__ __launch_bounds__(256) void k_shift_labels(const double* __restrict__ shift, int64_t n, double thr_mag,
                                                      double thr_z, uint8_t* __restrict__ labels,
                                                      u64* __restrict__ counts) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  bool high = false, leaf = false;
  if (i < n) {
    high = row_key(shift, i, 3, PYQSM_KEY_NORM) > thr_mag;
    leaf = high && shift[3 * i + 2] > thr_z;
    labels[i] = high ? (leaf ? 1 : 2) : 0;
  }
  const u64 mh = __ballot(high), ml = __ballot(leaf);
  if ((threadIdx.x & 63) == 0) {
    if (mh) atomicAdd(&counts[0], u64(__popcll(mh)));
    if (ml) atomicAdd(&counts[1], u64(__popcll(ml)));
  }
}

// NumPy's default percentile on m sorted values: the ranks around the virtual index (m - 1) q / 100
// and the weight of the upper one; _lerp with its t >= 0.5 branch.
static void percentile_ranks(int64_t m, double q, int64_t* lo, int64_t* hi, double* t) {
  const double v = double(m - 1) * (q / 100.0);
  const double f = std::floor(v);
  *t = v - f;
  *lo = int64_t(f);
  *hi = std::min<int64_t>(*lo + 1, m - 1);
}
static double np_lerp(double a, double b, double t) {
  const double diff = b - a;
  double out = a + diff * t;
  if (t >= 0.5) out = b - diff * (1.0 - t);
  if (t == 0.0) out = a;
  return out;
}

static int check_key(int32_t width, int32_t key, const char* who) {
  if (width != 1 && width != 3) return fail(PYQSM_EINVAL, "%s: rows of %d values, must be 1 or 3", who, int(width));
  if (key == PYQSM_KEY_NORM ? width != 3 : (key < 0 || key >= width))
    return fail(PYQSM_EINVAL, "%s: key %d on rows of %d values", who, int(key), int(width));
  return 0;
}

// The elements of `ranks` (host, a negative one marks an unused slot) of the sorted keys of the device
// rows, into values (host). Synchronises once, at the end.
static int select_device(Ctx* c, const double* d_v, int64_t n, int width, int key, const int64_t* ranks, int n_ranks,
                         double* values) {
  const int R = std::max(n_ranks, 1);
  std::vector<u64> remaining(size_t(R), 0);
  std::vector<int32_t> group(size_t(R) + 2, -1);  // [R] groups, then gcount, then the NaN flag
  bool any = false;
  for (int r = 0; r < n_ranks; ++r) {
    values[r] = 0.0;
    if (ranks[r] < 0) continue;
    if (ranks[r] >= n)
      return fail(PYQSM_EINVAL, "rank %lld of %lld keys", (long long)ranks[r], (long long)n);
    remaining[size_t(r)] = u64(ranks[r]);
    group[size_t(r)] = 0;
    any = true;
  }
  group[size_t(R)] = any ? 1 : 0;
  group[size_t(R) + 1] = 0;
  if (!any) return 0;
  u64 *d_state, *d_rem;  // prefix [R], gprefix [R], histograms [R][256]: cleared together
  int32_t* d_group;
  const size_t n_state = 2 * size_t(R) + size_t(R) * kSelBins;
  PQ_TRY(c->arena.get(n_state, &d_state));
  PQ_TRY(upload(c, remaining.data(), size_t(R), &d_rem));
  PQ_TRY(upload(c, group.data(), size_t(R) + 2, &d_group));
  PQ_HIP(hipMemsetAsync(d_state, 0, n_state * sizeof(u64), c->stream));
  u64 *d_prefix = d_state, *d_gprefix = d_state + R, *d_hist = d_state + 2 * R;
  int32_t *d_gcount = d_group + R, *d_nan = d_group + R + 1;
  const int grid = int(std::min<int64_t>((n + kSelThreads - 1) / kSelThreads, int64_t(c->cu_count) * 8));
  const size_t lds = size_t(R) * kSelBins * sizeof(uint32_t);
  {
    ProfScope ps(c, "select_passes");
    for (int p = 0; p < kSelPasses; ++p) {
      hipLaunchKernelGGL(k_sel_hist, dim3(grid), dim3(kSelThreads), lds, c->stream, d_v, n, width, key, R, p,
                         d_gcount, d_gprefix, d_hist, d_nan);
      hipLaunchKernelGGL((k_radix_select_update<kSelBins, kSelMaxRanks>), dim3(1), dim3(64), 0, c->stream, R, d_hist,
                         d_prefix, d_rem, d_group, d_gcount, d_gprefix);
      PQ_HIP(hipGetLastError());
    }
  }
  std::vector<u64> keys(size_t(R), 0);
  int32_t nan = 0;
  PQ_TRY(download(c, keys.data(), d_prefix, size_t(R)));
  PQ_TRY(download(c, &nan, d_nan, 1));
  PQ_TRY(stream_sync(c));
  if (nan) return fail(PYQSM_EINVAL, "a NaN among the values");
  for (int r = 0; r < n_ranks; ++r)
    if (ranks[r] >= 0) values[r] = from_order_bits(keys[size_t(r)]);
  return 0;
}

static int percentile_device(Ctx* c, const double* d_v, int64_t n, int width, int key, double q, double* out) {
  int64_t rk[2];
  double t, ab[2];
  percentile_ranks(n, q, &rk[0], &rk[1], &t);
  PQ_TRY(select_device(c, d_v, n, width, key, rk, 2, ab));
  *out = np_lerp(ab[0], ab[1], t);
  return 0;
}

static bool bad_percentile(double q) { return !(q >= 0.0 && q <= 100.0); }

// d_labels u8 [n] on the device; thresholds [2] and counts [3] on the host
static int shift_components_device(Ctx* c, const double* d_shift, int64_t n, double q_mag, double q_z,
                                   uint8_t* d_labels, double* thresholds, int64_t* counts) {
  PQ_TRY(percentile_device(c, d_shift, n, 3, PYQSM_KEY_NORM, q_mag, &thresholds[0]));
  int32_t* d_flags;
  double* d_high;
  u64* d_counts;
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_flags));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_high));
  PQ_TRY(c->arena.get(2, &d_counts));
  int32_t m = 0;
  {
    ProfScope ps(c, "shift_split");
    hipLaunchKernelGGL(k_split_flags, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, d_shift, n, 3,
                       int(PYQSM_KEY_NORM), int(kCmpGt), thresholds[0], d_flags);
    PQ_HIP(hipGetLastError());
    PQ_TRY(compact_flagged(c, d_flags, n, nullptr, nullptr, d_shift, d_high));
  }
  PQ_TRY(fetch(c, &m, d_flags + n));
  thresholds[1] = std::nan("");
  if (m > 0) PQ_TRY(percentile_device(c, d_high, m, 3, 2, q_z, &thresholds[1]));
  u64 h_counts[2] = {0, 0};
  {
    ProfScope ps(c, "shift_labels");
    PQ_HIP(hipMemsetAsync(d_counts, 0, 2 * sizeof(u64), c->stream));
    hipLaunchKernelGGL(k_shift_labels, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, d_shift, n, thresholds[0],
                       thresholds[1], d_labels, d_counts);
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(fetch(c, h_counts, d_counts, 2));
  counts[0] = n - int64_t(h_counts[0]);
  counts[1] = int64_t(h_counts[1]);
  counts[2] = int64_t(h_counts[0]) - int64_t(h_counts[1]);
  return 0;
}

// ---------------------------------------------------------------- k-means++ and Lloyd

static constexpr int kPpMaxK = PYQSM_KMEANSPP_MAX_K;
static constexpr int kPpMaxT = 8;       // trials per seeding step: 2 + int(ln 64) = 6
static constexpr int kPpThreads = 256;  // four waves, a chunk each
static constexpr int kPpBurst = 32;     // most Lloyd iterations queued between two reads of the state

struct KppState {
  double mu[3];
  double tol_abs, inertia, pot;
  int32_t done, strict, iter, changed, n_empty, pad;
};

// ((dx*dx) + dy*dy) + dz*dz, always direct
template <int D>
__device__ __forceinline__ double kpp_d2(const double* p, const double* c) {
  const double dx = p[0] - c[0];
  double d = dx * dx;
  if (D > 1) {
    const double dy = p[1] - c[1];
    d = d + dy * dy;
  }
  if (D > 2) {
    const double dz = p[2] - c[2];
    d = d + dz * dz;
  }
  return d;
}

// Lane `lane` of the wave that owns chunk b: its four consecutive points (zeros past the end)
template <int D>
__device__ __forceinline__ void kpp_load(const double* __restrict__ x, int64_t n, int64_t b, int lane, double (&p)[4][3],
                                         bool (&in)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t i = b * kChunk + lane * 4 + u;
    in[u] = i < n;
#pragma unroll
    for (int j = 0; j < 3; ++j) p[u][j] = (j < D && in[u]) ? x[i * D + j] : 0.0;
  }
}

// Lane j's value of v in every lane, j uniform over the wave: two v_readlane, no LDS crossbar
__device__ __forceinline__ double wave_read(double v, int j) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}

// p[0], p[1], ... p[m - 1] added one at a time from 0.0, by a whole wave that loads 64 at once (the
// next 64 are on their way while these are added); the same bits in every lane. The chain of m
// dependent additions is what the contract costs: about m add latencies, whatever the bandwidth.
__device__ __forceinline__ double wave_seq_total(const double* __restrict__ p, int64_t m, int lane) {
  double s = 0.0;
  double v = lane < m ? p[lane] : 0.0;
  for (int64_t b0 = 0; b0 < m; b0 += 64) {
    const double nxt = b0 + 64 + lane < m ? p[b0 + 64 + lane] : 0.0;
    if (m - b0 >= 64) {
#pragma unroll
      for (int j = 0; j < 64; ++j) s = s + wave_read(v, j);
    } else {
      for (int j = 0; j < int(m - b0); ++j) s = s + wave_read(v, j);
    }
    v = nxt;
  }
  return s;
}

// the nearest centre of `p` among cen[0 .. k), ties to the lowest
template <int D>
__device__ __forceinline__ int kpp_nearest(const double* p, const double* cen, int k, double* d_out) {
  int best = 0;
  double bd = 0.0;
  for (int c = 0; c < k; ++c) {
    const double d = kpp_d2<D>(p, cen + 3 * c);
    if (c == 0 || d < bd) {
      bd = d;
      best = c;
    }
  }
  *d_out = bd;
  return best;
}

#define KPP_CHUNK_LOOP(b)                                                  \
  const int lane = threadIdx.x & 63;                                       \
  for (int64_t b = int64_t(blockIdx.x) * (kPpThreads / 64) + (threadIdx.x >> 6); b < nch; \
       b += int64_t(gridDim.x) * (kPpThreads / 64))

// part[j * nch + b] = chunk sum of column j over chunk b
template <int D>
__global__ __launch_bounds__(kPpThreads) void k_kpp_colsum(const double* __restrict__ x, int64_t n, int64_t nch,
                                                           double* __restrict__ part) {
  KPP_CHUNK_LOOP(b) {
    double p[4][3];
    bool in[4];
    kpp_load<D>(x, n, b, lane, p, in);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const double s = chunk_wave_sum(p[0][j], p[1][j], p[2][j], p[3][j]);
      if (lane == 0) part[j * nch + b] = s;
    }
  }
}

// mu[j] = total of column j / n: one wave per column
__global__ __launch_bounds__(64) void k_kpp_mu(const double* __restrict__ part, int64_t nch, int64_t n,
                                               KppState* __restrict__ st) {
  const double s = wave_seq_total(part + blockIdx.x * nch, nch, threadIdx.x);
  if (threadIdx.x == 0) st->mu[blockIdx.x] = s / double(n);
}

// xc = x - mu, part[j * nch + b] = chunk sum of xc_j^2 over chunk b
template <int D>
__global__ __launch_bounds__(kPpThreads) void k_kpp_centre(const double* __restrict__ x, int64_t n, int64_t nch,
                                                           const KppState* __restrict__ st, double* __restrict__ xc,
                                                           double* __restrict__ part) {
  KPP_CHUNK_LOOP(b) {
    double p[4][3];
    bool in[4];
    kpp_load<D>(x, n, b, lane, p, in);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const double m = st->mu[j];
      double q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double v = p[u][j] - m;
        if (in[u]) xc[(b * kChunk + lane * 4 + u) * D + j] = v;
        q[u] = in[u] ? v * v : 0.0;
      }
      const double s = chunk_wave_sum(q[0], q[1], q[2], q[3]);
      if (lane == 0) part[j * nch + b] = s;
    }
  }
}

// tol_abs = tol * mean_j(total of column j's squares / n); the first centre is point `first`.
// One block of D waves.
__global__ __launch_bounds__(192) void k_kpp_tol(const double* __restrict__ part, int64_t nch, int64_t n, int D,
                                                 double tol, int64_t first, const double* __restrict__ xc,
                                                 KppState* __restrict__ st, double* __restrict__ cen,
                                                 int64_t* __restrict__ seeds) {
  __shared__ double s_var[3];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double s = wave_seq_total(part + w * nch, nch, lane);
  if (lane == 0) s_var[w] = s / double(n);
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = s_var[0];
    for (int j = 1; j < D; ++j) sum = sum + s_var[j];
    st->tol_abs = tol * (sum / double(D));
    for (int j = 0; j < D; ++j) cen[j] = xc[first * D + j];
    seeds[0] = first;
  }
}

// closest = d2 to centre ci (is_first) or min(closest, that); ct[b] = chunk sum of closest over chunk b
template <int D>
__global__ __launch_bounds__(kPpThreads) void k_kpp_closest(const double* __restrict__ xc, int64_t n, int64_t nch,
                                                            const double* __restrict__ cen, int ci, int is_first,
                                                            double* __restrict__ closest, double* __restrict__ ct) {
  const double c[3] = {cen[3 * ci], cen[3 * ci + 1], cen[3 * ci + 2]};
  KPP_CHUNK_LOOP(b) {
    double p[4][3], v[4];
    bool in[4];
    kpp_load<D>(xc, n, b, lane, p, in);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = b * kChunk + lane * 4 + u;
      double d = kpp_d2<D>(p[u], c);
      if (in[u] && !is_first) {
        const double old = closest[i];
        d = d < old ? d : old;
      }
      if (in[u]) closest[i] = d;
      v[u] = in[u] ? d : 0.0;
    }
    const double s = chunk_wave_sum(v[0], v[1], v[2], v[3]);
    if (lane == 0) ct[b] = s;
  }
}

// pot = the chunk totals added in order: one wave
__global__ __launch_bounds__(64) void k_kpp_pot(const double* __restrict__ ct, int64_t nch, KppState* __restrict__ st) {
  const double s = wave_seq_total(ct, nch, threadIdx.x);
  if (threadIdx.x == 0) st->pot = s;
}

// The T candidates of a seeding step, one wave. r_t = u[t] * pot; the running sum of `closest` is the
// chunk totals added in order from 0.0 up to the first chunk whose cumulative total reaches r_t (the
// last chunk if none does), then the chunk's values one at a time from the total before it; the
// candidate is the first point at which the sum reaches r_t, the chunk's last if none does.
__global__ __launch_bounds__(64) void k_kpp_pick(const double* __restrict__ ct, int64_t nch,
                                                 const double* __restrict__ closest, int64_t n,
                                                 const double* __restrict__ u, int T, const KppState* __restrict__ st,
                                                 int64_t* __restrict__ cand) {
  const int lane = threadIdx.x;
  const double r = lane < T ? u[lane] * st->pot : 0.0;
  bool found = lane >= T;
  int chunk = int(nch - 1);  // nch < 2^23
  double base = 0.0, cum = 0.0;  // cum: the same in every lane
  double v = lane < nch ? ct[lane] : 0.0;
  for (int64_t b0 = 0; b0 < nch && !__all(found); b0 += 64) {
    const double nxt_v = b0 + 64 + lane < nch ? ct[b0 + 64 + lane] : 0.0;  // on its way while these are added
    if (nch - b0 > 64) {  // not the last chunks: selects, no branches
#pragma unroll
      for (int j = 0; j < 64; ++j) {
        const double nxt = cum + wave_read(v, j);
        const bool hit = !found && nxt >= r;
        chunk = hit ? int(b0) + j : chunk;
        base = hit ? cum : base;
        found |= hit;
        cum = nxt;
      }
    } else {
      for (int j = 0; j < int(nch - b0); ++j) {
        const double nxt = cum + wave_read(v, j);
        if (!found && (nxt >= r || b0 + j == nch - 1)) {  // the last chunk takes what none has reached
          found = true;
          chunk = int(b0) + j;
          base = cum;
        }
        cum = nxt;
      }
    }
    v = nxt_v;
  }
  for (int t = 0; t < T; ++t) {  // the wave serves one trial at a time
    const int64_t bt = __shfl(chunk, t, 64);
    const double rt = __shfl(r, t, 64);
    double s = __shfl(base, t, 64);
    const int64_t i0 = bt * kChunk;
    const int len = n - i0 < kChunk ? int(n - i0) : kChunk;
    double v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = lane * 4 + q < len ? closest[i0 + lane * 4 + q] : 0.0;
    int64_t pick = i0 + len - 1;
    bool hit = false;
    for (int l = 0; l < 64 && !hit && l * 4 < len; ++l) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double a = wave_read(v[q], l);
        if (!hit && l * 4 + q < len) {
          s = s + a;
          if (s >= rt) {
            hit = true;
            pick = i0 + l * 4 + q;
          }
        }
      }
    }
    if (lane == 0) cand[t] = pick;
  }
}

// tp[t * nch + b] = chunk sum over chunk b of min(closest, d2 to candidate t)
template <int D>
__global__ __launch_bounds__(kPpThreads) void k_kpp_trial(const double* __restrict__ xc, int64_t n, int64_t nch,
                                                          const double* __restrict__ closest,
                                                          const int64_t* __restrict__ cand, int T,
                                                          double* __restrict__ tp) {
  __shared__ double s_c[kPpMaxT * 3];
  if (threadIdx.x < T * 3) {
    const int t = threadIdx.x / 3, j = threadIdx.x % 3;
    s_c[threadIdx.x] = j < D ? xc[cand[t] * D + j] : 0.0;
  }
  __syncthreads();
  KPP_CHUNK_LOOP(b) {
    double p[4][3], old[4];
    bool in[4];
    kpp_load<D>(xc, n, b, lane, p, in);
#pragma unroll
    for (int u = 0; u < 4; ++u) old[u] = in[u] ? closest[b * kChunk + lane * 4 + u] : 0.0;
    for (int t = 0; t < T; ++t) {
      double v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double d = kpp_d2<D>(p[u], s_c + 3 * t);
        v[u] = in[u] ? (d < old[u] ? d : old[u]) : 0.0;
      }
      const double s = chunk_wave_sum(v[0], v[1], v[2], v[3]);
      if (lane == 0) tp[t * nch + b] = s;
    }
  }
}

// One block of T waves: wave t totals trial t's potential; the smallest wins, ties to the earlier
// trial; its candidate becomes centre ci and its potential the next step's.
__global__ __launch_bounds__(64 * kPpMaxT) void k_kpp_choose(const double* __restrict__ tp, int64_t nch, int T,
                                                             const int64_t* __restrict__ cand,
                                                             const double* __restrict__ xc, int D, int ci,
                                                             double* __restrict__ cen, int64_t* __restrict__ seeds,
                                                             KppState* __restrict__ st) {
  __shared__ double s_pot[kPpMaxT];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double s = wave_seq_total(tp + w * nch, nch, lane);
  if (lane == 0) s_pot[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = 0;
    for (int t = 1; t < T; ++t)
      if (s_pot[t] < s_pot[best]) best = t;
    const int64_t i = cand[best];
    seeds[ci] = i;
    for (int j = 0; j < 3; ++j) cen[3 * ci + j] = j < D ? xc[i * D + j] : 0.0;
    st->pot = s_pot[best];
  }
}

// One Lloyd assignment (a no-op once the state says done): label, note whether any label changed, and
// write every centre's masked chunk sums of each coordinate P[(c * D + j) * nch + b] and member
// counts C[c * nch + b].
template <int D>
__global__ __launch_bounds__(kPpThreads) void k_kpp_assign(const double* __restrict__ xc, int64_t n, int64_t nch, int k,
                                                           const double* __restrict__ cen, int32_t* __restrict__ labels,
                                                           double* __restrict__ P, int32_t* __restrict__ C,
                                                           KppState* __restrict__ st) {
  __shared__ double s_cen[kPpMaxK * 3];
  if (st->done) return;  // kernel-uniform
  for (int t = threadIdx.x; t < k * 3; t += kPpThreads) s_cen[t] = cen[t];
  __syncthreads();
  bool changed = false;
  KPP_CHUNK_LOOP(b) {
    double p[4][3];
    bool in[4];
    int l[4];
    kpp_load<D>(xc, n, b, lane, p, in);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = b * kChunk + lane * 4 + u;
      double d;
      const int best = kpp_nearest<D>(p[u], s_cen, k, &d);
      l[u] = in[u] ? best : -1;
      if (in[u]) {
        changed |= labels[i] != best;
        labels[i] = best;
      }
    }
    for (int c = 0; c < k; ++c) {
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double s = chunk_wave_sum(l[0] == c ? p[0][j] : 0.0, l[1] == c ? p[1][j] : 0.0,
                                        l[2] == c ? p[2][j] : 0.0, l[3] == c ? p[3][j] : 0.0);
        if (lane == 0) P[(int64_t(c) * D + j) * nch + b] = s;
      }
      const int cnt = __popcll(__ballot(l[0] == c)) + __popcll(__ballot(l[1] == c)) + __popcll(__ballot(l[2] == c)) +
                      __popcll(__ballot(l[3] == c));
      if (lane == 0) C[int64_t(c) * nch + b] = cnt;
    }
  }
  if (__any(changed) && (threadIdx.x & 63) == 0) atomicOr(&st->changed, 1);
}

// Block q < k * D: sums[q] = column q of P, its chunk totals added in chunk order. Block k * D + c:
// cnts[c] = members of centre c. One wave each.
__global__ __launch_bounds__(64) void k_kpp_colsums(const double* __restrict__ P, const int32_t* __restrict__ C,
                                                    int64_t nch, int kd, double* __restrict__ sums,
                                                    int64_t* __restrict__ cnts, const KppState* __restrict__ st,
                                                    int honour_done) {
  if (honour_done && st->done) return;
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q < kd) {
    const double s = wave_seq_total(P + int64_t(q) * nch, nch, lane);
    if (lane == 0) sums[q] = s;
    return;
  }
  const int32_t* col = C + int64_t(q - kd) * nch;
  int64_t cnt = 0;
  for (int64_t b = lane; b < nch; b += 64) cnt += col[b];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) cnt += __shfl_xor(cnt, off, 64);
  if (lane == 0) cnts[q - kd] = cnt;
}

// The centres move to their members' means (an empty one keeps its place); then scikit-learn's checks
// in its order: labels repeated -> strict convergence; summed squared shift <= tol_abs, or max_iter
// reached -> done, a final assignment follows.
__global__ __launch_bounds__(256) void k_kpp_update(const double* __restrict__ sums, const int64_t* __restrict__ cnts,
                                                    int k, int D, double* __restrict__ cen, KppState* __restrict__ st,
                                                    int max_iter) {
  __shared__ double s_d[kPpMaxK * 3];
  if (st->done) return;
  const int t = threadIdx.x;
  if (t < k * D) {
    const int c = t / D, j = t % D;
    const double old = cen[3 * c + j];
    const double nv = cnts[c] > 0 ? sums[t] / double(cnts[c]) : old;
    s_d[3 * c + j] = nv - old;
    cen[3 * c + j] = nv;
  }
  __syncthreads();
  if (t == 0) {
    double shift = 0.0;
    for (int c = 0; c < k; ++c) {
      double d = s_d[3 * c] * s_d[3 * c];
      if (D > 1) d = d + s_d[3 * c + 1] * s_d[3 * c + 1];
      if (D > 2) d = d + s_d[3 * c + 2] * s_d[3 * c + 2];
      shift = shift + d;
    }
    const int it = st->iter + 1;
    st->iter = it;
    if (!st->changed) {
      st->strict = 1;
      st->done = 1;
    } else if (shift <= st->tol_abs || it >= max_iter) {
      st->done = 1;
    }
    st->changed = 0;
  }
}

// After the loop: without strict convergence the points are assigned once more to the final centres.
// ip[b] = chunk sum of the squared distances to the labelled centres, C as in k_kpp_assign.
template <int D>
__global__ __launch_bounds__(kPpThreads) void k_kpp_final(const double* __restrict__ xc, int64_t n, int64_t nch, int k,
                                                          const double* __restrict__ cen, int32_t* __restrict__ labels,
                                                          double* __restrict__ ip, int32_t* __restrict__ C,
                                                          const KppState* __restrict__ st) {
  __shared__ double s_cen[kPpMaxK * 3];
  for (int t = threadIdx.x; t < k * 3; t += kPpThreads) s_cen[t] = cen[t];
  __syncthreads();
  const bool strict = st->strict != 0;
  KPP_CHUNK_LOOP(b) {
    double p[4][3], v[4];
    bool in[4];
    int l[4];
    kpp_load<D>(xc, n, b, lane, p, in);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = b * kChunk + lane * 4 + u;
      l[u] = -1;
      v[u] = 0.0;
      if (in[u]) {
        if (strict) {
          l[u] = labels[i];
        } else {
          double d;
          l[u] = kpp_nearest<D>(p[u], s_cen, k, &d);
          labels[i] = l[u];
        }
        v[u] = kpp_d2<D>(p[u], s_cen + 3 * l[u]);
      }
    }
    const double s = chunk_wave_sum(v[0], v[1], v[2], v[3]);
    if (lane == 0) ip[b] = s;
    for (int c = 0; c < k; ++c) {
      const int cnt = __popcll(__ballot(l[0] == c)) + __popcll(__ballot(l[1] == c)) + __popcll(__ballot(l[2] == c)) +
                      __popcll(__ballot(l[3] == c));
      if (lane == 0) C[int64_t(c) * nch + b] = cnt;
    }
  }
}

// inertia, the centres with mu added back, the centres without members: one wave
__global__ __launch_bounds__(64) void k_kpp_finish(const double* __restrict__ ip, int64_t nch,
                                                   const int64_t* __restrict__ cnts, int k, int D,
                                                   const double* __restrict__ cen, KppState* __restrict__ st,
                                                   double* __restrict__ cen_out) {
  const int lane = threadIdx.x;
  const double s = wave_seq_total(ip, nch, lane);
  for (int t = lane; t < k * D; t += 64) cen_out[t] = cen[3 * (t / D) + t % D] + st->mu[t % D];
  if (lane == 0) {
    int empty = 0;
    for (int c = 0; c < k; ++c) empty += cnts[c] == 0;
    st->inertia = s;
    st->n_empty = empty;
  }
}

static int kpp_trials(int k) { return 2 + int(std::log(double(k))); }

template <int D>
static int kmeans_pp_device(Ctx* c, const double* d_x, int64_t n, int k, int64_t first, const double* u, int max_iter,
                            double tol, int32_t* labels, double* centres, double* inertia, int32_t* n_iter,
                            int32_t* n_empty, int64_t* seeds) {
  const int64_t nch = (n + kChunk - 1) / kChunk;
  const int T = kpp_trials(k), kd = k * D;
  const int grid = int(std::min<int64_t>((nch + 3) / 4, int64_t(c->cu_count) * 8));
  const int64_t n_u = int64_t(k - 1) * T;
  double *d_xc, *d_part, *d_cen, *d_closest, *d_ct, *d_tp, *d_u, *d_P, *d_sums, *d_cen_out;
  int64_t *d_seeds, *d_cand, *d_cnts;
  int32_t *d_labels, *d_C;
  KppState* d_st;
  PQ_TRY(c->arena.get(size_t(n) * D, &d_xc));
  PQ_TRY(c->arena.get(size_t(nch) * 3, &d_part));
  PQ_TRY(c->arena.get(size_t(kPpMaxK) * 3, &d_cen));
  PQ_TRY(c->arena.get(size_t(n), &d_closest));
  PQ_TRY(c->arena.get(size_t(nch), &d_ct));
  PQ_TRY(c->arena.get(size_t(nch) * kPpMaxT, &d_tp));
  PQ_TRY(upload(c, u, size_t(n_u), &d_u));
  PQ_TRY(c->arena.get(size_t(nch) * kd, &d_P));
  PQ_TRY(c->arena.get(size_t(nch) * k, &d_C));
  PQ_TRY(c->arena.get(size_t(kd), &d_sums));
  PQ_TRY(c->arena.get(size_t(kd), &d_cen_out));
  PQ_TRY(c->arena.get(size_t(k), &d_cnts));
  PQ_TRY(c->arena.get(size_t(k), &d_seeds));
  PQ_TRY(c->arena.get(size_t(kPpMaxT), &d_cand));
  PQ_TRY(c->arena.get(size_t(n), &d_labels));
  PQ_TRY(c->arena.get(1, &d_st));
  PQ_HIP(hipMemsetAsync(d_st, 0, sizeof(KppState), c->stream));
  PQ_HIP(hipMemsetAsync(d_cen, 0, size_t(kPpMaxK) * 3 * sizeof(double), c->stream));
  PQ_HIP(hipMemsetAsync(d_labels, 0xFF, size_t(n) * sizeof(int32_t), c->stream));  // -1: no label yet
  {
    ProfScope ps(c, "kmeanspp_centre");
    hipLaunchKernelGGL(k_kpp_colsum<D>, dim3(grid), dim3(kPpThreads), 0, c->stream, d_x, n, nch, d_part);
    hipLaunchKernelGGL(k_kpp_mu, dim3(D), dim3(64), 0, c->stream, d_part, nch, n, d_st);
    hipLaunchKernelGGL(k_kpp_centre<D>, dim3(grid), dim3(kPpThreads), 0, c->stream, d_x, n, nch, d_st, d_xc, d_part);
    hipLaunchKernelGGL(k_kpp_tol, dim3(1), dim3(64 * D), 0, c->stream, d_part, nch, n, D, tol, first, d_xc, d_st,
                       d_cen, d_seeds);
    PQ_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "kmeanspp_seed");
    for (int ci = 1; ci < k; ++ci) {
      {
        ProfScope pk(c, "kmeanspp_closest", 1, 2);
        hipLaunchKernelGGL(k_kpp_closest<D>, dim3(grid), dim3(kPpThreads), 0, c->stream, d_xc, n, nch, d_cen, ci - 1,
                           int(ci == 1), d_closest, d_ct);
      }
      if (ci == 1) hipLaunchKernelGGL(k_kpp_pot, dim3(1), dim3(64), 0, c->stream, d_ct, nch, d_st);
      {
        ProfScope pk(c, "kmeanspp_pick", 1, 2);
        hipLaunchKernelGGL(k_kpp_pick, dim3(1), dim3(64), 0, c->stream, d_ct, nch, d_closest, n,
                           d_u + size_t(ci - 1) * T, T, d_st, d_cand);
      }
      {
        ProfScope pk(c, "kmeanspp_trial", 1, 2);
        hipLaunchKernelGGL(k_kpp_trial<D>, dim3(grid), dim3(kPpThreads), 0, c->stream, d_xc, n, nch, d_closest,
                           d_cand, T, d_tp);
      }
      {
        ProfScope pk(c, "kmeanspp_choose", 1, 2);
        hipLaunchKernelGGL(k_kpp_choose, dim3(1), dim3(64 * T), 0, c->stream, d_tp, nch, T, d_cand, d_xc, D, ci,
                           d_cen, d_seeds, d_st);
      }
      PQ_HIP(hipGetLastError());
    }
  }
  KppState h{};
  {
    ProfScope ps(c, "kmeanspp_lloyd");
    for (int queued = 0; queued < max_iter && !h.done;) {
      // bursts of 4, 4, 8, 16, 32, 32, ...: a run that converges at once queues few no-ops
      const int burst = std::min(std::min(kPpBurst, std::max(4, queued)), max_iter - queued);
      for (int it = 0; it < burst; ++it) {
        {
          ProfScope pk(c, "kmeanspp_assign", 1, 2);
          hipLaunchKernelGGL(k_kpp_assign<D>, dim3(grid), dim3(kPpThreads), 0, c->stream, d_xc, n, nch, k, d_cen,
                             d_labels, d_P, d_C, d_st);
        }
        {
          ProfScope pk(c, "kmeanspp_colsums", 1, 2);
          hipLaunchKernelGGL(k_kpp_colsums, dim3(kd + k), dim3(64), 0, c->stream, d_P, d_C, nch, kd, d_sums, d_cnts,
                             d_st, 1);
        }
        hipLaunchKernelGGL(k_kpp_update, dim3(1), dim3(256), 0, c->stream, d_sums, d_cnts, k, D, d_cen, d_st,
                           max_iter);
      }
      PQ_HIP(hipGetLastError());
      queued += burst;
      PQ_TRY(fetch(c, reinterpret_cast<char*>(&h), reinterpret_cast<const char*>(d_st), sizeof h));
    }
  }
  {
    ProfScope ps(c, "kmeanspp_final");
    hipLaunchKernelGGL(k_kpp_final<D>, dim3(grid), dim3(kPpThreads), 0, c->stream, d_xc, n, nch, k, d_cen, d_labels,
                       d_ct, d_C, d_st);
    hipLaunchKernelGGL(k_kpp_colsums, dim3(kd + k), dim3(64), 0, c->stream, d_P, d_C, nch, kd, d_sums, d_cnts, d_st,
                       0);
    hipLaunchKernelGGL(k_kpp_finish, dim3(1), dim3(64), 0, c->stream, d_ct, nch, d_cnts, k, D, d_cen, d_st,
                       d_cen_out);
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(download(c, labels, d_labels, size_t(n)));
  PQ_TRY(download(c, centres, d_cen_out, size_t(kd)));
  PQ_TRY(download(c, seeds, d_seeds, size_t(k)));
  PQ_TRY(fetch(c, reinterpret_cast<char*>(&h), reinterpret_cast<const char*>(d_st), sizeof h));
  *inertia = h.inertia;
  *n_iter = h.iter;
  *n_empty = h.n_empty;
  return 0;
}

static int kmeans_pp_check(const void* x, int64_t n, int32_t d, int32_t k, int64_t first, const double* u, int64_t n_u,
                           int32_t max_iter, double tol, const void* labels, const void* centres, const void* inertia,
                           const void* n_iter, const void* n_empty, const void* seeds) {
  if (d < 1 || d > 3) return fail(PYQSM_EINVAL, "pyqsm_kmeans_pp: d = %d, must be 1, 2 or 3", int(d));
  if (k < 1 || k > kPpMaxK) return fail(PYQSM_EINVAL, "pyqsm_kmeans_pp: k = %d, must be in [1, %d]", int(k), kPpMaxK);
  if (n < k) return fail(PYQSM_EINVAL, "pyqsm_kmeans_pp: %lld points for %d centres", (long long)n, int(k));
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  if (!x || !labels || !centres || !inertia || !n_iter || !n_empty || !seeds)
    return fail(PYQSM_EINVAL, "pyqsm_kmeans_pp: NULL pointer");
  if (first < 0 || first >= n) return fail(PYQSM_EINVAL, "pyqsm_kmeans_pp: first index outside [0, n)");
  if (n_u != int64_t(k - 1) * kpp_trials(k) || (n_u > 0 && !u))
    return fail(PYQSM_EINVAL, "pyqsm_kmeans_pp: %lld uniforms, (k - 1) (2 + int(ln k)) = %lld are needed",
                (long long)n_u, (long long)(int64_t(k - 1) * kpp_trials(k)));
  for (int64_t i = 0; i < n_u; ++i)
    if (!(u[i] >= 0.0 && u[i] < 1.0)) return fail(PYQSM_EINVAL, "pyqsm_kmeans_pp: a uniform outside [0, 1)");
  if (max_iter < 1) return fail(PYQSM_EINVAL, "max_iter must be >= 1");
  if (!(tol >= 0.0)) return fail(PYQSM_EINVAL, "tol must be >= 0");
  return 0;
}

static int kmeans_pp_dispatch(Ctx* c, const double* d_x, int64_t n, int d, int k, int64_t first, const double* u,
                              int max_iter, double tol, int32_t* labels, double* centres, double* inertia,
                              int32_t* n_iter, int32_t* n_empty, int64_t* seeds) {
  if (d == 1)
    return kmeans_pp_device<1>(c, d_x, n, k, first, u, max_iter, tol, labels, centres, inertia, n_iter, n_empty, seeds);
  if (d == 2)
    return kmeans_pp_device<2>(c, d_x, n, k, first, u, max_iter, tol, labels, centres, inertia, n_iter, n_empty, seeds);
  return kmeans_pp_device<3>(c, d_x, n, k, first, u, max_iter, tol, labels, centres, inertia, n_iter, n_empty, seeds);
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_select_values_dev(const double* v_dev, int64_t n, int32_t width, int32_t key, const int64_t* ranks,
                            int32_t n_ranks, double* values, int32_t device) {
  PQ_API_RANGE("pyqsm_select_values");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  PQ_TRY(check_key(width, key, "pyqsm_select_values"));
  if (n_ranks < 0 || n_ranks > kSelMaxRanks)
    return fail(PYQSM_EINVAL, "pyqsm_select_values: %d ranks, at most %d", int(n_ranks), kSelMaxRanks);
  if (n_ranks > 0 && (!ranks || !values)) return fail(PYQSM_EINVAL, "pyqsm_select_values: NULL pointer");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 rows per call");
  if (n == 0) {  // answered on the host: there is no rank to give
    for (int r = 0; r < n_ranks; ++r) {
      if (ranks[r] >= 0) return fail(PYQSM_EINVAL, "rank %lld of 0 keys", (long long)ranks[r]);
      values[r] = 0.0;
    }
    return 0;
  }
  if (!v_dev) return fail(PYQSM_EINVAL, "pyqsm_select_values: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  return select_device(c, v_dev, n, width, key, ranks, n_ranks, values);
}

int pyqsm_select_values(const double* v, int64_t n, int32_t width, int32_t key, const int64_t* ranks, int32_t n_ranks,
                        double* values, int32_t device) {
  PQ_API_RANGE("pyqsm_select_values");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  PQ_TRY(check_key(width, key, "pyqsm_select_values"));
  if (n_ranks < 0 || n_ranks > kSelMaxRanks)
    return fail(PYQSM_EINVAL, "pyqsm_select_values: %d ranks, at most %d", int(n_ranks), kSelMaxRanks);
  if (n_ranks > 0 && (!ranks || !values)) return fail(PYQSM_EINVAL, "pyqsm_select_values: NULL pointer");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 rows per call");
  if (n == 0) {
    for (int r = 0; r < n_ranks; ++r) {
      if (ranks[r] >= 0) return fail(PYQSM_EINVAL, "rank %lld of 0 keys", (long long)ranks[r]);
      values[r] = 0.0;
    }
    return 0;
  }
  if (!v) return fail(PYQSM_EINVAL, "pyqsm_select_values: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_v;
  PQ_TRY(upload(c, v, size_t(n) * width, &d_v));
  return select_device(c, d_v, n, width, key, ranks, n_ranks, values);
}

int pyqsm_split_above_dev(const double* v_dev, int64_t n, int32_t width, int32_t key, int32_t cmp, double threshold,
                          const double* rows_dev, int64_t* idx_dev, double* out_rows_dev, int64_t* count,
                          int32_t device) {
  PQ_API_RANGE("pyqsm_split_above");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!count) return fail(PYQSM_EINVAL, "pyqsm_split_above_dev: NULL pointer");
  *count = 0;
  PQ_TRY(check_key(width, key, "pyqsm_split_above_dev"));
  if (cmp < kCmpGt || cmp > kCmpLe) return fail(PYQSM_EINVAL, "pyqsm_split_above_dev: comparison %d", int(cmp));
  if (threshold != threshold) return fail(PYQSM_EINVAL, "pyqsm_split_above_dev: the threshold is NaN");
  if (n == 0) return 0;
  if (!v_dev || (rows_dev && !out_rows_dev)) return fail(PYQSM_EINVAL, "pyqsm_split_above_dev: NULL pointer");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 rows per call");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  int32_t* d_flags;
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_flags));
  {
    ProfScope ps(c, "split_above");
    hipLaunchKernelGGL(k_split_flags, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, v_dev, n, int(width),
                       int(key), int(cmp), threshold, d_flags);
    PQ_HIP(hipGetLastError());
    PQ_TRY(compact_flagged(c, d_flags, n, idx_dev, nullptr, rows_dev, rows_dev ? out_rows_dev : nullptr));
  }
  int32_t total = 0;
  PQ_TRY(fetch(c, &total, d_flags + n));
  *count = total;
  return 0;
}

int pyqsm_shift_components_dev(const double* shift_dev, int64_t n, double q_mag, double q_z, uint8_t* labels_dev,
                               double* thresholds, int64_t* counts, int32_t device) {
  PQ_API_RANGE("pyqsm_shift_components");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!thresholds || !counts) return fail(PYQSM_EINVAL, "pyqsm_shift_components: NULL pointer");
  if (bad_percentile(q_mag) || bad_percentile(q_z)) return fail(PYQSM_EINVAL, "percentiles must be in [0, 100]");
  thresholds[0] = thresholds[1] = std::nan("");
  counts[0] = counts[1] = counts[2] = 0;
  if (n == 0) return 0;
  if (!shift_dev || !labels_dev) return fail(PYQSM_EINVAL, "pyqsm_shift_components: NULL pointer");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 rows per call");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  return shift_components_device(c, shift_dev, n, q_mag, q_z, labels_dev, thresholds, counts);
}

int pyqsm_shift_components(const double* shift, int64_t n, double q_mag, double q_z, uint8_t* labels,
                           double* thresholds, int64_t* counts, int32_t device) {
  PQ_API_RANGE("pyqsm_shift_components");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!thresholds || !counts) return fail(PYQSM_EINVAL, "pyqsm_shift_components: NULL pointer");
  if (bad_percentile(q_mag) || bad_percentile(q_z)) return fail(PYQSM_EINVAL, "percentiles must be in [0, 100]");
  thresholds[0] = thresholds[1] = std::nan("");
  counts[0] = counts[1] = counts[2] = 0;
  if (n == 0) return 0;
  if (!shift || !labels) return fail(PYQSM_EINVAL, "pyqsm_shift_components: NULL pointer");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 rows per call");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_shift;
  uint8_t* d_labels;
  PQ_TRY(upload(c, shift, size_t(n) * 3, &d_shift));
  PQ_TRY(c->arena.get(size_t(n), &d_labels));
  PQ_TRY(shift_components_device(c, d_shift, n, q_mag, q_z, d_labels, thresholds, counts));
  return fetch(c, labels, d_labels, size_t(n));
}

int pyqsm_kmeans_pp_dev(const double* x_dev, int64_t n, int32_t d, int32_t k, int64_t first, const double* u,
                        int64_t n_u, int32_t max_iter, double tol, int32_t* labels, double* centres, double* inertia,
                        int32_t* n_iter, int32_t* n_empty, int64_t* seeds, int32_t device) {
  PQ_API_RANGE("pyqsm_kmeans_pp");
  PQ_TRY(kmeans_pp_check(x_dev, n, d, k, first, u, n_u, max_iter, tol, labels, centres, inertia, n_iter, n_empty,
                         seeds));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  return kmeans_pp_dispatch(c, x_dev, n, d, k, first, u, max_iter, tol, labels, centres, inertia, n_iter, n_empty,
                            seeds);
}

int pyqsm_kmeans_pp(const double* x, int64_t n, int32_t d, int32_t k, int64_t first, const double* u, int64_t n_u,
                    int32_t max_iter, double tol, int32_t* labels, double* centres, double* inertia, int32_t* n_iter,
                    int32_t* n_empty, int64_t* seeds, int32_t device) {
  PQ_API_RANGE("pyqsm_kmeans_pp");
  PQ_TRY(kmeans_pp_check(x, n, d, k, first, u, n_u, max_iter, tol, labels, centres, inertia, n_iter, n_empty, seeds));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_x;
  PQ_TRY(upload(c, x, size_t(n) * d, &d_x));
  return kmeans_pp_dispatch(c, d_x, n, d, k, first, u, max_iter, tol, labels, centres, inertia, n_iter, n_empty, seeds);
}

}  // extern "C"
