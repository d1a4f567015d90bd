// kmeans.hip — the clustering and ball-stepping kernels of branch tracing:
// pyQSM's sphere_step (qsm_generation.py:182-316) and the kmeans it reaches through
// choose_and_cluster (math_utils/fit.py:58-85, 168-214).
//
//   Lloyd k-means    scipy.cluster.vq.kmeans2(data, k, iter, minit='matrix') on the xy of m points:
//                    one workgroup per labelling runs every iteration (k <= 8). vq labels by the
//                    squared distance dx*dx + dy*dy, ties to the lowest centroid; the centroid is
//                    the mean of its members, an empty one keeps its place; the labels returned are
//                    those of the last assignment, before the last update.
//   silhouette       sklearn.metrics.silhouette_score of m 3-D points: the labellings are grouped by
//                    label with the reproducible radix sort of scan.hip, then one lane per point
//                    walks every cluster's members in ascending index order, staged 256 at a time in
//                    LDS, summing sqrt(((dx*dx) + dy*dy) + dz*dz) one add at a time. fp64 bound.
//   ball step        the points within r of a centre (d2 <= r2, pyqsm_ball_query's bound) that the
//                    HBM `found` mask does not hold, compacted by scan to ascending indices and
//                    gathered into a contiguous xyz buffer (the input of DBSCAN and k-means).
//
// Every sum has a fixed order and there are no float atomics: the results are the same bits on
// every run. "Chunk sum" below is the one reduction used for the centroid sums and the mean
// silhouette: 256 consecutive values per chunk, lane l of a wave holding values 4l..4l+3 summed
// as ((v0 + v1) + v2) + v3, then an xor butterfly over the 64 lanes (pairs of neighbours first);
// the chunk totals are added one at a time from 0.0 in chunk order.
#include "grid.hpp"  // sqdist3
#include "reduce.hpp"  // chunk_wave_sum, kChunk

#include <cmath>

namespace pyqsm {

static constexpr int kKmMaxK = PYQSM_KMEANS_MAX_K;  // centroids per labelling
static constexpr int kLloydThreads = 1024;          // one workgroup per labelling
static constexpr int kSilTile = 256;                // points staged per LDS tile
static constexpr int kSilThreads = 64;              // one wave per block of 64 query points

// ---------------------------------------------------------------- Lloyd

// Block q: labelling q with ks[q] centroids, initial centroids init[q][c][0..1]. Each iteration is
// one pass over the points in chunks of 256 (one wave per chunk, four consecutive points per lane):
// label, store the label, and write the chunk's per-centroid sums of x and y and member counts
// into part / pcnt; after a barrier 2k lanes add the chunk totals in chunk order and divide.
__global__ __launch_bounds__(kLloydThreads) void k_lloyd(const double* __restrict__ xyz, int64_t m,
                                                         const int32_t* __restrict__ ks,
                                                         const double* __restrict__ init, int32_t iters,
                                                         int32_t* __restrict__ labels,
                                                         double* __restrict__ cent_out,
                                                         double* __restrict__ part,
                                                         int32_t* __restrict__ pcnt) {
  __shared__ double cen[kKmMaxK][2];
  const int q = blockIdx.x;
  const int k = ks[q];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, nw = blockDim.x >> 6;
  const int64_t nch = (m + kChunk - 1) / kChunk;
  int32_t* lab = labels + int64_t(q) * m;
  double* P = part + int64_t(q) * nch * kKmMaxK * 2;
  int32_t* C = pcnt + int64_t(q) * nch * kKmMaxK;
  if (t < 2 * k) cen[t >> 1][t & 1] = init[(int64_t(q) * kKmMaxK + (t >> 1)) * 2 + (t & 1)];
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    for (int64_t b = w; b < nch; b += nw) {
      double x[4], y[4];
      int l[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = b * kChunk + lane * 4 + u;
        const bool in = i < m;
        x[u] = in ? xyz[3 * i] : 0.0;
        y[u] = in ? xyz[3 * i + 1] : 0.0;
        int best = 0;
        double bd = 0.0;
        for (int c = 0; c < k; ++c) {
          const double dx = x[u] - cen[c][0], dy = y[u] - cen[c][1];
          double d = dx * dx;
          d = d + dy * dy;
          if (c == 0 || d < bd) {
            bd = d;
            best = c;
          }
        }
        l[u] = in ? best : -1;
        if (in) lab[i] = best;
      }
#pragma unroll
      for (int c = 0; c < kKmMaxK; ++c) {
        if (c >= k) break;
        const double sx = chunk_wave_sum(l[0] == c ? x[0] : 0.0, l[1] == c ? x[1] : 0.0,
                                         l[2] == c ? x[2] : 0.0, l[3] == c ? x[3] : 0.0);
        const double sy = chunk_wave_sum(l[0] == c ? y[0] : 0.0, l[1] == c ? y[1] : 0.0,
                                         l[2] == c ? y[2] : 0.0, l[3] == c ? y[3] : 0.0);
        const int cnt = __popcll(__ballot(l[0] == c)) + __popcll(__ballot(l[1] == c)) +
                        __popcll(__ballot(l[2] == c)) + __popcll(__ballot(l[3] == c));
        if (lane == 0) {
          P[(b * kKmMaxK + c) * 2] = sx;
          P[(b * kKmMaxK + c) * 2 + 1] = sy;
          C[b * kKmMaxK + c] = cnt;
        }
      }
    }
    __syncthreads();
    double nv = 0.0;
    if (t < 2 * k) {
      const int c = t >> 1, d = t & 1;
      double s = 0.0;
      int64_t cnt = 0;
      int64_t b = 0;
      for (; b + 8 <= nch; b += 8) {  // eight loads in flight, added in order
        double v[8];
        int32_t n8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          v[u] = P[((b + u) * kKmMaxK + c) * 2 + d];
          n8[u] = C[(b + u) * kKmMaxK + c];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          s = s + v[u];
          cnt += n8[u];
        }
      }
      for (; b < nch; ++b) {
        s = s + P[(b * kKmMaxK + c) * 2 + d];
        cnt += C[b * kKmMaxK + c];
      }
      nv = cnt > 0 ? s / double(cnt) : cen[c][d];
    }
    __syncthreads();
    if (t < 2 * k) cen[t >> 1][t & 1] = nv;
    __syncthreads();
  }
  if (t < 2 * k) cent_out[(int64_t(q) * kKmMaxK + (t >> 1)) * 2 + (t & 1)] = cen[t >> 1][t & 1];
}

// ---------------------------------------------------------------- silhouette

// keys[q*m + i] = q * kmax + labels[q*m + i], vals = q*m + i: after the stable sort every cluster of
// every labelling is one run of ascending point indices.
__global__ __launch_bounds__(256) void k_sil_keys(const int32_t* __restrict__ labels, int64_t total,
                                                  int64_t m, int32_t kmax, uint32_t* __restrict__ keys,
                                                  int32_t* __restrict__ vals) {
  const int64_t g = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (g >= total) return;
  keys[g] = uint32_t((g / m) * kmax + labels[g]);
  vals[g] = int32_t(g);
}

// The points in sorted order (x, y, z, 0) and the run bounds: off[s] = first sorted position whose
// key is >= s, for s = 0 .. nseg (off[nseg] = total).
__global__ __launch_bounds__(256) void k_sil_gather(const double* __restrict__ xyz, int64_t m, int64_t total,
                                                    const int32_t* __restrict__ vals,
                                                    double4* __restrict__ sorted) {
  const int64_t p = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (p >= total) return;
  const int64_t i = int64_t(vals[p]) % m;
  sorted[p] = make_double4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.0);
}

__global__ __launch_bounds__(256) void k_sil_bounds(const uint32_t* __restrict__ keys, int64_t total,
                                                    int32_t nseg, int64_t* __restrict__ off) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > nseg) return;
  int64_t lo = 0, hi = total;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < uint32_t(s)) lo = mid + 1;
    else hi = mid;
  }
  off[s] = lo;
}

__device__ __forceinline__ int present_labels(const int64_t* off, int k) {
  int p = 0;
  for (int c = 0; c < k; ++c) p += off[c + 1] > off[c];
  return p;
}

// Block (x, q): query points i = 64 x + lane of labelling q. For every cluster c in order, its
// members are staged 256 at a time in LDS and every lane adds its distances to them one at a time
// from 0.0 (ascending member index). a = own sum / (n_own - 1); b = min over the other non-empty
// clusters of sum / n_c; s = (b - a) / max(a, b), 0 for a singleton and for 0/0. A labelling with
// fewer than 2 or more than m - 1 labels present is invalid: s = 0 everywhere.
__global__ __launch_bounds__(kSilThreads) void k_silhouette(const double* __restrict__ xyz, int64_t m,
                                                            const int32_t* __restrict__ labels,
                                                            const int32_t* __restrict__ ks, int32_t kmax,
                                                            const double4* __restrict__ sorted,
                                                            const int64_t* __restrict__ off_all,
                                                            double* __restrict__ samples) {
  __shared__ double4 tile[kSilTile];
  const int q = blockIdx.y;
  const int k = ks[q];
  const int64_t* off = off_all + int64_t(q) * kmax;
  const int64_t i = int64_t(blockIdx.x) * kSilThreads + threadIdx.x;
  const bool live = i < m;
  const int present = present_labels(off, k);
  if (present < 2 || present > m - 1) {
    if (live) samples[int64_t(q) * m + i] = 0.0;
    return;  // uniform over the block
  }
  const int own = live ? labels[int64_t(q) * m + i] : -1;
  const double xi = live ? xyz[3 * i] : 0.0, yi = live ? xyz[3 * i + 1] : 0.0,
               zi = live ? xyz[3 * i + 2] : 0.0;
  double a_sum = 0.0, b = __builtin_inf();
  int64_t n_own = 0;
  for (int c = 0; c < k; ++c) {
    const int64_t beg = off[c], end = off[c + 1];
    if (end == beg) continue;
    double acc = 0.0;
    for (int64_t t0 = beg; t0 < end; t0 += kSilTile) {
      const int len = int(end - t0 < kSilTile ? end - t0 : kSilTile);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kSilTile / kSilThreads; ++u) {
        const int j = u * kSilThreads + threadIdx.x;
        if (j < len) tile[j] = sorted[t0 + j];
      }
      __syncthreads();
      int j = 0;
      for (; j + 4 <= len; j += 4) {
        double d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double4 p = tile[j + u];
          const double dx = xi - p.x, dy = yi - p.y, dz = zi - p.z;
          double d2 = dx * dx;
          d2 = d2 + dy * dy;
          d2 = d2 + dz * dz;
          d[u] = sqrt(d2);
        }
        acc = acc + d[0];
        acc = acc + d[1];
        acc = acc + d[2];
        acc = acc + d[3];
      }
      for (; j < len; ++j) {
        const double4 p = tile[j];
        const double dx = xi - p.x, dy = yi - p.y, dz = zi - p.z;
        double d2 = dx * dx;
        d2 = d2 + dy * dy;
        d2 = d2 + dz * dz;
        acc = acc + sqrt(d2);
      }
    }
    const int64_t nc = end - beg;
    if (c == own) {
      a_sum = acc;
      n_own = nc;
    } else {
      const double mean = acc / double(nc);
      b = mean < b ? mean : b;
    }
  }
  if (!live) return;
  double s = 0.0;
  if (n_own > 1) {
    const double a = a_sum / double(n_own - 1);
    s = (b - a) / (a > b ? a : b);
    if (s != s) s = 0.0;
  }
  samples[int64_t(q) * m + i] = s;
}

// One wave per labelling: the chunk sum of its m samples over m; present labels alongside.
__global__ __launch_bounds__(64) void k_sil_mean(const double* __restrict__ samples, int64_t m,
                                                 const int32_t* __restrict__ ks, int32_t kmax,
                                                 const int64_t* __restrict__ off_all,
                                                 double* __restrict__ scores, int32_t* __restrict__ present) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const double* s = samples + int64_t(q) * m;
  double total = 0.0;
  for (int64_t b = 0; b * kChunk < m; ++b) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = b * kChunk + lane * 4 + u;
      v[u] = i < m ? s[i] : 0.0;
    }
    total = total + chunk_wave_sum(v[0], v[1], v[2], v[3]);
  }
  if (lane == 0) {
    scores[q] = total / double(m);
    present[q] = present_labels(off_all + int64_t(q) * kmax, ks[q]);
  }
}

// ---------------------------------------------------------------- ball step

__global__ __launch_bounds__(256) void k_ball_excl_flags(int64_t n, const double* __restrict__ xyz,
                                                         const uint8_t* __restrict__ found, double cx,
                                                         double cy, double cz, double r2,
                                                         int32_t* __restrict__ flags) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i > n) return;
  int32_t f = 0;
  if (i < n && !found[i]) {
    f = sqdist3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, cz) <= r2;
  }
  flags[i] = f;
}

__global__ __launch_bounds__(256) void k_mark_found(uint8_t* __restrict__ found, int64_t n,
                                                    const int64_t* __restrict__ idx, int64_t cnt) {
  const int64_t j = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (j >= cnt) return;
  const int64_t i = idx[j];
  if (i >= 0 && i < n) found[i] = 1;
}

// ---------------------------------------------------------------- drivers

static int check_ks(const int32_t* ks, int32_t nq) {
  if (nq < 1 || nq > PYQSM_KMEANS_MAX_Q) return fail(PYQSM_ERANGE, "between 1 and %d labellings per call", PYQSM_KMEANS_MAX_Q);
  for (int q = 0; q < nq; ++q)
    if (ks[q] < 1 || ks[q] > kKmMaxK) return fail(PYQSM_ERANGE, "k must be in [1, %d]", kKmMaxK);
  return 0;
}

// Lloyd for nq labellings of the same m points: init host [nq][k_q][2] packed; d_labels [nq][m]
// device; cent host [nq][k_q][2] packed or NULL (then no read-back and no synchronisation).
static int lloyd_device(Ctx* c, const double* d_xyz, int64_t m, const int32_t* ks, int32_t nq,
                        int32_t iters, const double* init, int32_t* d_labels, int32_t** d_ks_out,
                        double* cent) {
  const int64_t nch = (m + kChunk - 1) / kChunk;
  std::vector<double> init_pad(size_t(nq) * kKmMaxK * 2, 0.0);
  for (int q = 0, o = 0; q < nq; o += ks[q], ++q)
    for (int j = 0; j < ks[q] * 2; ++j) init_pad[size_t(q) * kKmMaxK * 2 + j] = init[size_t(o) * 2 + j];
  double *d_init, *d_cent, *d_part;
  int32_t *d_ks, *d_pcnt;
  PQ_TRY(c->arena.get(init_pad.size(), &d_init));
  PQ_TRY(c->arena.get(init_pad.size(), &d_cent));
  PQ_TRY(c->arena.get(size_t(nq) * nch * kKmMaxK * 2, &d_part));
  PQ_TRY(c->arena.get(size_t(nq) * nch * kKmMaxK, &d_pcnt));
  PQ_TRY(c->arena.get(size_t(nq), &d_ks));
  PQ_TRY(copy_in(c, d_init, init_pad.data(), init_pad.size()));
  PQ_TRY(copy_in(c, d_ks, ks, size_t(nq)));
  {
    ProfScope ps(c, "kmeans_lloyd");
    hipLaunchKernelGGL(k_lloyd, dim3(nq), dim3(kLloydThreads), 0, c->stream, d_xyz, m, d_ks, d_init, iters,
                       d_labels, d_cent, d_part, d_pcnt);
    PQ_HIP(hipGetLastError());
  }
  if (d_ks_out) *d_ks_out = d_ks;
  if (cent) {
    PQ_TRY(fetch(c, init_pad.data(), d_cent, init_pad.size()));
    for (int q = 0, o = 0; q < nq; o += ks[q], ++q)
      for (int j = 0; j < ks[q] * 2; ++j) cent[size_t(o) * 2 + j] = init_pad[size_t(q) * kKmMaxK * 2 + j];
  }
  return 0;
}

// Silhouettes of nq labellings (d_labels [nq][m], label counts d_ks) of the same m points:
// d_samples [nq][m], d_scores [nq], d_present [nq], all device. Asynchronous.
static int silhouette_device(Ctx* c, const double* d_xyz, int64_t m, const int32_t* d_labels,
                             const int32_t* d_ks, int32_t nq, int32_t kmax, double* d_samples,
                             double* d_scores, int32_t* d_present) {
  const int64_t total = int64_t(nq) * m;
  const int nseg = nq * kmax;
  uint32_t* d_keys;
  int32_t* d_vals;
  double4* d_sorted;
  int64_t* d_off;
  PQ_TRY(c->arena.get(size_t(total), &d_keys));
  PQ_TRY(c->arena.get(size_t(total), &d_vals));
  PQ_TRY(c->arena.get(size_t(total), &d_sorted));
  PQ_TRY(c->arena.get(size_t(nseg) + 1, &d_off));
  int bits = 1;
  while ((1 << bits) < nseg) ++bits;
  {
    ProfScope ps(c, "silhouette_group");
    hipLaunchKernelGGL(k_sil_keys, dim3(ceil_div(total, 256)), dim3(256), 0, c->stream, d_labels, total, m,
                       kmax, d_keys, d_vals);
    PQ_TRY(stable_sort_pairs_u32(c, &d_keys, &d_vals, total, bits));
    hipLaunchKernelGGL(k_sil_gather, dim3(ceil_div(total, 256)), dim3(256), 0, c->stream, d_xyz, m, total,
                       d_vals, d_sorted);
    hipLaunchKernelGGL(k_sil_bounds, dim3(ceil_div(nseg + 1, 256)), dim3(256), 0, c->stream, d_keys, total,
                       nseg, d_off);
    PQ_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "silhouette");
    hipLaunchKernelGGL(k_silhouette, dim3(ceil_div(m, kSilThreads), nq), dim3(kSilThreads), 0, c->stream,
                       d_xyz, m, d_labels, d_ks, kmax, d_sorted, d_off, d_samples);
    hipLaunchKernelGGL(k_sil_mean, dim3(nq), dim3(64), 0, c->stream, d_samples, m, d_ks, kmax, d_off,
                       d_scores, d_present);
    PQ_HIP(hipGetLastError());
  }
  return 0;
}

static int upload_points(Ctx* c, const double* xyz, int64_t m, double** d_xyz) {
  return upload(c, xyz, size_t(m) * 3, d_xyz);
}

static int kmeans_select_impl(Ctx* c, const double* d_xyz, int64_t m, int32_t k0, int32_t nk, int32_t iters,
                              const double* init, int32_t* labels, double* scores, int32_t* present) {
  std::vector<int32_t> ks(nk);
  for (int q = 0; q < nk; ++q) ks[q] = k0 + q;
  PQ_TRY(check_ks(ks.data(), nk));
  // one device block for the read-back: scores [nk] f64, present [nk] i32 (padded), labels [nk][m] i32
  const size_t head = size_t(nk) * 8 + ((size_t(nk) * 4 + 7) & ~size_t(7));
  const size_t bytes = head + size_t(nk) * m * 4;
  char* d_out;
  double* d_samples;
  int32_t* d_ks;
  PQ_TRY(c->arena.alloc(bytes, reinterpret_cast<void**>(&d_out)));
  PQ_TRY(c->arena.get(size_t(nk) * m, &d_samples));
  double* d_scores = reinterpret_cast<double*>(d_out);
  int32_t* d_present = reinterpret_cast<int32_t*>(d_out + size_t(nk) * 8);
  int32_t* d_labels = reinterpret_cast<int32_t*>(d_out + head);
  PQ_TRY(lloyd_device(c, d_xyz, m, ks.data(), nk, iters, init, d_labels, &d_ks, nullptr));
  PQ_TRY(silhouette_device(c, d_xyz, m, d_labels, d_ks, nk, kKmMaxK, d_samples, d_scores, d_present));
  std::vector<char> h(bytes);
  PQ_TRY(fetch(c, h.data(), d_out, bytes));
  memcpy(scores, h.data(), size_t(nk) * 8);
  memcpy(present, h.data() + size_t(nk) * 8, size_t(nk) * 4);
  memcpy(labels, h.data() + head, size_t(nk) * m * 4);
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_kmeans(const double* xyz, int64_t m, int32_t k, int32_t iters, const double* init,
                 double* centroids, int32_t* labels, int32_t device) {
  PQ_API_RANGE("pyqsm_kmeans");
  if (m < 1) return fail(PYQSM_EINVAL, "k-means needs at least one point");
  if (!xyz || !init || !centroids || !labels) return fail(PYQSM_EINVAL, "pyqsm_kmeans: NULL pointer");
  if (iters < 1) return fail(PYQSM_EINVAL, "iters must be >= 1");
  if (m > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  PQ_TRY(check_ks(&k, 1));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_xyz;
  int32_t* d_lab;
  PQ_TRY(upload_points(c, xyz, m, &d_xyz));
  PQ_TRY(c->arena.get(size_t(m), &d_lab));
  PQ_TRY(lloyd_device(c, d_xyz, m, &k, 1, iters, init, d_lab, nullptr, centroids));
  PQ_TRY(fetch(c, labels, d_lab, size_t(m)));
  return 0;
}

int pyqsm_silhouette(const double* xyz, int64_t m, const int32_t* labels, int32_t k, double* score,
                     int32_t* n_present, double* samples, int32_t device) {
  PQ_API_RANGE("pyqsm_silhouette");
  if (m < 1) return fail(PYQSM_EINVAL, "silhouette needs at least one point");
  if (!xyz || !labels || !score || !n_present) return fail(PYQSM_EINVAL, "pyqsm_silhouette: NULL pointer");
  if (k < 1 || k > PYQSM_SILHOUETTE_MAX_K) return fail(PYQSM_ERANGE, "k must be in [1, %d]", PYQSM_SILHOUETTE_MAX_K);
  if (m > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  for (int64_t i = 0; i < m; ++i)
    if (labels[i] < 0 || labels[i] >= k) return fail(PYQSM_EINVAL, "label outside [0, k)");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_xyz, *d_samples, *d_score;
  int32_t *d_lab, *d_ks, *d_present;
  PQ_TRY(upload_points(c, xyz, m, &d_xyz));
  PQ_TRY(c->arena.get(size_t(m), &d_lab));
  PQ_TRY(c->arena.get(size_t(m), &d_samples));
  PQ_TRY(c->arena.get(1, &d_score));
  PQ_TRY(c->arena.get(1, &d_present));
  PQ_TRY(c->arena.get(1, &d_ks));
  PQ_TRY(copy_in(c, d_lab, labels, size_t(m)));
  PQ_TRY(copy_in(c, d_ks, &k, 1));
  PQ_TRY(silhouette_device(c, d_xyz, m, d_lab, d_ks, 1, k, d_samples, d_score, d_present));
  PQ_TRY(download(c, score, d_score, 1));
  PQ_TRY(download(c, n_present, d_present, 1));
  if (samples) PQ_TRY(download(c, samples, d_samples, size_t(m)));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int pyqsm_kmeans_select_dev(const double* xyz_dev, int64_t m, int32_t k0, int32_t nk, int32_t iters,
                            const double* init, int32_t* labels, double* scores, int32_t* present,
                            int32_t device) {
  PQ_API_RANGE("pyqsm_kmeans_select");
  if (m < 1) return fail(PYQSM_EINVAL, "k-means needs at least one point");
  if (!xyz_dev || !init || !labels || !scores || !present)
    return fail(PYQSM_EINVAL, "pyqsm_kmeans_select: NULL pointer");
  if (iters < 1) return fail(PYQSM_EINVAL, "iters must be >= 1");
  if (m > 0x7FFFFF00LL / PYQSM_KMEANS_MAX_Q) return fail(PYQSM_ERANGE, "too many points per call");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  ProfScope ps(c, "kmeans_select");
  return kmeans_select_impl(c, xyz_dev, m, k0, nk, iters, init, labels, scores, present);
}

int pyqsm_kmeans_select(const double* xyz, int64_t m, int32_t k0, int32_t nk, int32_t iters,
                        const double* init, int32_t* labels, double* scores, int32_t* present,
                        int32_t device) {
  PQ_API_RANGE("pyqsm_kmeans_select");
  if (m < 1) return fail(PYQSM_EINVAL, "k-means needs at least one point");
  if (!xyz || !init || !labels || !scores || !present)
    return fail(PYQSM_EINVAL, "pyqsm_kmeans_select: NULL pointer");
  if (iters < 1) return fail(PYQSM_EINVAL, "iters must be >= 1");
  if (m > 0x7FFFFF00LL / PYQSM_KMEANS_MAX_Q) return fail(PYQSM_ERANGE, "too many points per call");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_xyz;
  PQ_TRY(upload_points(c, xyz, m, &d_xyz));
  return kmeans_select_impl(c, d_xyz, m, k0, nk, iters, init, labels, scores, present);
}

int pyqsm_ball_excl_dev(const double* xyz_dev, int64_t n, const uint8_t* found_dev, const double center[3],
                        double radius, int64_t* idx_dev, double* out_xyz_dev, int64_t* count,
                        int32_t device) {
  PQ_API_RANGE("pyqsm_ball_excl");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (!count || !center) return fail(PYQSM_EINVAL, "pyqsm_ball_excl_dev: NULL pointer");
  *count = 0;
  if (n == 0) return 0;
  if (!xyz_dev || !found_dev || !idx_dev || !out_xyz_dev)
    return fail(PYQSM_EINVAL, "pyqsm_ball_excl_dev: NULL pointer");
  if (!(radius >= 0)) return fail(PYQSM_EINVAL, "radius must be >= 0");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  int32_t* d_flags;
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_flags));
  {
    ProfScope ps(c, "ball_excl");
    hipLaunchKernelGGL(k_ball_excl_flags, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, n, xyz_dev,
                       found_dev, center[0], center[1], center[2], radius * radius, d_flags);
    PQ_TRY(compact_flagged(c, d_flags, n, idx_dev, nullptr, xyz_dev, out_xyz_dev));
  }
  int32_t total = 0;
  PQ_TRY(fetch(c, &total, d_flags + n));
  *count = total;
  return 0;
}

int pyqsm_mark_found_dev(uint8_t* found_dev, int64_t n, const int64_t* idx, int64_t cnt, int32_t device) {
  PQ_API_RANGE("pyqsm_mark_found");
  if (n < 0 || cnt < 0) return fail(PYQSM_EINVAL, "negative size");
  if (cnt == 0) return 0;
  if (!found_dev || !idx) return fail(PYQSM_EINVAL, "pyqsm_mark_found_dev: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  int64_t* d_idx;
  PQ_TRY(upload(c, idx, size_t(cnt), &d_idx));
  hipLaunchKernelGGL(k_mark_found, dim3(ceil_div(cnt, 256)), dim3(256), 0, c->stream, found_dev, n, d_idx, cnt);
  PQ_HIP(hipGetLastError());
  PQ_HIP(hipStreamSynchronize(c->stream));  // the caller's index array may go away on return
  return 0;
}

}  // extern "C"
