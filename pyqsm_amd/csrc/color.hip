// color.hip — colours of a scan on the device (pyQSM's viz/color.py: segment_hues, color_distribution,
// saturate_colors, get_color_by_hue, remove_color_pts, get_green_surfaces).
//
// The arithmetic is color_exact.hpp: fp64, one operation at a time, matplotlib's rgb_to_hsv / hsv_to_rgb
// bit for bit; the class of a row is the first rule that holds on the hsv of its corrected colour.
//
//   k_hsv_segment   one pass over rgb f64 [n,3]: conversion, lift, back-conversion, second conversion,
//                   class; writes cls u8 [n] and, on request, the corrected rgb and its hsv. A wave owns 512
//                   consecutive rows (8 per lane, as boxes.hip) and counts its members per class by ballots.
//   scan            exclusive_scan_i32 over [class][wave] (classes 0 .. K-1, then "none")
//   k_hsv_members   reads the class bytes only and writes every index at its ballot rank: a CSR by class
//                   with ascending indices. No atomics: the same bytes on every run.
//   k_hsv_hist      a private u32 histogram per block in LDS (integer LDS atomics), flushed with 64-bit
//                   integer atomicAdd: integer sums, independent of the arrival order.
//   k_rgb_to_hsv, k_hsv_to_rgb, k_color_flags    the plain passes; the flags go through compact_flagged.
//
// A NaN or a value outside [0, 1] is refused: by the host forms before any launch, by the _dev form
// through an error word the kernel raises (32-bit atomicOr), PYQSM_EINVAL after the call.
#include "color_exact.hpp"
#include "common.hpp"

namespace pyqsm {

static constexpr int kColRounds = 8;                  // rows per lane
static constexpr int kColWaveRows = 64 * kColRounds;  // 512
static constexpr int kHistMaxBins = PYQSM_COLOR_MAX_BINS;
static constexpr int kHistBlocks = 2048;

static_assert(kColorMaxRules == PYQSM_COLOR_MAX_RULES, "color_exact.hpp and the header disagree");

__device__ __forceinline__ int class_code(int k, int K) { return k < K ? k : kColorNone; }

// counts[k * nw + wave] = rows of class k (k == K: none) among the wave's 512
__global__ __launch_bounds__(256) void k_hsv_segment(const double* __restrict__ rgb, int64_t n, ColorRules R,
                                                     double min_s, double lift_div, int64_t nw,
                                                     uint8_t* __restrict__ cls, int32_t* __restrict__ counts,
                                                     double* __restrict__ rgb_out, double* __restrict__ hsv_out,
                                                     int32_t* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int64_t base = wave * kColWaveRows;
  if (base >= n) return;  // the whole wave
  int32_t mine = 0;       // lane k counts class k
  bool bad = false;
  for (int r = 0; r < kColRounds; ++r) {
    const int64_t i = base + r * 64 + lane;
    const bool ok = i < n;
    int c = -1;  // no class: a row past the end
    if (ok) {
      const double cr = rgb[3 * i], cg = rgb[3 * i + 1], cb = rgb[3 * i + 2];
      bad |= !(color_in_range(cr) && color_in_range(cg) && color_in_range(cb));
      double o[3], h[3];
      c = color_segment_row(R, min_s, lift_div, cr, cg, cb, o, h);
      cls[i] = uint8_t(c);
      if (rgb_out) {
        rgb_out[3 * i] = o[0];
        rgb_out[3 * i + 1] = o[1];
        rgb_out[3 * i + 2] = o[2];
      }
      if (hsv_out) {
        hsv_out[3 * i] = h[0];
        hsv_out[3 * i + 1] = h[1];
        hsv_out[3 * i + 2] = h[2];
      }
    }
    for (int k = 0; k <= R.K; ++k) {
      const int m = __popcll(__ballot(c == class_code(k, R.K)));
      if (lane == k) mine += m;
    }
  }
  if (lane <= R.K) counts[size_t(lane) * nw + wave] = mine;
  if (bad) atomicOr(err, 1);
}

// counts: the scanned offsets of [class][wave]
__global__ __launch_bounds__(256) void k_hsv_members(const uint8_t* __restrict__ cls, int64_t n, int K, int64_t nw,
                                                     const int32_t* __restrict__ counts,
                                                     int64_t* __restrict__ members) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
  const int64_t base = wave * kColWaveRows;
  if (base >= n) return;
  int c[kColRounds];
#pragma unroll
  for (int r = 0; r < kColRounds; ++r) {
    const int64_t i = base + r * 64 + lane;
    c[r] = i < n ? int(cls[i]) : -1;
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int k = 0; k <= K; ++k) {
    const int code = class_code(k, K);
    int64_t off = int64_t(counts[size_t(k) * nw + wave]);
#pragma unroll
    for (int r = 0; r < kColRounds; ++r) {
      const bool in = c[r] == code;
      const unsigned long long m = __ballot(in);
      if (in) members[off + __popcll(m & below)] = base + r * 64 + lane;
      off += __popcll(m);
    }
  }
}

// counts_out[k] = rows of class k, from the scanned [class][wave] table (its last entry is the total)
__global__ __launch_bounds__(64) void k_hsv_counts(int K, int64_t nw, const int32_t* __restrict__ scanned,
                                                   int64_t* __restrict__ counts_out) {
  const int k = threadIdx.x;
  if (k <= K) counts_out[k] = int64_t(scanned[size_t(k + 1) * nw]) - int64_t(scanned[size_t(k) * nw]);
}

__global__ __launch_bounds__(256) void k_rgb_to_hsv(const double* __restrict__ rgb, int64_t n,
                                                    double* __restrict__ hsv, int32_t* __restrict__ err) {
  const int64_t i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const double r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
  if (!(color_in_range(r) && color_in_range(g) && color_in_range(b))) atomicOr(err, 1);
  double h, s, v;
  rgb_to_hsv_exact(r, g, b, h, s, v);
  hsv[3 * i] = h;
  hsv[3 * i + 1] = s;
  hsv[3 * i + 2] = v;
}

__global__ __launch_bounds__(256) void k_hsv_to_rgb(const double* __restrict__ hsv, int64_t n,
                                                    double* __restrict__ rgb, int32_t* __restrict__ err) {
  const int64_t i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= n) return;
  const double h = hsv[3 * i], s = hsv[3 * i + 1], v = hsv[3 * i + 2];
  if (!(color_in_range(h) && color_in_range(s) && color_in_range(v))) atomicOr(err, 1);
  double r, g, b;
  hsv_to_rgb_exact(h, s, v, r, g, b);
  rgb[3 * i] = r;
  rgb[3 * i + 1] = g;
  rgb[3 * i + 2] = b;
}

// flags [n + 1] for compact_flagged
__global__ __launch_bounds__(256) void k_color_flags(const double* __restrict__ rgb, int64_t n, int kind,
                                                     double param, int32_t* __restrict__ flags) {
  const int64_t i = blockIdx.x * 256ll + threadIdx.x;
  if (i > n) return;
  flags[i] = i < n && color_mask_row(kind, param, rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]) ? 1 : 0;
}

// vals: hsv rows, or rgb rows converted here (is_hsv == 0); cls / which: count only rows of that class
__global__ __launch_bounds__(256) void k_hsv_hist(const double* __restrict__ vals, int64_t n, int is_hsv, int bh,
                                                  int bs, int bv, const uint8_t* __restrict__ cls, int which,
                                                  unsigned long long* __restrict__ hist,
                                                  int32_t* __restrict__ err) {
  __shared__ uint32_t sh[kHistMaxBins];
  const int nb = bh * bs * bv;  // <= kHistMaxBins, checked by the caller
  for (int t = threadIdx.x; t < nb; t += 256) sh[t] = 0u;
  __syncthreads();
  bool bad = false;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
    if (cls && int(cls[i]) != which) continue;
    double h = vals[3 * i], s = vals[3 * i + 1], v = vals[3 * i + 2];
    bad |= !(color_in_range(h) && color_in_range(s) && color_in_range(v));
    if (!is_hsv) {
      const double r = h, g = s, b = v;
      rgb_to_hsv_exact(r, g, b, h, s, v);
    }
    const int bin = (color_bin(h, bh) * bs + color_bin(s, bs)) * bv + color_bin(v, bv);  // each factor in range
    atomicAdd(&sh[bin], 1u);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nb; t += 256)
    if (sh[t]) atomicAdd(&hist[t], static_cast<unsigned long long>(sh[t]));
  if (bad) atomicOr(err, 1);
}

// ---- host side

static int check_values(const char* who, const double* a, int64_t count) {
  for (int64_t i = 0; i < count; ++i)
    if (!color_in_range(a[i]))
      return fail(PYQSM_EINVAL, "%s: value %g at row %lld is outside [0, 1]", who, a[i], (long long)(i / 3));
  return 0;
}

static int err_word(Ctx* c, int32_t** d_err) {
  PQ_TRY(c->arena.get(1, d_err));
  PQ_HIP(hipMemsetAsync(*d_err, 0, 4, c->stream));
  return 0;
}

static int segment_check(const void* rgb, int64_t n, double min_s, double lift_div, const double* rules,
                         const int32_t* closed, int32_t K, const void* cls, int64_t* counts, ColorRules* R) {
  if (n < 0 || K < 0) return fail(PYQSM_EINVAL, "pyqsm_hsv_segment: negative size");
  if (K > kColorMaxRules) return fail(PYQSM_EINVAL, "pyqsm_hsv_segment: at most %d rules", kColorMaxRules);
  if (!counts || (n > 0 && (!rgb || !cls)) || (K > 0 && (!rules || !closed)))
    return fail(PYQSM_EINVAL, "pyqsm_hsv_segment: NULL pointer");
  for (int32_t k = 0; k <= K; ++k) counts[k] = 0;
  if (!(lift_div >= 1.0)) return fail(PYQSM_EINVAL, "pyqsm_hsv_segment: lift_div must be at least 1");
  if (min_s != min_s) return fail(PYQSM_EINVAL, "pyqsm_hsv_segment: min_s is NaN");
  std::memset(R, 0, sizeof(*R));
  R->K = K;
  for (int32_t k = 0; k < K; ++k) {
    R->closed[k] = closed[k];
    for (int a = 0; a < 6; ++a) {
      const double v = rules[6 * k + a];
      if (v != v) return fail(PYQSM_EINVAL, "pyqsm_hsv_segment: rule %d has a NaN bound", int(k));
      R->b[k][a] = v;
    }
  }
  // the member counts are scanned in 32 bits
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "pyqsm_hsv_segment: more than 2^31 - 256 rows");
  return 0;
}

// every pointer but counts on the device; members, rgb_out, hsv_out may be null
static int segment_run(Ctx* c, const double* d_rgb, int64_t n, const ColorRules& R, double min_s, double lift_div,
                       uint8_t* d_cls, int64_t* counts, int64_t* d_members, double* d_rgb_out, double* d_hsv_out) {
  const int K = R.K;
  const int64_t nw = (n + kColWaveRows - 1) / kColWaveRows;
  const unsigned blocks = unsigned((nw + 3) / 4);
  int32_t *d_counts, *d_err;
  int64_t* d_out;
  PQ_TRY(c->arena.get(size_t(K + 1) * nw + 1, &d_counts));
  PQ_TRY(c->arena.get(size_t(K) + 1, &d_out));
  PQ_TRY(err_word(c, &d_err));
  PQ_HIP(hipMemsetAsync(d_counts + size_t(K + 1) * nw, 0, 4, c->stream));
  {
    ProfScope ps(c, "hsv_segment");
    hipLaunchKernelGGL(k_hsv_segment, dim3(blocks), dim3(256), 0, c->stream, d_rgb, n, R, min_s, lift_div, nw, d_cls,
                       d_counts, d_rgb_out, d_hsv_out, d_err);
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(exclusive_scan_i32(c, d_counts, int64_t(K + 1) * nw + 1));  // the last entry becomes the total
  hipLaunchKernelGGL(k_hsv_counts, dim3(1), dim3(64), 0, c->stream, K, nw, static_cast<const int32_t*>(d_counts),
                     d_out);
  PQ_HIP(hipGetLastError());
  if (d_members) {
    ProfScope ps(c, "hsv_members");
    hipLaunchKernelGGL(k_hsv_members, dim3(blocks), dim3(256), 0, c->stream, static_cast<const uint8_t*>(d_cls), n, K,
                       nw, static_cast<const int32_t*>(d_counts), d_members);
    PQ_HIP(hipGetLastError());
  }
  int32_t bad = 0;
  PQ_TRY(download(c, counts, d_out, size_t(K) + 1));
  PQ_TRY(fetch(c, &bad, d_err));
  if (bad) return fail(PYQSM_EINVAL, "pyqsm_hsv_segment: a colour is NaN or outside [0, 1]");
  return 0;
}

// one of the two plain conversions, host arrays
template <typename Kern>
static int convert(const char* who, Kern kern, const double* in, int64_t n, double* out, int32_t device) {
  if (n < 0) return fail(PYQSM_EINVAL, "%s: negative size", who);
  if (n == 0) return 0;
  if (!in || !out) return fail(PYQSM_EINVAL, "%s: NULL pointer", who);
  PQ_TRY(check_values(who, in, n * 3));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_in, *d_out;
  int32_t* d_err;
  PQ_TRY(upload(c, in, size_t(n) * 3, &d_in));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_out));
  PQ_TRY(err_word(c, &d_err));
  {
    ProfScope ps(c, who);
    hipLaunchKernelGGL(kern, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, static_cast<const double*>(d_in), n,
                       d_out, d_err);
    PQ_HIP(hipGetLastError());
  }
  return fetch(c, out, d_out, size_t(n) * 3);
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_rgb_to_hsv(const double* rgb, int64_t n, double* hsv, int32_t device) {
  PQ_API_RANGE("pyqsm_rgb_to_hsv");
  return convert("pyqsm_rgb_to_hsv", k_rgb_to_hsv, rgb, n, hsv, device);
}

int pyqsm_hsv_to_rgb(const double* hsv, int64_t n, double* rgb, int32_t device) {
  PQ_API_RANGE("pyqsm_hsv_to_rgb");
  return convert("pyqsm_hsv_to_rgb", k_hsv_to_rgb, hsv, n, rgb, device);
}

int pyqsm_hsv_segment(const double* rgb, int64_t n, double min_s, double lift_div, const double* rules,
                      const int32_t* closed, int32_t K, uint8_t* cls, int64_t* counts, int64_t* members,
                      double* rgb_out, double* hsv_out, int32_t device) {
  PQ_API_RANGE("pyqsm_hsv_segment");
  ColorRules R;
  PQ_TRY(segment_check(rgb, n, min_s, lift_div, rules, closed, K, cls, counts, &R));
  if (n == 0) return 0;
  PQ_TRY(check_values("pyqsm_hsv_segment", rgb, n * 3));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_rgb, *d_rgb_out = nullptr, *d_hsv_out = nullptr;
  uint8_t* d_cls;
  int64_t* d_members = nullptr;
  PQ_TRY(upload(c, rgb, size_t(n) * 3, &d_rgb));
  PQ_TRY(c->arena.get(size_t(n), &d_cls));
  if (members) PQ_TRY(c->arena.get(size_t(n), &d_members));
  if (rgb_out) PQ_TRY(c->arena.get(size_t(n) * 3, &d_rgb_out));
  if (hsv_out) PQ_TRY(c->arena.get(size_t(n) * 3, &d_hsv_out));
  PQ_TRY(segment_run(c, d_rgb, n, R, min_s, lift_div, d_cls, counts, d_members, d_rgb_out, d_hsv_out));
  PQ_TRY(download(c, cls, d_cls, size_t(n)));
  if (members) PQ_TRY(download(c, members, d_members, size_t(n)));
  if (rgb_out) PQ_TRY(download(c, rgb_out, d_rgb_out, size_t(n) * 3));
  if (hsv_out) PQ_TRY(download(c, hsv_out, d_hsv_out, size_t(n) * 3));
  return stream_sync(c);
}

int pyqsm_hsv_segment_dev(const double* rgb_dev, int64_t n, double min_s, double lift_div, const double* rules,
                          const int32_t* closed, int32_t K, uint8_t* cls_dev, int64_t* counts, int64_t* members_dev,
                          double* rgb_out_dev, double* hsv_out_dev, int32_t device) {
  PQ_API_RANGE("pyqsm_hsv_segment_dev");
  ColorRules R;
  PQ_TRY(segment_check(rgb_dev, n, min_s, lift_div, rules, closed, K, cls_dev, counts, &R));
  if (n == 0) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  return segment_run(c, rgb_dev, n, R, min_s, lift_div, cls_dev, counts, members_dev, rgb_out_dev, hsv_out_dev);
}

int pyqsm_hsv_histogram(const double* vals, int64_t n, int32_t is_hsv, const int32_t* bins, const uint8_t* cls,
                        int32_t which, int64_t* hist, int32_t device) {
  PQ_API_RANGE("pyqsm_hsv_histogram");
  if (n < 0) return fail(PYQSM_EINVAL, "pyqsm_hsv_histogram: negative size");
  if (!bins || !hist || (n > 0 && !vals)) return fail(PYQSM_EINVAL, "pyqsm_hsv_histogram: NULL pointer");
  int64_t nb = 1;
  for (int a = 0; a < 3; ++a) {
    if (bins[a] < 1) return fail(PYQSM_EINVAL, "pyqsm_hsv_histogram: bins must be at least 1");
    if (bins[a] > kHistMaxBins) return fail(PYQSM_ERANGE, "pyqsm_hsv_histogram: more than %d bins", kHistMaxBins);
    nb *= bins[a];
  }
  if (nb > kHistMaxBins) return fail(PYQSM_ERANGE, "pyqsm_hsv_histogram: more than %d bins", kHistMaxBins);
  if (which < -1 || which > 255 || (which >= 0 && !cls && n > 0))
    return fail(PYQSM_EINVAL, "pyqsm_hsv_histogram: which needs cls and a class in [0, 255]");
  for (int64_t t = 0; t < nb; ++t) hist[t] = 0;
  if (n == 0) return 0;
  PQ_TRY(check_values("pyqsm_hsv_histogram", vals, n * 3));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_vals;
  uint8_t* d_cls = nullptr;
  unsigned long long* d_hist;
  int32_t* d_err;
  PQ_TRY(upload(c, vals, size_t(n) * 3, &d_vals));
  if (which >= 0) PQ_TRY(upload(c, cls, size_t(n), &d_cls));
  PQ_TRY(c->arena.get(size_t(nb), &d_hist));
  PQ_TRY(err_word(c, &d_err));
  PQ_HIP(hipMemsetAsync(d_hist, 0, size_t(nb) * 8, c->stream));
  {
    ProfScope ps(c, "hsv_hist");
    const unsigned blocks = unsigned(std::min<int64_t>(ceil_div(n, 256), kHistBlocks));
    hipLaunchKernelGGL(k_hsv_hist, dim3(blocks), dim3(256), 0, c->stream, static_cast<const double*>(d_vals), n,
                       int(is_hsv != 0), int(bins[0]), int(bins[1]), int(bins[2]),
                       static_cast<const uint8_t*>(d_cls), int(which), d_hist, d_err);
    PQ_HIP(hipGetLastError());
  }
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the histogram is downloaded as int64");
  return fetch(c, hist, reinterpret_cast<const int64_t*>(d_hist), size_t(nb));
}

int pyqsm_color_mask(const double* rgb, int64_t n, int32_t kind, double param, int64_t* idx, int64_t* count,
                     int32_t device) {
  PQ_API_RANGE("pyqsm_color_mask");
  if (count) *count = 0;
  if (n < 0) return fail(PYQSM_EINVAL, "pyqsm_color_mask: negative size");
  if (kind != PYQSM_MASK_SUM_GT && kind != PYQSM_MASK_GREEN)
    return fail(PYQSM_EINVAL, "pyqsm_color_mask: unknown kind %d", int(kind));
  if (!count || (n > 0 && (!rgb || !idx))) return fail(PYQSM_EINVAL, "pyqsm_color_mask: NULL pointer");
  if (n == 0) return 0;
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "pyqsm_color_mask: more than 2^31 - 256 rows");
  PQ_TRY(check_values("pyqsm_color_mask", rgb, n * 3));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_rgb;
  int32_t* d_flags;
  int64_t* d_idx;
  PQ_TRY(upload(c, rgb, size_t(n) * 3, &d_rgb));
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_flags));
  PQ_TRY(c->arena.get(size_t(n), &d_idx));
  {
    ProfScope ps(c, "color_flags");
    hipLaunchKernelGGL(k_color_flags, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream,
                       static_cast<const double*>(d_rgb), n, int(kind), param, d_flags);
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(compact_flagged(c, d_flags, n, d_idx));
  int32_t m = 0;
  PQ_TRY(fetch(c, &m, d_flags + n));
  if (m > 0) PQ_TRY(fetch(c, idx, d_idx, size_t(m)));
  *count = m;
  return 0;
}

}  // extern "C"
