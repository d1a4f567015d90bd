// ransac.hip — per-hypothesis parallel RANSAC for circles / cylinders on gfx950.
//
// Stands in for pyransac3d.Circle().fit / Cylinder().fit as called from
// pyQSM/math_utils/fit.py:277-283 (pyransac3d is not vendored by the
// reference; the algorithm restated here is its published circle.py /
// cylinder.py / aux_functions.rodrigues_rot). The random 3-point samples come
// from the caller so that runs are reproducible.
//
//   k_models   one lane per hypothesis: circle through the three samples
//              (plane normal, Rodrigues rotation to z, 2-D circumcentre, back)
//   k_count    lanes = hypotheses, points staged through LDS in SoA tiles and
//              read as broadcasts; one atomicAdd per (block, hypothesis)
//   k_best_seg a block per point set: the first hypothesis with the largest count
//   k_flags    inlier flags of the winning model -> scan -> ascending indices
//
// There is one kernel per stage and one driver, fit_sets: pyqsm_ransac_batch runs it over S point
// sets stacked in one array, pyqsm_ransac over one set. With several sets (MANY) a k_count block looks
// its tile up in a list and a k_flags lane bisects for its set; with one set a tile is blockIdx.y,
// the set is the n points, and none of that is built, uploaded or compiled in.
//
// The point-to-model distance follows NumPy's operation order exactly (each
// product and sum rounded separately, sums left to right, IEEE sqrt), so for a
// given model the inlier set is bit-identical to the NumPy statement in
// oracle/__init__.py. FP64 VALU bound: ~35 flop per (point, hypothesis).
//
// Plane segmentation (Open3D's segment_plane) rides on the same kernels: a plane is a
// Model with the unit normal in the axis and d in r, the third distance function of k_count / k_flags,
// compared strictly. k_plane_models builds the hypotheses (3 samples: the cross product; more: the
// least-squares plane of the samples), the winner's inliers are refitted from exact 128-bit
// fixed-point moments (fixed128.hpp), and pyqsm_segment_planes peels up to P planes off a cloud that
// stays in HBM. tests/plane_restatement.py states the contract in NumPy.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "fixed128.hpp"
#include "pca.hpp"

namespace pyqsm {

struct Model {
  double cx, cy, cz, ax, ay, az, r, valid;
};

struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 scale(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double norm(V3 a) { return sqrt(dot(a, a)); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// aux_functions.rodrigues_rot for one point.
__device__ V3 rodrigues(V3 p, V3 n0, V3 n1) {
  n0 = scale(n0, 1.0 / norm(n0));
  n1 = scale(n1, 1.0 / norm(n1));
  V3 k = cross(n0, n1);
  double kn = norm(k);
  if (kn == 0.0) return p;
  k = scale(k, 1.0 / kn);
  double theta = acos(dot(n0, n1));
  double c = cos(theta), s = sin(theta);
  V3 kxp = cross(k, p);
  double kd = dot(k, p) * (1.0 - c);
  return {p.x * c + kxp.x * s + k.x * kd, p.y * c + kxp.y * s + k.y * kd,
          p.z * c + kxp.z * s + k.z * kd};
}

// the model through three points of the set pts[0..n) (invalid when an index is out of range or the
// construction is not finite)
__device__ Model model_of(const double* __restrict__ pts, int64_t n, int64_t i0, int64_t i1, int64_t i2) {
  Model m = {0, 0, 0, 0, 0, 0, 0, 0};
  if (i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < n && i1 < n && i2 < n) {
    V3 p0 = {pts[3 * i0], pts[3 * i0 + 1], pts[3 * i0 + 2]};
    V3 p1 = {pts[3 * i1], pts[3 * i1 + 1], pts[3 * i1 + 2]};
    V3 p2 = {pts[3 * i2], pts[3 * i2 + 1], pts[3 * i2 + 2]};
    V3 vA = sub(p1, p0);
    vA = scale(vA, 1.0 / norm(vA));
    V3 vB = sub(p2, p0);
    vB = scale(vB, 1.0 / norm(vB));
    V3 vC = cross(vA, vB);
    vC = scale(vC, 1.0 / norm(vC));
    const V3 ez = {0.0, 0.0, 1.0};
    V3 q[3] = {rodrigues(p0, vC, ez), rodrigues(p1, vC, ez), rodrigues(p2, vC, ez)};
    double ma = 0.0, mb = 0.0;
    for (int it = 0; it < 3; ++it) {
      ma = (q[1].y - q[0].y) / (q[1].x - q[0].x);
      mb = (q[2].y - q[1].y) / (q[2].x - q[1].x);
      if (ma == 0.0) {  // np.roll(P_rot, -1, axis=0)
        V3 t = q[0];
        q[0] = q[1];
        q[1] = q[2];
        q[2] = t;
      } else {
        break;
      }
    }
    double pcx = (ma * mb * (q[0].y - q[2].y) + mb * (q[0].x + q[1].x) - ma * (q[1].x + q[2].x)) /
                 (2.0 * (mb - ma));
    double pcy = -1.0 / ma * (pcx - (q[0].x + q[1].x) / 2.0) + (q[0].y + q[1].y) / 2.0;
    V3 pc = {pcx, pcy, 0.0};
    double radius = norm(sub(pc, q[0]));
    V3 ctr = rodrigues(pc, ez, vC);
    bool ok = isfinite(ctr.x) && isfinite(ctr.y) && isfinite(ctr.z) && isfinite(radius) &&
              isfinite(vC.x) && isfinite(vC.y) && isfinite(vC.z);
    m = {ctr.x, ctr.y, ctr.z, vC.x, vC.y, vC.z, radius, ok ? 1.0 : 0.0};
  }
  return m;
}

// The point sets of one launch, on the device: S sets stacked in one array of n points. One set
// (S == 1) is the n points themselves and has no lists: every pointer is null and nothing reads it.
struct Sets {
  int64_t S;
  const int64_t* seg_start;  // [S + 1], from 0 to n
  const int32_t* tile_set;   // [tiles] the tiles of kTile points of all sets: the set of each ...
  const int64_t* tile_base;  // [tiles] ... and its first point
  int64_t tiles;             // k_count's grid.y
};

// hypothesis h of set s is thread s * H + h, its triple local to the set
__global__ __launch_bounds__(256) void k_models(const double* __restrict__ pts, int64_t n, Sets sets,
                                                const int64_t* __restrict__ triples, int64_t H,
                                                Model* __restrict__ models) {
  const int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (t >= sets.S * H) return;
  int64_t b = 0, cnt = n;
  if (sets.seg_start) {
    const int64_t s = t / H;
    b = sets.seg_start[s];
    cnt = sets.seg_start[s + 1] - b;
  }
  models[t] = model_of(pts + 3 * b, cnt, triples[3 * t], triples[3 * t + 1], triples[3 * t + 2]);
}

// |distance| of one point to one model, NumPy operation order (oracle.ransac_distance).
template <int SHAPE>
__device__ __forceinline__ double model_dist(const Model& m, double x, double y, double z) {
  if (SHAPE == 2) return fabs(((m.ax * x + m.ay * y) + m.az * z) + m.r);  // plane: normal in a, d in r
  // d = center - pts ; cr = cross(axis, d)
  const double dx = m.cx - x, dy = m.cy - y, dz = m.cz - z;
  const double c0 = m.ay * dz - m.az * dy;
  const double c1 = m.az * dx - m.ax * dz;
  const double c2 = m.ax * dy - m.ay * dx;
  const double nr = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  if (SHAPE == 1) return fabs(nr - m.r);
  const double plane = (m.ax * (x - m.cx) + m.ay * (y - m.cy)) + m.az * (z - m.cz);
  const double dinf = nr - m.r;
  return fabs(sqrt(dinf * dinf + plane * plane));
}

// circle and cylinder: within the threshold, inclusive (pyransac3d); plane: strictly inside (Open3D)
template <int SHAPE>
__device__ __forceinline__ bool is_inlier(double dist, double thresh) {
  return SHAPE == 2 ? dist < thresh : dist <= thresh;
}

static constexpr int kTile = 1024;  // points per LDS tile

// blockIdx.y = a tile of kTile points of one set; models and counts are [S, H]
template <int SHAPE, bool MANY>
__global__ __launch_bounds__(256) void k_count(const double* __restrict__ pts, int64_t n, Sets sets,
                                               const Model* __restrict__ models, int64_t H,
                                               double thresh, int32_t* __restrict__ counts) {
  __shared__ double lx[kTile], ly[kTile], lz[kTile];
  const int s = MANY ? sets.tile_set[blockIdx.y] : 0;
  const int64_t base = MANY ? sets.tile_base[blockIdx.y] : int64_t(blockIdx.y) * kTile;
  const int64_t end = MANY ? sets.seg_start[s + 1] : n;
  const int cnt = int(end - base < kTile ? end - base : kTile);
  for (int i = threadIdx.x; i < cnt; i += 256) {
    lx[i] = pts[3 * (base + i)];
    ly[i] = pts[3 * (base + i) + 1];
    lz[i] = pts[3 * (base + i) + 2];
  }
  __syncthreads();
  const int64_t h = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (h >= H) return;
  const Model m = models[int64_t(s) * H + h];
  if (m.valid == 0.0) return;
  int32_t c = 0;
  for (int i = 0; i < cnt; ++i) c += is_inlier<SHAPE>(model_dist<SHAPE>(m, lx[i], ly[i], lz[i]), thresh);
  if (c) atomicAdd(&counts[int64_t(s) * H + h], c);
}

// a block per set: the first hypothesis with the largest count (none when every count is 0)
__global__ __launch_bounds__(256) void k_best_seg(const int32_t* __restrict__ counts, int64_t H,
                                                  int64_t* __restrict__ best, int32_t* __restrict__ best_cnt) {
  __shared__ int32_t rc[256];
  __shared__ int64_t rh[256];
  const int64_t s = blockIdx.x;
  int32_t c = 0;
  int64_t hb = -1;
  for (int64_t h = threadIdx.x; h < H; h += 256) {
    const int32_t v = counts[s * H + h];
    if (v > c) {  // ascending h within a thread: the first of the largest
      c = v;
      hb = h;
    }
  }
  rc[threadIdx.x] = c;
  rh[threadIdx.x] = hb;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (int(threadIdx.x) < off) {
      const int32_t oc = rc[threadIdx.x + off];
      const int64_t oh = rh[threadIdx.x + off];
      if (oc > rc[threadIdx.x] || (oc == rc[threadIdx.x] && oc > 0 && oh < rh[threadIdx.x])) {
        rc[threadIdx.x] = oc;
        rh[threadIdx.x] = oh;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    best[s] = rh[0];
    best_cnt[s] = rc[0];
  }
}

// flags [n + 1]: point i is an inlier of its set's winner (none: 0), flags[n] = 0. The winner of
// set s is best[s], where k_best_seg left it (-1: none); a plane's is chosen on the host
// (plane_select) and comes as best0.
template <int SHAPE, bool MANY>
__global__ __launch_bounds__(256) void k_flags(const double* __restrict__ pts, int64_t n, Sets sets,
                                               const Model* __restrict__ models, int64_t H,
                                               const int64_t* __restrict__ best, int64_t best0, double thresh,
                                               int32_t* __restrict__ flags, int32_t* __restrict__ set_of) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    flags[n] = 0;
    return;
  }
  int64_t lo = 0;
  if (MANY) {
    int64_t hi = sets.S - 1;  // the set of point i: the last s with seg_start[s] <= i
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (sets.seg_start[mid] <= i) lo = mid; else hi = mid - 1;
    }
    set_of[i] = int32_t(lo);
  }
  const int64_t b = SHAPE == 2 ? best0 : best[lo];
  int32_t f = 0;
  if (SHAPE == 2 || b >= 0) {
    const Model m = models[lo * H + b];
    f = is_inlier<SHAPE>(model_dist<SHAPE>(m, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]), thresh);
  }
  flags[i] = f;
}

// What a fit returns per set, in one record so that one copy brings it to the host: the winning
// hypothesis (-1: none has an inlier), its model (zeros when there is none) and its inlier count.
struct Winner {
  Model m;
  int64_t best, count;
};

// inliers as indices local to their set, set by set
__global__ __launch_bounds__(256) void k_compact_seg(int64_t n, const int64_t* __restrict__ seg_start,
                                                     const int32_t* __restrict__ set_of,
                                                     const int32_t* __restrict__ pos, int64_t* __restrict__ out) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  if (pos[i + 1] != pos[i]) out[pos[i]] = i - seg_start[set_of[i]];
}

__global__ __launch_bounds__(256) void k_gather_best(int64_t S, const Model* __restrict__ models, int64_t H,
                                                     const int64_t* __restrict__ best,
                                                     const int32_t* __restrict__ best_cnt, Winner* __restrict__ out) {
  const int64_t s = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (s >= S) return;
  out[s] = Winner{best[s] >= 0 ? models[s * H + best[s]] : Model{0, 0, 0, 0, 0, 0, 0, 0}, best[s], best_cnt[s]};
}

static constexpr int64_t kMaxTiles = 65535;  // k_count's grid.y

static Sets one_set(int64_t n) { return Sets{1, nullptr, nullptr, nullptr, ceil_div(n, kTile)}; }

// Every path that counts refuses an input of more tiles before it stages anything.
static int check_tiles(const char* who, int64_t tiles) {
  if (tiles > kMaxTiles) return fail(PYQSM_ERANGE, "%s: more than 65535 tiles of 1024 points per call", who);
  return 0;
}

// f(SHAPE, MANY) with the run-time pair as compile-time constants: the one place that turns a shape
// into a template argument. Planes (shape 2) come one set at a time.
template <class F>
static void with_kind(int shape, bool many, F f) {
  using std::false_type;
  using std::integral_constant;
  using std::true_type;
  if (shape == 2) f(integral_constant<int, 2>{}, false_type{});
  else if (shape == 0) many ? f(integral_constant<int, 0>{}, true_type{}) : f(integral_constant<int, 0>{}, false_type{});
  else many ? f(integral_constant<int, 1>{}, true_type{}) : f(integral_constant<int, 1>{}, false_type{});
}

// counts [S, H] of the models [S, H], each over the points of its set
static int count_on_device(Ctx* c, const double* d_pts, int64_t n, const Sets& sets, const Model* d_models,
                           int64_t H, int shape, double thresh, int32_t* d_counts) {
  PQ_HIP(hipMemsetAsync(d_counts, 0, size_t(sets.S * H) * 4, c->stream));
  if (n == 0 || H == 0) return 0;
  ProfScope ps(c, shape == 2 ? "plane_count" : "ransac_count");
  const dim3 grid(ceil_div(H, 256), unsigned(sets.tiles));
  with_kind(shape, sets.S > 1, [&](auto sh, auto many) {
    hipLaunchKernelGGL((k_count<decltype(sh)::value, decltype(many)::value>), grid, dim3(256), 0, c->stream, d_pts, n,
                       sets, d_models, H, thresh, d_counts);
  });
  PQ_HIP(hipGetLastError());
  return 0;
}

// the inlier flags [n + 1] of every set's winner: d_best [S], or for a plane best0
static int flags_on_device(Ctx* c, const double* d_pts, int64_t n, const Sets& sets, const Model* d_models,
                           int64_t H, const int64_t* d_best, int64_t best0, int shape, double thresh,
                           int32_t* d_flags, int32_t* d_set_of) {
  with_kind(shape, sets.S > 1, [&](auto sh, auto many) {
    hipLaunchKernelGGL((k_flags<decltype(sh)::value, decltype(many)::value>), dim3(ceil_div(n + 1, 256)), dim3(256), 0,
                       c->stream, d_pts, n, sets, d_models, H, d_best, best0, thresh, d_flags, d_set_of);
  });
  PQ_HIP(hipGetLastError());
  return 0;
}

static int check_args(const double* pts, int64_t n, int64_t H, int32_t shape) {
  if (n < 0 || H < 0) return fail(PYQSM_EINVAL, "negative size");
  if (shape != 0 && shape != 1) return fail(PYQSM_EINVAL, "shape must be 0 (circle) or 1 (cylinder)");
  if (n > 0 && !pts) return fail(PYQSM_EINVAL, "pts is NULL");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  return 0;
}

static void put_model(const Model& m, double center[3], double axis[3], double* radius) {
  center[0] = m.cx; center[1] = m.cy; center[2] = m.cz;
  axis[0] = m.ax; axis[1] = m.ay; axis[2] = m.az;
  *radius = m.r;
}

// The fit of S point sets stacked in d_pts (seg_start on the host, [S + 1] from 0 to n; S == 1: the n
// points, seg_start unread), H hypotheses per set from d_tri [S, H, 3]: models, counts, the first
// hypothesis of the largest count per set, its inlier flags, and the inliers as ascending indices
// local to their set, set by set. win: [S] on the host. Two synchronisations: before the inlier total
// is known, and for the inliers. Needs n > 0, H > 0 and at most kMaxTiles tiles.
static int fit_sets(Ctx* c, const double* d_pts, int64_t n, const int64_t* seg_start, int64_t S,
                    const int64_t* d_tri, int64_t H, int shape, double thresh, Winner* win, int64_t* inliers) {
  const int64_t SH = S * H;
  Sets sets = one_set(n);
  int32_t* d_set_of = nullptr;
  if (S > 1) {  // the tiles of all sets
    std::vector<int32_t> h_tile_set;
    std::vector<int64_t> h_tile_base;
    for (int64_t s = 0; s < S; ++s)
      for (int64_t b = seg_start[s]; b < seg_start[s + 1]; b += kTile) {
        h_tile_set.push_back(int32_t(s));
        h_tile_base.push_back(b);
      }
    int64_t *d_seg, *d_tile_base;
    int32_t* d_tile_set;
    PQ_TRY(upload(c, seg_start, size_t(S) + 1, &d_seg));
    PQ_TRY(upload(c, h_tile_base.data(), h_tile_base.size(), &d_tile_base));
    PQ_TRY(upload(c, h_tile_set.data(), h_tile_set.size(), &d_tile_set));
    PQ_TRY(c->arena.get(size_t(n), &d_set_of));
    sets = Sets{S, d_seg, d_tile_set, d_tile_base, int64_t(h_tile_set.size())};
  }
  Model* d_models;
  Winner* d_win;
  int64_t *d_best, *d_out;
  int32_t *d_counts, *d_best_cnt, *d_flags;
  PQ_TRY(c->arena.get(size_t(SH), &d_models));
  PQ_TRY(c->arena.get(size_t(SH), &d_counts));
  PQ_TRY(c->arena.get(size_t(S), &d_best));
  PQ_TRY(c->arena.get(size_t(S), &d_best_cnt));
  PQ_TRY(c->arena.get(size_t(S), &d_win));
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_flags));
  PQ_TRY(c->arena.get(size_t(n), &d_out));
  {
    ProfScope ps(c, "ransac_models");
    hipLaunchKernelGGL(k_models, dim3(ceil_div(SH, 256)), dim3(256), 0, c->stream, d_pts, n, sets, d_tri, H,
                       d_models);
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(count_on_device(c, d_pts, n, sets, d_models, H, shape, thresh, d_counts));
  {
    ProfScope ps(c, "ransac_compact");
    hipLaunchKernelGGL(k_best_seg, dim3(unsigned(S)), dim3(256), 0, c->stream, d_counts, H, d_best, d_best_cnt);
    PQ_TRY(flags_on_device(c, d_pts, n, sets, d_models, H, d_best, -1, shape, thresh, d_flags, d_set_of));
    if (S > 1) {
      PQ_TRY(exclusive_scan_i32(c, d_flags, n + 1));
      hipLaunchKernelGGL(k_compact_seg, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, n, sets.seg_start, d_set_of,
                         d_flags, d_out);
    } else {
      PQ_TRY(compact_flagged(c, d_flags, n, d_out));
    }
    hipLaunchKernelGGL(k_gather_best, dim3(ceil_div(S, 256)), dim3(256), 0, c->stream, S, d_models, H, d_best,
                       d_best_cnt, d_win);
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(fetch(c, win, d_win, size_t(S)));
  int64_t total = 0;  // a winner's count is the number of its flags: the same predicate on the same points
  for (int64_t s = 0; s < S; ++s) total += win[s].count;
  if (total > 0) PQ_TRY(fetch(c, inliers, d_out, size_t(total)));
  return 0;
}

// the counts of H models over n points, staged from and fetched to the host
static int staged_count(int32_t device, const double* pts, int64_t n, const Model* models, int64_t H, int shape,
                        double thresh, int32_t* counts) {
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_pts;
  Model* d_models;
  int32_t* d_counts;
  PQ_TRY(c->arena.get(size_t(n) * 3 + 1, &d_pts));
  PQ_TRY(c->arena.get(size_t(H), &d_models));
  PQ_TRY(c->arena.get(size_t(H), &d_counts));
  if (n) PQ_TRY(copy_in(c, d_pts, pts, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_models, models, size_t(H)));
  PQ_TRY(count_on_device(c, d_pts, n, one_set(n), d_models, H, shape, thresh, d_counts));
  PQ_TRY(fetch(c, counts, d_counts, size_t(H)));
  return 0;
}

// ---- plane segmentation (pyqsm_plane_models / _count, pyqsm_segment_plane / _planes) -----------
// A plane is a Model with the unit normal in (ax, ay, az) and d in r: k_count<2> / k_flags<2> above
// count and flag with dist = |((a x + b y) + c z) + d| < thresh, strictly. DESIGN.md §20.

static constexpr int kPlaneMaxM = 32;    // samples per hypothesis
static constexpr int kFoldBlocks = 256;  // blocks of the bounding-box and moment folds

struct Cone {  // hypotheses with |n . axis| < cos_limit are invalid; cos_limit <= 0: no cone
  double ax, ay, az, cos_limit;
};

// the sign rule: c > 0, or c == 0 and b > 0, or c == b == 0 and a > 0
__device__ __forceinline__ void plane_orient(double p[4]) {
  const bool keep = p[2] > 0.0 || (p[2] == 0.0 && (p[1] > 0.0 || (p[1] == 0.0 && p[0] > 0.0)));
  if (!keep)
    for (int a = 0; a < 4; ++a) p[a] = -p[a];
}

// One lane per hypothesis. Sample j of hypothesis h is samples[h * m + j] (int64, an index into
// pts) or, with DRAW, the high 64 bits of draws[h * m + j] * n: an index into the dense array of the
// n points still alive. m == 3: the plane through the three points; m > 3: the least-squares plane
// of the m samples (sequential sums in sample order). Invalid hypotheses are rows of zeros.
template <bool DRAW>
__global__ __launch_bounds__(256) void k_plane_models(const double* __restrict__ pts, int64_t n,
                                                      const void* __restrict__ samples, int64_t H, int m,
                                                      Cone cone, Model* __restrict__ models,
                                                      double* __restrict__ planes) {
  const int64_t h = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (h >= H) return;
  const int64_t* si = static_cast<const int64_t*>(samples) + h * m;
  const unsigned long long* su = static_cast<const unsigned long long*>(samples) + h * m;
  auto index = [&](int j) -> int64_t {
    return DRAW ? int64_t(__umul64hi(su[j], (unsigned long long)n)) : si[j];
  };
  bool ok = true;
  for (int j = 0; j < m; ++j) {
    const int64_t i = index(j);
    if (i < 0 || i >= n) ok = false;
  }
  double p[4] = {0.0, 0.0, 0.0, 0.0};
  if (ok) {
    if (m == 3) {
      const int64_t i0 = index(0), i1 = index(1), i2 = index(2);
      const V3 p0 = {pts[3 * i0], pts[3 * i0 + 1], pts[3 * i0 + 2]};
      const V3 p1 = {pts[3 * i1], pts[3 * i1 + 1], pts[3 * i1 + 2]};
      const V3 p2 = {pts[3 * i2], pts[3 * i2 + 1], pts[3 * i2 + 2]};
      const V3 nrm = cross(sub(p1, p0), sub(p2, p0));
      const double L = norm(nrm);
      ok = L > 0.0;
      p[0] = nrm.x / L;
      p[1] = nrm.y / L;
      p[2] = nrm.z / L;
      p[3] = -((p[0] * p0.x + p[1] * p0.y) + p[2] * p0.z);
    } else {
      double sx = 0.0, sy = 0.0, sz = 0.0;
      for (int j = 0; j < m; ++j) {
        const int64_t i = index(j);
        sx = sx + pts[3 * i];
        sy = sy + pts[3 * i + 1];
        sz = sz + pts[3 * i + 2];
      }
      const double dm = double(m);
      const double cx = sx / dm, cy = sy / dm, cz = sz / dm;
      double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
      for (int j = 0; j < m; ++j) {
        const int64_t i = index(j);
        const double dx = pts[3 * i] - cx, dy = pts[3 * i + 1] - cy, dz = pts[3 * i + 2] - cz;
        c00 = c00 + dx * dx;
        c01 = c01 + dx * dy;
        c02 = c02 + dx * dz;
        c11 = c11 + dy * dy;
        c12 = c12 + dy * dz;
        c22 = c22 + dz * dz;
      }
      double nn[3];
      smallest_eigvec(Sym3{c00 / dm, c01 / dm, c02 / dm, c11 / dm, c12 / dm, c22 / dm}, nn);
      p[0] = nn[0];
      p[1] = nn[1];
      p[2] = nn[2];
      p[3] = -((nn[0] * cx + nn[1] * cy) + nn[2] * cz);
    }
    ok = ok && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(p[3]);
    if (ok) {
      plane_orient(p);
      if (cone.cos_limit > 0.0 && fabs((p[0] * cone.ax + p[1] * cone.ay) + p[2] * cone.az) < cone.cos_limit)
        ok = false;
    }
    if (!ok) p[0] = p[1] = p[2] = p[3] = 0.0;
  }
  models[h] = Model{0.0, 0.0, 0.0, p[0], p[1], p[2], p[3], ok ? 1.0 : 0.0};
  if (planes)
    for (int a = 0; a < 4; ++a) planes[4 * h + a] = p[a];
}

// The refit's frame: offsets are taken from the middle of the inliers' bounding box and scaled by
// its extents, so the refit plane is a function of the inlier SET alone.
struct PlaneFrame {
  double org[3];
  FeatScale sc;
};

// min / max of a block's six values (mn[3], mx[3]) into thread 0 (exact, so order-free)
__device__ __forceinline__ void block_box(double mn[3], double mx[3]) {
  __shared__ double sh[4][6];
  for (int off = 32; off > 0; off >>= 1)
    for (int a = 0; a < 3; ++a) {
      mn[a] = fmin(mn[a], __shfl_xor(mn[a], off, 64));
      mx[a] = fmax(mx[a], __shfl_xor(mx[a], off, 64));
    }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; ++a) {
      sh[w][a] = mn[a];
      sh[w][3 + a] = mx[a];
    }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int v = 1; v < 4; ++v)
      for (int a = 0; a < 3; ++a) {
        mn[a] = fmin(mn[a], sh[v][a]);
        mx[a] = fmax(mx[a], sh[v][3 + a]);
      }
}

// pos: the scanned inlier flags [n + 1]; point i is an inlier iff pos[i + 1] != pos[i].
// part [gridDim.x, 6]: every block's bounding box of its inliers (+inf / -inf when it has none).
__global__ __launch_bounds__(256) void k_inlier_box(const double* __restrict__ pts, int64_t n,
                                                    const int32_t* __restrict__ pos,
                                                    double* __restrict__ part) {
  const double inf = __builtin_inf();
  double mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
  for (int64_t i = blockIdx.x * int64_t(256) + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256)
    if (pos[i + 1] != pos[i])
      for (int a = 0; a < 3; ++a) {
        mn[a] = fmin(mn[a], pts[3 * i + a]);
        mx[a] = fmax(mx[a], pts[3 * i + a]);
      }
  block_box(mn, mx);
  if (threadIdx.x == 0)
    for (int a = 0; a < 3; ++a) {
      part[6 * size_t(blockIdx.x) + a] = mn[a];
      part[6 * size_t(blockIdx.x) + 3 + a] = mx[a];
    }
}

// one block: the fold of the nb <= 256 partial boxes, then the frame
__global__ __launch_bounds__(256) void k_plane_frame(const double* __restrict__ part, int nb,
                                                     PlaneFrame* __restrict__ frame) {
  const double inf = __builtin_inf();
  double mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
  if (int(threadIdx.x) < nb)
    for (int a = 0; a < 3; ++a) {
      mn[a] = part[6 * threadIdx.x + a];
      mx[a] = part[6 * threadIdx.x + 3 + a];
    }
  block_box(mn, mx);
  if (threadIdx.x == 0) {
    PlaneFrame f;
    double bound[3];
    for (int a = 0; a < 3; ++a) {
      const bool any = mn[a] <= mx[a];  // false when no point is flagged
      f.org[a] = any ? 0.5 * mn[a] + 0.5 * mx[a] : 0.0;
      bound[a] = any ? mx[a] - mn[a] : 0.0;
    }
    f.sc = feat_scale(bound);
    *frame = f;
  }
}

// part [gridDim.x, 9]: every block's exact moments of its inliers' offsets from the frame's origin
__global__ __launch_bounds__(256) void k_plane_moments(const double* __restrict__ pts, int64_t n,
                                                       const int32_t* __restrict__ pos,
                                                       const PlaneFrame* __restrict__ frame,
                                                       I128* __restrict__ part) {
  __shared__ I128 sh[4][9];
  const PlaneFrame f = *frame;
  I128 M[9];
  for (int t = 0; t < 9; ++t) M[t] = I128{0ull, 0LL};
  for (int64_t i = blockIdx.x * int64_t(256) + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256)
    if (pos[i + 1] != pos[i])
      add_moments(M, f.sc, pts[3 * i] - f.org[0], pts[3 * i + 1] - f.org[1], pts[3 * i + 2] - f.org[2]);
  for (int off = 32; off > 0; off >>= 1)
    for (int t = 0; t < 9; ++t) fold128(M[t], off);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int t = 0; t < 9; ++t) sh[w][t] = M[t];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int t = 0; t < 9; ++t) {
      for (int v = 1; v < 4; ++v) add128(M[t], sh[v][t]);
      part[9 * size_t(blockIdx.x) + t] = M[t];
    }
}

// one wave: the fold of the nb partial moments, then the least-squares plane through the inliers
// (centroid, covariance over N, smallest_eigvec, the sign rule). hyp <- the winning hypothesis; fit
// <- the refit, or the hypothesis with fewer than 3 inliers or a non-finite refit.
__global__ __launch_bounds__(64) void k_plane_refit(const I128* __restrict__ part, int nb,
                                                    const PlaneFrame* __restrict__ frame,
                                                    const int32_t* __restrict__ pos, int64_t n,
                                                    const Model* __restrict__ models, int64_t best,
                                                    double* __restrict__ fit, double* __restrict__ hyp) {
  I128 M[9];
  for (int t = 0; t < 9; ++t) M[t] = I128{0ull, 0LL};
  for (int b = threadIdx.x; b < nb; b += 64)
    for (int t = 0; t < 9; ++t) add128(M[t], part[9 * size_t(b) + t]);
  for (int off = 32; off > 0; off >>= 1)
    for (int t = 0; t < 9; ++t) fold128(M[t], off);
  if (threadIdx.x != 0) return;
  const Model mh = models[best];
  const double ph[4] = {mh.ax, mh.ay, mh.az, mh.r};
  double p[4] = {ph[0], ph[1], ph[2], ph[3]};
  const int32_t N = pos[n];
  if (N >= 3) {
    const PlaneFrame f = *frame;
    const double dn = double(N);
    double s1[3], cen[3], cv[6];
    for (int a = 0; a < 3; ++a) {
      s1[a] = to_double(M[a]) * f.sc.u1[a];
      cen[a] = f.org[a] + s1[a] / dn;
    }
    const int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};
    for (int e = 0; e < 6; ++e) {
      const double s2 = to_double(M[3 + e]) * f.sc.u2[e];
      cv[e] = (s2 - s1[A[e]] * (s1[B[e]] / dn)) / dn;
    }
    double nn[3];
    smallest_eigvec(Sym3{cv[0], cv[1], cv[2], cv[3], cv[4], cv[5]}, nn);
    double q[4] = {nn[0], nn[1], nn[2], -((nn[0] * cen[0] + nn[1] * cen[1]) + nn[2] * cen[2])};
    if (isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && isfinite(q[3])) {
      plane_orient(q);
      for (int a = 0; a < 4; ++a) p[a] = q[a];
    }
  }
  for (int a = 0; a < 4; ++a) {
    fit[a] = p[a];
    hyp[a] = ph[a];
  }
}

// flags[i] = point i carries no label yet (flags [n + 1], flags[n] = 0)
__global__ __launch_bounds__(256) void k_alive_flags(int64_t n, const int32_t* __restrict__ labels,
                                                     int32_t* __restrict__ flags) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i > n) return;
  flags[i] = i < n && labels[i] < 0;
}

// labels[alive[i]] = r for the inliers among the n alive points
__global__ __launch_bounds__(256) void k_plane_labels(int64_t n, const int32_t* __restrict__ pos,
                                                      const int64_t* __restrict__ alive, int32_t r,
                                                      int32_t* __restrict__ labels) {
  const int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  if (pos[i + 1] != pos[i]) labels[alive[i]] = r;
}

// What one segmentation works in, besides the points: taken once per call from the arena.
struct PlaneScratch {
  Model* models;
  double* planes;  // [H,4]
  int32_t* counts;
  int32_t* flags;  // [n + 1]
  double* boxes;   // [kFoldBlocks, 6]
  I128* moments;   // [kFoldBlocks, 9]
  PlaneFrame* frame;
};

static int plane_scratch(Ctx* c, int64_t n, int64_t H, PlaneScratch* s) {
  PQ_TRY(c->arena.get(size_t(H) + 1, &s->models));
  PQ_TRY(c->arena.get(size_t(H) * 4 + 4, &s->planes));
  PQ_TRY(c->arena.get(size_t(H) + 1, &s->counts));
  PQ_TRY(c->arena.get(size_t(n) + 1, &s->flags));
  PQ_TRY(c->arena.get(size_t(kFoldBlocks) * 6, &s->boxes));
  PQ_TRY(c->arena.get(size_t(kFoldBlocks) * 9, &s->moments));
  PQ_TRY(c->arena.get(1, &s->frame));
  return 0;
}

static int plane_models_device(Ctx* c, const double* d_pts, int64_t n, const void* d_samples, bool draw,
                               int64_t H, int m, const Cone& cone, Model* d_models, double* d_planes) {
  ProfScope ps(c, "plane_models");
  if (draw)
    hipLaunchKernelGGL(k_plane_models<true>, dim3(ceil_div(H, 256)), dim3(256), 0, c->stream, d_pts, n, d_samples, H,
                       m, cone, d_models, d_planes);
  else
    hipLaunchKernelGGL(k_plane_models<false>, dim3(ceil_div(H, 256)), dim3(256), 0, c->stream, d_pts, n, d_samples,
                       H, m, cone, d_models, d_planes);
  PQ_HIP(hipGetLastError());
  return 0;
}

// The selection rule over the H counts of n points: the first row with the largest count among
// the rows looked at, and the early stop of the adaptive iteration bound (the same log and pow as
// Python's math.log and ** in the restatement).
static void plane_select(const int32_t* cnt, int64_t H, int64_t n, int m, double probability, int64_t* best,
                         int64_t* best_cnt, int64_t* used) {
  int64_t b = -1, bc = 0, h = 0;
  double stop = double(H);
  for (; h < H; ++h) {
    if (double(h) > stop) break;
    if (cnt[h] > bc) {
      b = h;
      bc = cnt[h];
      const double f = double(bc) / double(n);
      if (f >= 1.0) {
        stop = 0.0;
      } else if (probability == 1.0) {
        stop = double(H);
      } else {
        const double den = std::log(1.0 - std::pow(f, double(m)));
        stop = den == 0.0 ? double(H) : std::fmin(std::log(1.0 - probability) / den, double(H));
      }
    }
  }
  *best = b;
  *best_cnt = bc;
  *used = h;
}

// counts of the H models over the n points, read back once, and the selection
static int plane_pick(Ctx* c, const double* d_pts, int64_t n, const PlaneScratch& s, int64_t H, int m, double thresh,
                      double probability, int64_t* best, int64_t* best_cnt, int64_t* used) {
  PQ_TRY(count_on_device(c, d_pts, n, one_set(n), s.models, H, 2, thresh, s.counts));
  std::vector<int32_t> h_counts(size_t(H), 0);
  PQ_TRY(fetch(c, h_counts.data(), s.counts, size_t(H)));
  plane_select(h_counts.data(), H, n, m, probability, best, best_cnt, used);
  return 0;
}

// the inlier flags of model `best`, scanned (s.flags becomes pos); idx (may be null) <- the inliers
static int plane_flag(Ctx* c, const double* d_pts, int64_t n, const PlaneScratch& s, int64_t best, double thresh,
                      int64_t* d_idx) {
  ProfScope ps(c, "plane_flag");
  PQ_TRY(flags_on_device(c, d_pts, n, one_set(n), s.models, 0 /* the row stride, unread with one set */, nullptr, best,
                         2, thresh, s.flags, nullptr));
  PQ_TRY(compact_flagged(c, s.flags, n, d_idx));
  return 0;
}

// the refit through the points flagged in s.flags (scanned) -> d_fit[4]; the hypothesis -> d_hyp[4]
static int plane_refit(Ctx* c, const double* d_pts, int64_t n, const PlaneScratch& s, int64_t best, double* d_fit,
                       double* d_hyp) {
  ProfScope ps(c, "plane_refit");
  const int nb = int(std::min<int64_t>(kFoldBlocks, ceil_div(n, 256)));
  hipLaunchKernelGGL(k_inlier_box, dim3(nb), dim3(256), 0, c->stream, d_pts, n, s.flags, s.boxes);
  hipLaunchKernelGGL(k_plane_frame, dim3(1), dim3(256), 0, c->stream, s.boxes, nb, s.frame);
  hipLaunchKernelGGL(k_plane_moments, dim3(nb), dim3(256), 0, c->stream, d_pts, n, s.flags, s.frame, s.moments);
  hipLaunchKernelGGL(k_plane_refit, dim3(1), dim3(64), 0, c->stream, s.moments, nb, s.frame, s.flags, n, s.models,
                     best, d_fit, d_hyp);
  PQ_HIP(hipGetLastError());
  return 0;
}

static constexpr int64_t kPlaneMaxN = kMaxTiles * kTile;

// the checks every plane call makes before it touches a device
static int plane_check(const char* who, const double* pts, int64_t n, int64_t H, int64_t m, bool need_m_points,
                       double thresh, double probability, const double* axis, double cos_limit) {
  if (n < 0 || H < 0) return fail(PYQSM_EINVAL, "%s: negative size", who);
  if (m < 3 || m > kPlaneMaxM) return fail(PYQSM_EINVAL, "%s: %d samples per hypothesis, need 3 ... 32", who, int(m));
  if (need_m_points && n < m) return fail(PYQSM_EINVAL, "%s: fewer points than samples per hypothesis", who);
  if (!std::isfinite(thresh) || thresh <= 0.0) return fail(PYQSM_EINVAL, "%s: the threshold must be finite and > 0", who);
  if (!(probability > 0.0 && probability <= 1.0)) return fail(PYQSM_EINVAL, "%s: probability must be in (0, 1]", who);
  if (n > 0 && !pts) return fail(PYQSM_EINVAL, "%s: pts is NULL", who);
  if (!std::isfinite(cos_limit)) return fail(PYQSM_EINVAL, "%s: cos_limit is not finite", who);
  if (cos_limit > 0.0) {
    if (!axis) return fail(PYQSM_EINVAL, "%s: a cone needs an axis", who);
    if (!std::isfinite(axis[0]) || !std::isfinite(axis[1]) || !std::isfinite(axis[2]))
      return fail(PYQSM_EINVAL, "%s: the axis is not finite", who);
  }
  if (n > kPlaneMaxN) return fail(PYQSM_ERANGE, "%s: more than 65535 * 1024 points per call", who);
  if (double(H) * double(m) > 2.0e9) return fail(PYQSM_ERANGE, "%s: more than 2e9 samples per call", who);
  for (int64_t i = 0; i < 3 * n; ++i)
    if (!std::isfinite(pts[i])) return fail(PYQSM_EINVAL, "%s: non-finite coordinate", who);
  return 0;
}

static Cone cone_of(const double* axis, double cos_limit) {
  if (!(cos_limit > 0.0) || !axis) return Cone{0.0, 0.0, 0.0, 0.0};
  return Cone{axis[0], axis[1], axis[2], cos_limit};
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_ransac_models(const double* pts, int64_t n, const int64_t* triples, int64_t H,
                        double* models, int32_t device) {
  PQ_API_RANGE("pyqsm_ransac_models");
  PQ_TRY(check_args(pts, n, H, 0));
  if (H == 0) return 0;
  if (!triples || !models) return fail(PYQSM_EINVAL, "pyqsm_ransac_models: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_pts;
  int64_t* d_tri;
  Model* d_models;
  PQ_TRY(c->arena.get(size_t(n) * 3 + 1, &d_pts));
  PQ_TRY(c->arena.get(size_t(H) * 3, &d_tri));
  PQ_TRY(c->arena.get(size_t(H), &d_models));
  if (n) PQ_TRY(copy_in(c, d_pts, pts, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_tri, triples, size_t(H) * 3));
  hipLaunchKernelGGL(k_models, dim3(ceil_div(H, 256)), dim3(256), 0, c->stream, d_pts, n, one_set(n), d_tri, H,
                     d_models);
  PQ_HIP(hipGetLastError());
  PQ_TRY(fetch(c, reinterpret_cast<Model*>(models), d_models, size_t(H)));
  return 0;
}

int pyqsm_ransac_count(const double* pts, int64_t n, const double* models, int64_t H,
                       int32_t shape, double thresh, int32_t* counts, int32_t device) {
  PQ_API_RANGE("pyqsm_ransac_count");
  PQ_TRY(check_args(pts, n, H, shape));
  PQ_TRY(check_tiles("pyqsm_ransac_count", ceil_div(n, kTile)));
  if (H == 0) return 0;
  if (!models || !counts) return fail(PYQSM_EINVAL, "pyqsm_ransac_count: NULL pointer");
  return staged_count(device, pts, n, reinterpret_cast<const Model*>(models), H, shape, thresh, counts);
}

int pyqsm_ransac(const double* pts, int64_t n, const int64_t* triples, int64_t H, int32_t shape,
                 double thresh, double center[3], double axis[3], double* radius,
                 int64_t* inliers, int64_t* n_inliers, int64_t* best_out, int32_t device) {
  PQ_API_RANGE("pyqsm_ransac");
  PQ_TRY(check_args(pts, n, H, shape));
  PQ_TRY(check_tiles("pyqsm_ransac", ceil_div(n, kTile)));
  if (n_inliers) *n_inliers = 0;
  if (best_out) *best_out = -1;
  if (n == 0 || H == 0) return 0;
  if (!triples || !center || !axis || !radius || !inliers || !n_inliers)
    return fail(PYQSM_EINVAL, "pyqsm_ransac: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_pts;
  int64_t* d_tri;
  PQ_TRY(upload(c, pts, size_t(n) * 3, &d_pts));
  PQ_TRY(upload(c, triples, size_t(H) * 3, &d_tri));
  Winner w;
  PQ_TRY(fit_sets(c, d_pts, n, nullptr, 1, d_tri, H, shape, thresh, &w, inliers));
  if (w.best < 0) return 0;
  put_model(w.m, center, axis, radius);
  *n_inliers = w.count;
  if (best_out) *best_out = w.best;
  return 0;
}

// Many independent fits in one call: S point sets stacked in pts (seg_start int64 [S+1], from 0 to n),
// H hypotheses per set (triples int64 [S,H,3], indices LOCAL to the set). Per set the result of
// pyqsm_ransac: the first hypothesis with the largest inlier count (best = -1 and zeros when no
// hypothesis has an inlier), its model, and its inliers as ascending local indices, written set
// by set into `inliers` (n_inliers [S] says how many each set has).
int pyqsm_ransac_batch(const double* pts, int64_t n, const int64_t* seg_start, int64_t n_seg,
                       const int64_t* triples, int64_t H, int32_t shape, double thresh, double* centers,
                       double* axes, double* radii, int64_t* inliers, int64_t* n_inliers, int64_t* best_out,
                       int32_t device) {
  PQ_API_RANGE("pyqsm_ransac_batch");
  PQ_TRY(check_args(pts, n, H, shape));
  if (n_seg < 0) return fail(PYQSM_EINVAL, "negative number of sets");
  if (n_seg == 0) return 0;
  if (!seg_start || !centers || !axes || !radii || !n_inliers || !best_out || (n > 0 && !inliers))
    return fail(PYQSM_EINVAL, "pyqsm_ransac_batch: NULL pointer");
  if (seg_start[0] != 0 || seg_start[n_seg] != n) return fail(PYQSM_EINVAL, "seg_start must run from 0 to n");
  for (int64_t s = 0; s < n_seg; ++s)
    if (seg_start[s + 1] < seg_start[s]) return fail(PYQSM_EINVAL, "seg_start must not decrease");
  for (int64_t s = 0; s < n_seg; ++s) {
    n_inliers[s] = 0;
    best_out[s] = -1;
    radii[s] = 0.0;
    for (int a = 0; a < 3; ++a) centers[3 * s + a] = axes[3 * s + a] = 0.0;
  }
  if (n == 0 || H == 0) return 0;
  if (!triples) return fail(PYQSM_EINVAL, "pyqsm_ransac_batch: triples is NULL");
  if (double(n_seg) * double(H) > 2.0e9) return fail(PYQSM_ERANGE, "more than 2^31 hypotheses per call");
  int64_t tiles = 0;
  for (int64_t s = 0; s < n_seg; ++s) tiles += ceil_div(seg_start[s + 1] - seg_start[s], kTile);
  PQ_TRY(check_tiles("pyqsm_ransac_batch", tiles));
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_pts;
  int64_t* d_tri;
  PQ_TRY(upload(c, pts, size_t(n) * 3, &d_pts));
  PQ_TRY(upload(c, triples, size_t(n_seg * H) * 3, &d_tri));
  std::vector<Winner> win(static_cast<size_t>(n_seg));
  PQ_TRY(fit_sets(c, d_pts, n, seg_start, n_seg, d_tri, H, shape, thresh, win.data(), inliers));
  for (int64_t s = 0; s < n_seg; ++s) {
    const Winner& w = win[size_t(s)];
    put_model(w.m, centers + 3 * s, axes + 3 * s, radii + s);
    n_inliers[s] = w.count;
    best_out[s] = w.best;
  }
  return 0;
}

// ---- plane segmentation ----------------------------------------------------------

int pyqsm_plane_models(const double* pts, int64_t n, const int64_t* samples, int64_t H, int32_t m,
                       const double* axis, double cos_limit, double* planes, int32_t device) {
  PQ_API_RANGE("pyqsm_plane_models");
  PQ_TRY(plane_check("pyqsm_plane_models", pts, n, H, m, false, 1.0, 1.0, axis, cos_limit));
  if (H == 0) return 0;
  if (!samples || !planes) return fail(PYQSM_EINVAL, "pyqsm_plane_models: NULL pointer");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_pts, *d_planes;
  int64_t* d_smp;
  Model* d_models;
  PQ_TRY(c->arena.get(size_t(n) * 3 + 1, &d_pts));
  PQ_TRY(c->arena.get(size_t(H) * m, &d_smp));
  PQ_TRY(c->arena.get(size_t(H), &d_models));
  PQ_TRY(c->arena.get(size_t(H) * 4, &d_planes));
  if (n) PQ_TRY(copy_in(c, d_pts, pts, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_smp, samples, size_t(H) * m));
  PQ_TRY(plane_models_device(c, d_pts, n, d_smp, false, H, m, cone_of(axis, cos_limit), d_models, d_planes));
  PQ_TRY(fetch(c, planes, d_planes, size_t(H) * 4));
  return 0;
}

int pyqsm_plane_count(const double* pts, int64_t n, const double* planes, int64_t H, double thresh,
                      int32_t* counts, int32_t device) {
  PQ_API_RANGE("pyqsm_plane_count");
  PQ_TRY(plane_check("pyqsm_plane_count", pts, n, H, 3, false, thresh, 1.0, nullptr, 0.0));
  if (H == 0) return 0;
  if (!planes || !counts) return fail(PYQSM_EINVAL, "pyqsm_plane_count: NULL pointer");
  std::vector<Model> h_models(static_cast<size_t>(H));
  for (int64_t h = 0; h < H; ++h) {  // a row of zeros is an invalid hypothesis
    const double* p = planes + 4 * h;
    const bool ok = p[0] != 0.0 || p[1] != 0.0 || p[2] != 0.0;
    h_models[size_t(h)] = Model{0.0, 0.0, 0.0, p[0], p[1], p[2], p[3], ok ? 1.0 : 0.0};
  }
  return staged_count(device, pts, n, h_models.data(), H, 2, thresh, counts);
}

int pyqsm_segment_plane(const double* pts, int64_t n, const int64_t* samples, int64_t H, int32_t m,
                        double thresh, double probability, const double* axis, double cos_limit,
                        double plane_fit[4], double plane_hyp[4], int64_t* inliers, int64_t* n_inliers,
                        int64_t* best_out, int64_t* used_out, int32_t device) {
  PQ_API_RANGE("pyqsm_segment_plane");
  PQ_TRY(plane_check("pyqsm_segment_plane", pts, n, H, m, true, thresh, probability, axis, cos_limit));
  if (!plane_fit || !plane_hyp || !inliers || !n_inliers || !best_out || !used_out)
    return fail(PYQSM_EINVAL, "pyqsm_segment_plane: NULL pointer");
  for (int a = 0; a < 4; ++a) plane_fit[a] = plane_hyp[a] = 0.0;
  *n_inliers = 0;
  *best_out = -1;
  *used_out = 0;
  if (H == 0) return 0;
  if (!samples) return fail(PYQSM_EINVAL, "pyqsm_segment_plane: samples is NULL");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_pts, *d_out;
  int64_t *d_smp, *d_idx;
  PlaneScratch s;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_pts));
  PQ_TRY(c->arena.get(size_t(H) * m, &d_smp));
  PQ_TRY(c->arena.get(size_t(n), &d_idx));
  PQ_TRY(c->arena.get(8, &d_out));
  PQ_TRY(plane_scratch(c, n, H, &s));
  PQ_TRY(copy_in(c, d_pts, pts, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_smp, samples, size_t(H) * m));
  PQ_TRY(plane_models_device(c, d_pts, n, d_smp, false, H, m, cone_of(axis, cos_limit), s.models, s.planes));
  int64_t best = -1, bc = 0, used = 0;
  PQ_TRY(plane_pick(c, d_pts, n, s, H, m, thresh, probability, &best, &bc, &used));
  *used_out = used;
  if (best < 0) return 0;
  PQ_TRY(plane_flag(c, d_pts, n, s, best, thresh, d_idx));
  PQ_TRY(plane_refit(c, d_pts, n, s, best, d_out, d_out + 4));
  double h_out[8];
  PQ_TRY(download(c, h_out, d_out, 8));
  PQ_TRY(download(c, inliers, d_idx, size_t(bc)));
  PQ_HIP(hipStreamSynchronize(c->stream));
  for (int a = 0; a < 4; ++a) {
    plane_fit[a] = h_out[a];
    plane_hyp[a] = h_out[4 + a];
  }
  *n_inliers = bc;
  *best_out = best;
  return 0;
}

int pyqsm_segment_planes(const double* pts, int64_t n, const uint64_t* draws, int64_t P, int64_t H, int32_t m,
                         double thresh, double probability, int64_t min_inliers, const double* axis,
                         double cos_limit, int32_t* labels, double* planes_fit, double* planes_hyp,
                         int64_t* counts, int64_t* best_out, int64_t* used_out, int64_t* n_planes,
                         int32_t device) {
  PQ_API_RANGE("pyqsm_segment_planes");
  if (P < 1) return fail(PYQSM_EINVAL, "pyqsm_segment_planes: need at least one plane");
  PQ_TRY(plane_check("pyqsm_segment_planes", pts, n, H, m, true, thresh, probability, axis, cos_limit));
  if (double(P) * double(H) * double(m) > 2.0e9)
    return fail(PYQSM_ERANGE, "pyqsm_segment_planes: more than 2e9 draws per call");
  if (!labels || !planes_fit || !planes_hyp || !counts || !best_out || !used_out || !n_planes)
    return fail(PYQSM_EINVAL, "pyqsm_segment_planes: NULL pointer");
  for (int64_t i = 0; i < n; ++i) labels[i] = -1;
  for (int64_t r = 0; r < P; ++r) {
    for (int a = 0; a < 4; ++a) planes_fit[4 * r + a] = planes_hyp[4 * r + a] = 0.0;
    counts[r] = 0;
    best_out[r] = -1;
    used_out[r] = 0;
  }
  *n_planes = 0;
  if (H == 0) return 0;
  if (!draws) return fail(PYQSM_EINVAL, "pyqsm_segment_planes: draws is NULL");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  // the loop's scratch, taken once
  double *d_pts, *d_alive_pts, *d_out;
  uint64_t* d_draws;
  int64_t* d_alive;
  int32_t *d_labels, *d_aflags;
  PlaneScratch s;
  const size_t per_round = size_t(H) * m;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_pts));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_alive_pts));
  PQ_TRY(c->arena.get(size_t(P) * per_round, &d_draws));
  PQ_TRY(c->arena.get(size_t(n), &d_alive));
  PQ_TRY(c->arena.get(size_t(n), &d_labels));
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_aflags));
  PQ_TRY(c->arena.get(size_t(P) * 8, &d_out));
  PQ_TRY(plane_scratch(c, n, H, &s));
  PQ_TRY(copy_in(c, d_pts, pts, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_draws, draws, size_t(P) * per_round));
  PQ_HIP(hipMemsetAsync(d_labels, 0xFF, size_t(n) * 4, c->stream));  // -1: alive
  const Cone cone = cone_of(axis, cos_limit);
  int64_t n_alive = n, np = 0;
  for (int64_t r = 0; r < P && n_alive >= m; ++r) {
    const Arena::Mark mk = c->arena.mark();  // the scans' block sums
    {
      ProfScope ps(c, "plane_compact");
      hipLaunchKernelGGL(k_alive_flags, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, n, d_labels, d_aflags);
      PQ_HIP(hipGetLastError());
      PQ_TRY(compact_flagged(c, d_aflags, n, d_alive, nullptr, d_pts, d_alive_pts));
    }
    PQ_TRY(plane_models_device(c, d_alive_pts, n_alive, d_draws + size_t(r) * per_round, true, H, m, cone, s.models,
                               s.planes));
    int64_t best = -1, bc = 0, used = 0;
    PQ_TRY(plane_pick(c, d_alive_pts, n_alive, s, H, m, thresh, probability, &best, &bc, &used));
    if (best < 0 || bc < min_inliers) break;  // this round labels nothing
    PQ_TRY(plane_flag(c, d_alive_pts, n_alive, s, best, thresh, nullptr));
    hipLaunchKernelGGL(k_plane_labels, dim3(ceil_div(n_alive, 256)), dim3(256), 0, c->stream, n_alive, s.flags,
                       d_alive, int32_t(r), d_labels);
    PQ_HIP(hipGetLastError());
    PQ_TRY(plane_refit(c, d_alive_pts, n_alive, s, best, d_out + 8 * r, d_out + 8 * r + 4));
    counts[r] = bc;
    best_out[r] = best;
    used_out[r] = used;
    n_alive -= bc;
    ++np;
    c->arena.rewind(mk);
  }
  std::vector<double> h_out(size_t(P) * 8, 0.0);
  PQ_TRY(download(c, labels, d_labels, size_t(n)));
  if (np) PQ_TRY(download(c, h_out.data(), d_out, size_t(np) * 8));
  PQ_HIP(hipStreamSynchronize(c->stream));
  for (int64_t r = 0; r < np; ++r)
    for (int a = 0; a < 4; ++a) {
      planes_fit[4 * r + a] = h_out[size_t(8 * r + a)];
      planes_hyp[4 * r + a] = h_out[size_t(8 * r + 4 + a)];
    }
  *n_planes = np;
  return 0;
}

}  // extern "C"
