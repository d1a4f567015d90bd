// normals.hip — the stem stage of pyQSM's QSM route (pyQSM/qsm_generation.py:71-120 get_stem_pcd):
// Open3D's PointCloud.estimate_normals and orient_normals_consistent_tangent_plane, the angle filter
// of filter_by_norm, and the whole stage resident in HBM. Recollected from Open3D, parity unpinned;
// tests/normals_restatement.py states the contract in NumPy/SciPy and the kernels are held to it bit
// for bit.
//
// Normals. Hybrid search (radius > 0 and finite): the source cloud is binned into cells of the
// radius (grid.hpp: ball_grid); one wave per query (in the grid's sorted order) selects and sorts its
// candidates with d2 < r2 in the 27 cells around it with the pieces of wave_select.hpp: all of them,
// or, when more than kNormCap lie inside, those up to the max_nn-th smallest d2 and every tie at it
// (more than kNormCap of those: the overflow flag); it keeps the first max_nn. KNN search: the
// exact kNN (knn.hip, the point itself counted) already comes ascending by (d2, index). Either way
// the wave gathers the offsets p_j - p_i into LDS, three lanes sum the mean and six lanes the
// covariance entries, one add at a time in neighbour order; k_normal_finish then runs the Jacobi
// solve (pca.hpp) and the sign rule on one lane per point.
//
// Orientation. Boruvka over the directed kNN edges (boruvka.hpp has the rounds and why their outcome
// does not depend on the order of the atomics) with labels that carry a parity bit (label = root << 1
// | parity of the point relative to its root): the weight of an edge is 1 - |n_i . n_j|, its flip bit
// the sign of the dot. A point's parity ends up the XOR of the flip bits along its tree path; the
// component's highest point (lowest index on ties) fixes the sign.
#include <algorithm>
#include <cmath>

#include "boruvka.hpp"
#include "common.hpp"
#include "grid.hpp"
#include "knn.hpp"
#include "pca.hpp"
#include "wave_select.hpp"

namespace pyqsm {

// (kKnnMaxK, knn.hpp: largest max_nn of a KNN search and largest k of the orientation)
static constexpr int kNormMaxNN = 256;        // largest max_nn of a hybrid search
static constexpr int kNormCap = 512;          // (d2, index) pairs a wave sorts in LDS

// ---- neighbourhoods and covariance --------------------------------------------------------------
// Covariance of the first cnt neighbours listed in nb (LDS, ascending (d2, index)) of point i:
// o_j = p_j - p_i, m = (sum o) / cnt, C = (sum (o - m)(o - m)^T) / cnt, every sum from 0.0 one add
// at a time in list order. o: LDS [3][kNormMaxNN], scratch: LDS, at least 3 doubles. Lane c < 6
// writes entry c of (c00, c01, c02, c11, c12, c22) to cov[6 i + c]; lane 0 the count.
__device__ void covariance_of_list(int lane, int i, int cnt, const int* nb, const double* __restrict__ xyz,
                                   double (*o)[kNormMaxNN], double* scratch, double* __restrict__ cov,
                                   int32_t* __restrict__ cnt_out) {
  const double px = xyz[3 * size_t(i)], py = xyz[3 * size_t(i) + 1], pz = xyz[3 * size_t(i) + 2];
  for (int t = lane; t < cnt; t += 64) {
    const size_t j = size_t(nb[t]) * 3;
    o[0][t] = xyz[j] - px;
    o[1][t] = xyz[j + 1] - py;
    o[2][t] = xyz[j + 2] - pz;
  }
  wave_sync();
  const double dn = double(cnt);
  if (lane < 3) {
    double s = 0.0;
    for (int t = 0; t < cnt; ++t) s = s + o[lane][t];
    scratch[lane] = s / dn;
  }
  wave_sync();
  if (lane < 6) {
    const int a = lane < 3 ? 0 : (lane < 5 ? 1 : 2);
    const int b = lane < 3 ? lane : (lane < 5 ? lane - 2 : 2);
    const double ma = scratch[a], mb = scratch[b];
    double s = 0.0;
    for (int t = 0; t < cnt; ++t) s = s + (o[a][t] - ma) * (o[b][t] - mb);
    cov[6 * size_t(i) + lane] = s / dn;
  }
  if (lane == 0) cnt_out[i] = cnt;
}

// Hybrid search, one wave per query: wave p serves the point at sorted position p (neighbouring
// waves then read neighbouring cells). *overflow = 1 when more than kNormCap points tie at the
// max_nn-th distance of some query (the result of that query is then not the contract's).
template <class CO>
__global__ __launch_bounds__(128) void k_normal_hybrid(int n, const double* __restrict__ xyz, GridParams g,
                                                       const int32_t* __restrict__ start,
                                                       const int32_t* __restrict__ order, CO co, double r2, int k,
                                                       double* __restrict__ cov, int32_t* __restrict__ cnt_out,
                                                       int32_t* __restrict__ overflow) {
  __shared__ double sd[2][kNormCap];
  __shared__ int si[2][kNormCap];
  __shared__ double so[2][3][kNormMaxNN];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = blockIdx.x * 2 + w;
  if (p >= n) return;  // whole wave
  const int i = order[p];
  const double x = xyz[3 * size_t(i)], y = xyz[3 * size_t(i) + 1], z = xyz[3 * size_t(i) + 2];
  StencilRuns rr;  // clamped like the points were binned: the grid may cover less than the cloud
  point_stencil_runs(g, start, x, y, z, &rr);
  auto count_le = [&](double tau) {  // candidates with d2 < r2 and d2 <= tau
    return wave_count(rr, [=](int q) {
      const double d = co.d2(q, x, y, z);
      return d < r2 && d <= tau;
    });
  };
  const int total = count_le(__builtin_inf());
  // too many for the LDS: only those up to the k-th smallest d2 (k < total), every tie at it included
  const double tau = total > kNormCap ? kth_by_bits(r2, k, count_le) : __builtin_inf();
  int have = 0;
  wave_candidates(rr, [=, &have](int q, bool live) {
    double d = 0.0;
    bool take = false;
    if (live) {
      d = co.d2(q, x, y, z);
      take = d < r2 && d <= tau;
    }
    const int slot = wave_append(take, have);
    if (take && slot < kNormCap) {
      sd[w][slot] = d;
      si[w][slot] = order[q];
    }
  });
  if (have > kNormCap) {
    if (lane == 0) *overflow = 1;
    have = kNormCap;
  }
  wave_sort_pairs(sd[w], si[w], have);
  covariance_of_list(lane, i, min(have, k), si[w], xyz, so[w], sd[w], cov, cnt_out);
}

// KNN search: the k nearest (knn_device, ascending by (d2, index)), one wave per point.
__global__ __launch_bounds__(128) void k_normal_knn(int n, const double* __restrict__ xyz,
                                                    const int32_t* __restrict__ idx, int k,
                                                    double* __restrict__ cov, int32_t* __restrict__ cnt_out) {
  __shared__ int si[2][kKnnMaxK];
  __shared__ double so[2][3][kNormMaxNN];
  __shared__ double sm[2][4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 2 + w;
  if (i >= n) return;
  for (int t = lane; t < k; t += 64) si[w][t] = idx[size_t(i) * k + t];
  wave_sync();
  covariance_of_list(lane, i, k, si[w], xyz, so[w], sm[w], cov, cnt_out);
}

// One lane per point: fewer than 3 neighbours or an all-zero covariance keep the previous normal,
// or give (0, 0, 1) without one; otherwise the smallest eigenvector, flipped when it points away
// from the previous normal (dot < 0) or, without one, when n_z < 0.
__global__ __launch_bounds__(256) void k_normal_finish(int n, const double* __restrict__ cov,
                                                       const int32_t* __restrict__ cnt,
                                                       const double* __restrict__ prev, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* c = cov + 6 * size_t(i);
  const Sym3 A = {c[0], c[1], c[2], c[3], c[4], c[5]};
  double* o = out + 3 * size_t(i);
  const bool zero = A.a00 == 0.0 && A.a01 == 0.0 && A.a02 == 0.0 && A.a11 == 0.0 && A.a12 == 0.0 && A.a22 == 0.0;
  if (cnt[i] < 3 || zero) {
    o[0] = prev ? prev[3 * size_t(i)] : 0.0;
    o[1] = prev ? prev[3 * size_t(i) + 1] : 0.0;
    o[2] = prev ? prev[3 * size_t(i) + 2] : 1.0;
    return;
  }
  double v[3];
  smallest_eigvec(A, v);
  bool flip;
  if (prev) {
    const double* q = prev + 3 * size_t(i);
    flip = (v[0] * q[0] + v[1] * q[1]) + v[2] * q[2] < 0.0;
  } else {
    flip = v[2] < 0.0;
  }
  o[0] = flip ? -v[0] : v[0];
  o[1] = flip ? -v[1] : v[1];
  o[2] = flip ? -v[2] : v[2];
}

// ---- orientation: the edge policy of boruvka.hpp, then the sign --------------------------------
__device__ __forceinline__ double dot3(const double* __restrict__ nrm, int a, int b) {
  const double* p = nrm + 3 * size_t(a);
  const double* q = nrm + 3 * size_t(b);
  return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2];
}

// Every entry of the kNN table but the point itself is an edge, of weight 1 - |n_i . n_j|; it flips
// when the dot is negative. A hook records nothing beyond the parity.
struct OrientEdges {
  const int32_t* idx;
  const double* nrm;
  int k;
  __device__ void init(int) const {}
  __device__ bool ends(int64_t e, int* i, int* j) const {
    *i = int(e / k);
    *j = idx[e];
    return *j != *i;
  }
  __device__ unsigned long long key(int64_t, int i, int j) const { return ord_bits(1.0 - fabs(dot3(nrm, i, j))); }
  __device__ uint32_t flip(int a, int b) const { return dot3(nrm, a, b) < 0.0 ? 1u : 0u; }
  __device__ void hooked(uint32_t, unsigned long long, unsigned long long) const {}
};

// The highest point of every component, lowest index on ties: orderable z first, then the index.
__global__ __launch_bounds__(256) void k_top_z(int n, const double* __restrict__ xyz, const uint32_t* __restrict__ lab,
                                               unsigned long long* __restrict__ tz) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = lab[i] >> 1;
  const unsigned long long z = ord_bits(xyz[3 * size_t(i) + 2]);
  if (z > tz[r]) atomicMax(&tz[r], z);  // the maxima only rise: see k_bv_min_w
}

__global__ __launch_bounds__(256) void k_top_i(int n, const double* __restrict__ xyz, const uint32_t* __restrict__ lab,
                                               const unsigned long long* __restrict__ tz, uint32_t* __restrict__ ti) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = lab[i] >> 1;
  if (ord_bits(xyz[3 * size_t(i) + 2]) == tz[r]) atomicMin(&ti[r], uint32_t(i));
}

// Sign of i = parity of i relative to the highest point, XOR (that point's n_z < 0).
__global__ __launch_bounds__(256) void k_orient_final(int n, const double* __restrict__ nrm,
                                                      const uint32_t* __restrict__ lab,
                                                      const uint32_t* __restrict__ ti, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t l = lab[i];
  const uint32_t top = ti[l >> 1];
  const uint32_t s = ((l ^ lab[top]) & 1u) ^ (nrm[3 * size_t(top) + 2] < 0.0 ? 1u : 0u);
  const double* v = nrm + 3 * size_t(i);
  double* o = out + 3 * size_t(i);
  o[0] = s ? -v[0] : v[0];
  o[1] = s ? -v[1] : v[1];
  o[2] = s ? -v[2] : v[2];
}

// ---- stem stage: crop and angle filter -----------------------------------------------------------
// keep[i] = z > bound (pyQSM's crop removes z <= min z + offset); entry n = 0 for the scan
__global__ __launch_bounds__(256) void k_crop_mask(int n, const double* __restrict__ xyz, double bound,
                                                   int32_t* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  keep[i] = i < n && xyz[3 * size_t(i) + 2] > bound ? 1 : 0;
}

// filter_by_norm: angle = degrees(atan(n_z / sqrt(n_x^2 + n_y^2))), 0 when n_x = n_y = 0; keep
// -t < angle < t (rev: angle < -t or angle > t)
__global__ __launch_bounds__(256) void k_angle_mask(int n, const double* __restrict__ nrm, double t, int rev,
                                                    int32_t* __restrict__ keep) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    keep[n] = 0;
    return;
  }
  const double* v = nrm + 3 * size_t(i);
  const double den = sqrt(v[0] * v[0] + v[1] * v[1]);
  const double ang = den != 0.0 ? atan(v[2] / den) * (180.0 / M_PI) : 0.0;
  const bool in = ang > -t && ang < t;
  keep[i] = (rev ? (ang < -t || ang > t) : in) ? 1 : 0;
}

// ---- device-resident steps ---------------------------------------------------------------------
static bool hybrid_search(double radius) { return radius > 0 && std::isfinite(radius); }

static int check_max_nn(double radius, int32_t max_nn) {
  const int top = hybrid_search(radius) ? kNormMaxNN : kKnnMaxK;
  if (max_nn < 1 || max_nn > top)
    return fail(PYQSM_ERANGE, "max_nn must be in [1, %d] for a %s search", top, hybrid_search(radius) ? "hybrid" : "KNN");
  return 0;
}

// Normals of the n points at d_xyz into d_out (both device); d_prev (device, may be null) the
// previous normals.
static int normals_device(Ctx* c, const double* d_xyz, int64_t n, double radius, int32_t max_nn,
                          const double* d_prev, double* d_out) {
  if (n == 0) return 0;
  const int N = int(n);
  double* cov;
  int32_t* cnt;
  PQ_TRY(c->arena.get(size_t(n) * 6, &cov));
  PQ_TRY(c->arena.get(size_t(n), &cnt));
  int32_t* overflow = nullptr;
  if (hybrid_search(radius)) {
    PQ_TRY(c->arena.get(1, &overflow));
    PQ_HIP(hipMemsetAsync(overflow, 0, 4, c->stream));
    DevGrid g;
    {
      ProfScope ps(c, "normals_grid");
      PQ_TRY(ball_grid(c, d_xyz, n, radius, &g));
    }
    ProfScope ps(c, "normals_cov");
    on_coords(g, [&](auto co) {
      hipLaunchKernelGGL(k_normal_hybrid<decltype(co)>, dim3(ceil_div(n, 2)), dim3(128), 0, c->stream, N, d_xyz,
                         grid_params(g), g.start, g.order, co, radius * radius, int(max_nn), cov, cnt, overflow);
    });
    PQ_HIP(hipGetLastError());
  } else {
    const int k = int(std::min<int64_t>(max_nn, n));
    int32_t* idx;
    double* d2;
    PQ_TRY(c->arena.get(size_t(n) * k, &idx));
    PQ_TRY(c->arena.get(size_t(n) * k, &d2));
    {
      ProfScope ps(c, "normals_knn");
      PQ_TRY(knn_device(c, d_xyz, n, k, 0, idx, d2));
    }
    ProfScope ps(c, "normals_cov");
    hipLaunchKernelGGL(k_normal_knn, dim3(ceil_div(n, 2)), dim3(128), 0, c->stream, N, d_xyz,
                       static_cast<const int32_t*>(idx), k, cov, cnt);
    PQ_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "normals_eig");
    hipLaunchKernelGGL(k_normal_finish, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, N,
                       static_cast<const double*>(cov), static_cast<const int32_t*>(cnt), d_prev, d_out);
    PQ_HIP(hipGetLastError());
  }
  if (overflow) {
    int32_t of = 0;
    PQ_TRY(fetch(c, &of, overflow));
    if (of) return fail(PYQSM_ERANGE, "more than %d points tie at the max_nn-th distance of a query", kNormCap);
  }
  return 0;
}

// Orients the normals d_nrm of the n points d_xyz into d_out (all device). *rounds: Boruvka rounds
// that hooked at least one component.
static int orient_device(Ctx* c, const double* d_xyz, int64_t n, int32_t k, const double* d_nrm, double* d_out,
                         int32_t* rounds) {
  *rounds = 0;
  if (n == 0) return 0;
  const int N = int(n);
  const int kk = int(std::min<int64_t>(k, n));
  const int64_t ne = int64_t(n) * kk;
  int32_t *idx, *ctl;
  double* d2;
  uint32_t *lab, *hk, *ti;
  unsigned long long *bw, *be, *tz;
  PQ_TRY(c->arena.get(size_t(ne), &idx));
  PQ_TRY(c->arena.get(size_t(ne), &d2));
  PQ_TRY(c->arena.get(size_t(n), &lab));
  PQ_TRY(c->arena.get(size_t(n), &hk));
  PQ_TRY(c->arena.get(size_t(n), &ti));
  PQ_TRY(c->arena.get(size_t(n), &bw));
  PQ_TRY(c->arena.get(size_t(n), &be));
  PQ_TRY(c->arena.get(size_t(n), &tz));
  PQ_TRY(c->arena.get(size_t(kBvCtlWords), &ctl));
  {
    ProfScope ps(c, "orient_knn");
    PQ_TRY(knn_device(c, d_xyz, n, kk, 0, idx, d2));
  }
  PQ_TRY(boruvka_forest(c, "orientation", n, ne, OrientEdges{idx, d_nrm, kk},
                        BvScopes{"orient_min_edge", "orient_hook", "orient_jump"}, lab, hk, bw, be, ctl, rounds));
  const int pb = ceil_div(n, 256);
  ProfScope ps(c, "orient_sign");
  PQ_HIP(hipMemsetAsync(tz, 0, size_t(n) * 8, c->stream));
  PQ_HIP(hipMemsetAsync(ti, 0xFF, size_t(n) * 4, c->stream));
  hipLaunchKernelGGL(k_top_z, dim3(pb), dim3(256), 0, c->stream, N, d_xyz, static_cast<const uint32_t*>(lab), tz);
  hipLaunchKernelGGL(k_top_i, dim3(pb), dim3(256), 0, c->stream, N, d_xyz, static_cast<const uint32_t*>(lab),
                     static_cast<const unsigned long long*>(tz), ti);
  hipLaunchKernelGGL(k_orient_final, dim3(pb), dim3(256), 0, c->stream, N, d_nrm, static_cast<const uint32_t*>(lab),
                     static_cast<const uint32_t*>(ti), d_out);
  PQ_HIP(hipGetLastError());
  return 0;
}

static int check_n(int64_t n) {
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  return 0;
}

static int check_orient_k(int32_t k) {
  if (k < 1 || k > kKnnMaxK) return fail(PYQSM_ERANGE, "k must be in [1, %d]", kKnnMaxK);
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_estimate_normals(const double* xyz, int64_t n, double radius, int32_t max_nn, const double* prev_normals,
                           double* normals, int32_t device) {
  PQ_API_RANGE("pyqsm_estimate_normals");
  PQ_TRY(check_n(n));
  PQ_TRY(check_max_nn(radius, max_nn));
  if (n > 0 && (!xyz || !normals)) return fail(PYQSM_EINVAL, "pyqsm_estimate_normals: NULL pointer");
  if (n == 0) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_xyz, *d_prev = nullptr, *d_out;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_out));
  PQ_TRY(copy_in(c, d_xyz, xyz, size_t(n) * 3));
  if (prev_normals) {
    PQ_TRY(upload(c, prev_normals, size_t(n) * 3, &d_prev));
  }
  PQ_TRY(normals_device(c, d_xyz, n, radius, max_nn, d_prev, d_out));
  PQ_TRY(fetch(c, normals, d_out, size_t(n) * 3));
  return 0;
}

int pyqsm_orient_normals_tangent_plane(const double* xyz, int64_t n, const double* normals, int32_t k,
                                       double* oriented, int32_t* rounds, int32_t device) {
  PQ_API_RANGE("pyqsm_orient_normals_tangent_plane");
  PQ_TRY(check_n(n));
  PQ_TRY(check_orient_k(k));
  if (n > 0 && (!xyz || !normals || !oriented)) return fail(PYQSM_EINVAL, "pyqsm_orient_normals_tangent_plane: NULL pointer");
  if (rounds) *rounds = 0;
  if (n == 0) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_xyz, *d_nrm, *d_out;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_nrm));
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_out));
  PQ_TRY(copy_in(c, d_xyz, xyz, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_nrm, normals, size_t(n) * 3));
  int32_t r = 0;
  PQ_TRY(orient_device(c, d_xyz, n, k, d_nrm, d_out, &r));
  PQ_TRY(fetch(c, oriented, d_out, size_t(n) * 3));
  if (rounds) *rounds = r;
  return 0;
}

int pyqsm_stem_cloud(const double* xyz, int64_t n, const double* prev_normals, double crop_offset, double radius,
                     int32_t max_nn, int32_t orient_k, double angle_cutoff, int64_t* keep, double* normals,
                     int64_t* m_out, int32_t device) {
  PQ_API_RANGE("pyqsm_stem_cloud");
  PQ_TRY(check_n(n));
  if (!m_out) return fail(PYQSM_EINVAL, "pyqsm_stem_cloud: NULL out-parameter");
  *m_out = 0;
  PQ_TRY(check_max_nn(radius, max_nn));
  PQ_TRY(check_orient_k(orient_k));
  if (!std::isfinite(crop_offset)) return fail(PYQSM_EINVAL, "crop_offset must be finite");
  if (std::isnan(angle_cutoff)) return fail(PYQSM_EINVAL, "angle_cutoff must not be NaN");
  if (n > 0 && (!xyz || !keep || !normals)) return fail(PYQSM_EINVAL, "pyqsm_stem_cloud: NULL pointer");
  if (n == 0) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int N = int(n);
  double *d_xyz, *d_prev = nullptr;
  PQ_TRY(upload(c, xyz, size_t(n) * 3, &d_xyz));
  if (prev_normals) {
    PQ_TRY(upload(c, prev_normals, size_t(n) * 3, &d_prev));
  }
  // crop: pyQSM removes z <= min z + offset, and skips the crop when that bound is exactly 0
  double mn[3], mx[3];
  PQ_TRY(cloud_bbox(c, d_xyz, n, mn, mx));
  const double bound = mn[2] + crop_offset;
  const double* cxyz = d_xyz;
  const double* cprev = d_prev;
  int64_t* c_idx = nullptr;
  int64_t m = n;
  if (bound != 0.0) {
    ProfScope ps(c, "stem_crop");
    int32_t* pos;
    double *nx, *np = nullptr;
    PQ_TRY(c->arena.get(size_t(n) + 1, &pos));
    PQ_TRY(c->arena.get(size_t(n) * 3, &nx));
    if (d_prev) PQ_TRY(c->arena.get(size_t(n) * 3, &np));
    PQ_TRY(c->arena.get(size_t(n), &c_idx));
    hipLaunchKernelGGL(k_crop_mask, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, N, d_xyz, bound, pos);
    PQ_HIP(hipGetLastError());
    PQ_TRY(compact_flagged(c, pos, n, c_idx, nullptr, d_xyz, nx, d_prev, np));
    int32_t cnt = 0;
    PQ_TRY(fetch(c, &cnt, pos + n));
    m = cnt;
    if (m == 0) return 0;
    cxyz = nx;
    cprev = np;
  }
  double *nrm, *ori;
  PQ_TRY(c->arena.get(size_t(m) * 3, &nrm));
  PQ_TRY(c->arena.get(size_t(m) * 3, &ori));
  PQ_TRY(normals_device(c, cxyz, m, radius, max_nn, cprev, nrm));
  int32_t rounds = 0;
  PQ_TRY(orient_device(c, cxyz, m, orient_k, nrm, ori, &rounds));
  int32_t* pos;
  double* k_nrm;
  int64_t* k_idx;
  PQ_TRY(c->arena.get(size_t(m) + 1, &pos));
  PQ_TRY(c->arena.get(size_t(m) * 3, &k_nrm));
  PQ_TRY(c->arena.get(size_t(m), &k_idx));
  {
    ProfScope ps(c, "stem_filter");
    hipLaunchKernelGGL(k_angle_mask, dim3(ceil_div(m + 1, 256)), dim3(256), 0, c->stream, int(m),
                       static_cast<const double*>(ori), angle_cutoff, 0, pos);
    PQ_HIP(hipGetLastError());
    PQ_TRY(compact_flagged(c, pos, m, k_idx, c_idx, ori, k_nrm));
  }
  int32_t cnt = 0;
  PQ_TRY(fetch(c, &cnt, pos + m));
  if (cnt > 0) {
    PQ_TRY(download(c, keep, k_idx, size_t(cnt)));
    PQ_TRY(download(c, normals, k_nrm, size_t(cnt) * 3));
    PQ_HIP(hipStreamSynchronize(c->stream));
  }
  *m_out = cnt;
  return 0;
}

}  // extern "C"
