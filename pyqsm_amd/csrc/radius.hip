// radius.hip — fixed-radius queries on gfx950.
//
//   pyqsm_ball_query    all points within r of ONE centre: what
//                       scipy KDTree(points).query_ball_point(center, r) returns at
//                       pyQSM/utils/lib_integration.py:114-115 (find_neighbors_in_ball,
//                       called once per branch segment by qsm_generation.sphere_step;
//                       the reference rebuilds the KD-tree of the whole cloud every
//                       call). One HBM pass: 24 B per point, inclusive d <= r.
//   pyqsm_radius_mark   for a set of query points, the union of their (up to k nearest)
//                       neighbours within a distance bound: the index set that
//                       KDTree(src).query(query, k, distance_upper_bound=dist) yields at
//                       pyQSM/geometry/reconstruction.py:238-244 and
//                       pyQSM/tree_isolation.py:126-131,207-209. Strict d < dist, like
//                       cKDTree. The source cloud is binned into cells of edge `dist`;
//                       one lane per query walks its 27 cells (radius_walk.hpp). When more
//                       than k points lie inside the bound, the k-th smallest squared distance
//                       is found exactly and only those are marked.
//   pyqsm_radius_knn    the same neighbours as sorted padded tables, and pyqsm_radius_reduce,
//                       which reduces their value rows in the kernel: one wave per query
//                       (wave_select.hpp), the same selection as the walk to the bit.
// Squared distances are fp64, ((dx*dx)+dy*dy)+dz*dz, the accumulation of cKDTree.
#include "radius_walk.hpp"
#include "wave_select.hpp"

#include <algorithm>
#include <cmath>

namespace pyqsm {

__global__ __launch_bounds__(256) void k_ball_flags(int64_t n, const double* __restrict__ xyz,
                                                    double cx, double cy, double cz, double r2,
                                                    int32_t* __restrict__ flags) {
  int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
  if (i > n) return;
  flags[i] = i < n && sqdist3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cx, cy, cz) <= r2;
}

// One lane per query. walk<> and the tau selection live in radius_walk.hpp (shared with grow.hip).
template <class CO>
__global__ __launch_bounds__(256) void k_radius_mark(int m, const double* __restrict__ qry,
                                                     GridParams g, const int32_t* __restrict__ start,
                                                     const int32_t* __restrict__ order,
                                                     CO co, double r2,
                                                     int k, uint8_t* __restrict__ mark,
                                                     int32_t* __restrict__ counts,
                                                     const int32_t* __restrict__ qlab /*may be null*/,
                                                     int32_t* __restrict__ lab_out,
                                                     const int32_t* __restrict__ perm /*queries in cell order, may be null*/) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= m) return;
  const int i = perm ? perm[gid] : gid;
  const double x = qry[3 * i], y = qry[3 * i + 1], z = qry[3 * i + 2];
  const MarkSink sink{order, mark, qlab ? lab_out : nullptr, qlab ? qlab[i] : 0};
  const int c = radius_select(g, start, co, x, y, z, r2, k, sink);
  counts[i] = c < k ? c : k;
}


// ---- k nearest within a bound, as sorted padded tables (cKDTree.query semantics) --------
// One wave per query, with the pieces of wave_select.hpp: count the source points inside the bound;
// if there are more than k, find the k-th smallest squared distance (rare: k defaults to 500 at a
// 5 cm bound); collect the survivors in LDS, sort them by (d2, index) and write k entries, padded
// with (inf, n).
static constexpr int kKnnCap = 2048;  // largest k (LDS: 24 KB per wave)

// The front both kernels share: the neighbours of (x, y, z) — at most k, d2 < r2 — into sd / si (this
// wave's LDS, kKnnCap entries each), ascending by (d2, index). Returns how many. Whole wave.
template <class CO>
__device__ __forceinline__ int radius_collect_sorted(const GridParams& g, const int32_t* __restrict__ start,
                                                     const int32_t* __restrict__ order, CO co, double x, double y,
                                                     double z, double r2, int k, double* sd, int* si) {
  StencilRuns rr;
  point_stencil_runs(g, start, x, y, z, &rr);
  auto count_le = [&](double tau) {  // candidates with d2 < r2 and d2 <= tau
    return wave_count(rr, [=](int q) {
      const double d = co.d2(q, x, y, z);
      return d < r2 && d <= tau;
    });
  };
  int total = count_le(__builtin_inf());
  double tau = __builtin_inf();
  int budget = 0;  // ties at tau that still fit
  if (total > k) {
    tau = kth_by_bits(r2, k, count_le);
    const long long tb = __double_as_longlong(tau);
    const int n_below = tb == 0 ? 0 : count_le(__longlong_as_double(tb - 1));
    budget = k - n_below;
    total = k;
  }
  // everything below tau, and the ties at tau in candidate order until the budget is used up: the
  // tie rule of radius_walk.hpp's walk<2>
  int have = 0, ties = 0;
  if (total > 0)
    wave_candidates(rr, [=, &have, &ties](int q, bool live) {
      double d = 0.0;
      bool below = false, tie = false;
      if (live) {
        d = co.d2(q, x, y, z);
        below = d < r2 && d < tau;
        tie = d < r2 && d == tau;
      }
      const int tie_rank = wave_append(tie, ties);
      const bool take = below || (tie && tie_rank < budget);
      const int slot = wave_append(take, have);
      if (take) {
        sd[slot] = d;
        si[slot] = order[q];
      }
    });
  wave_sort_pairs(sd, si, have);
  return have;
}

template <class CO>
__global__ __launch_bounds__(128) void k_radius_knn(int m, const double* __restrict__ qry, GridParams g,
                                                    const int32_t* __restrict__ start,
                                                    const int32_t* __restrict__ order,
                                                    CO co, double r2, int k,
                                                    int n_src, int64_t* __restrict__ out_idx,
                                                    double* __restrict__ out_dist) {
  __shared__ double sd[2][kKnnCap];
  __shared__ int si[2][kKnnCap];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 2 + w;
  if (i >= m) return;  // whole wave
  const double x = qry[3 * i], y = qry[3 * i + 1], z = qry[3 * i + 2];
  const int have = radius_collect_sorted(g, start, order, co, x, y, z, r2, k, sd[w], si[w]);
  for (int t = lane; t < k; t += 64) {
    const bool real = t < have;
    out_idx[size_t(i) * k + t] = real ? int64_t(si[w][t]) : int64_t(n_src);
    out_dist[size_t(i) * k + t] = real ? sqrt(sd[w][t]) : __builtin_inf();
  }
}

// ---- the same neighbours, reduced in the kernel -------------------------------------------
// pyQSM's expand_features_to_orig / get_smoothed_features (canopy_metrics.py:236-252, 564-570) take
// the padded tables above to the host and reduce values[nbrs] there: 6 KB per query at k = 500.
// Here the sorted list stays in LDS. The distances are no longer needed after the sort, so their
// 16 KB hold the neighbours' value rows, gathered by the whole wave a tile of kKnnCap / F
// neighbours at a time; lane f < F then folds column f in neighbour order, one operation at a time
// (the mean's sum from 0.0, as pyqsm_smooth_values): no atomics, the same bits on every run.
// reducer: 0 mean, 2 min, 3 max (NaN propagates), 4 first.
static constexpr int kReduceMaxF = 64;

template <class CO>
__global__ __launch_bounds__(128) void k_radius_reduce(int m, const double* __restrict__ qry, GridParams g,
                                                       const int32_t* __restrict__ start,
                                                       const int32_t* __restrict__ order, CO co, double r2, int k,
                                                       const double* __restrict__ values, int F, int reducer,
                                                       int64_t empty_row, double* __restrict__ out,
                                                       int32_t* __restrict__ counts) {
  __shared__ double sd[2][kKnnCap];
  __shared__ int si[2][kKnnCap];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int i = blockIdx.x * 2 + w;
  if (i >= m) return;  // whole wave
  const double x = qry[3 * i], y = qry[3 * i + 1], z = qry[3 * i + 2];
  const int have = radius_collect_sorted(g, start, order, co, x, y, z, r2, k, sd[w], si[w]);
  if (counts && lane == 0) counts[i] = have;
  double* o = out + size_t(i) * F;
  if (have == 0) {
    if (lane < F) o[lane] = empty_row >= 0 ? values[size_t(empty_row) * F + lane] : __builtin_nan("");
    return;
  }
  if (reducer == 4) {
    if (lane < F) o[lane] = values[size_t(si[w][0]) * F + lane];
    return;
  }
  double* stage = sd[w];
  const int tile = kKnnCap / F;  // neighbours whose rows fit the stage
  double acc = 0.0;
  bool nan = false;
  for (int t0 = 0; t0 < have; t0 += tile) {
    const int cnt = min(tile, have - t0);
    for (int e = lane; e < cnt * F; e += 64) {
      const int nb = e / F;
      stage[e] = values[size_t(si[w][t0 + nb]) * F + (e - nb * F)];
    }
    wave_sync();
    if (lane < F) {
      if (reducer == 0) {
        for (int q = 0; q < cnt; ++q) acc = acc + stage[q * F + lane];
      } else {
        for (int q = 0; q < cnt; ++q) {
          const double v = stage[q * F + lane];
          nan = nan || v != v;
          if ((t0 == 0 && q == 0) || (reducer == 2 ? v < acc : v > acc)) acc = v;
        }
      }
    }
    wave_sync();
  }
  if (lane < F) o[lane] = reducer == 0 ? acc / double(have) : (nan ? __builtin_nan("") : acc);
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_ball_query(const double* xyz, int64_t n, const double center[3], double radius,
                     int64_t* out_idx, int64_t* count, int32_t device) {
  PQ_API_RANGE("pyqsm_ball_query");
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (count) *count = 0;
  if (n == 0) return 0;
  if (!xyz || !center || !out_idx || !count)
    return fail(PYQSM_EINVAL, "pyqsm_ball_query: NULL pointer");
  if (!(radius >= 0)) return fail(PYQSM_EINVAL, "radius must be >= 0");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double* d_xyz;
  int32_t* d_flags;
  int64_t* d_out;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(n) + 1, &d_flags));
  PQ_TRY(c->arena.get(size_t(n), &d_out));
  PQ_TRY(copy_in(c, d_xyz, xyz, size_t(n) * 3));
  {
    ProfScope ps(c, "ball_query");
    hipLaunchKernelGGL(k_ball_flags, dim3(ceil_div(n + 1, 256)), dim3(256), 0, c->stream, n, d_xyz,
                       center[0], center[1], center[2], radius * radius, d_flags);
    PQ_TRY(compact_flagged(c, d_flags, n, d_out));
  }
  int32_t total = 0;
  PQ_TRY(fetch(c, &total, d_flags + n));
  if (total)
    PQ_TRY(download(c, out_idx, d_out, size_t(total)));
  PQ_HIP(hipStreamSynchronize(c->stream));
  *count = total;
  return 0;
}

int pyqsm_radius_mark(const double* src, int64_t n, const double* qry, int64_t m, double radius,
                      int32_t k_cap, uint8_t* mark, int32_t* counts, int32_t device) {
  PQ_API_RANGE("pyqsm_radius_mark");
  if (n < 0 || m < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n > 0 && (!src || !mark)) return fail(PYQSM_EINVAL, "pyqsm_radius_mark: NULL pointer");
  if (m > 0 && (!qry || !counts)) return fail(PYQSM_EINVAL, "pyqsm_radius_mark: NULL pointer");
  if (!(radius > 0) || !std::isfinite(radius)) return fail(PYQSM_EINVAL, "radius must be positive");
  if (k_cap <= 0) return fail(PYQSM_EINVAL, "k must be positive");
  if (n > 0) memset(mark, 0, size_t(n));
  if (m > 0) memset(counts, 0, size_t(m) * 4);
  if (n == 0 || m == 0) return 0;
  if (m > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 query points per call");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_src, *d_qry;
  uint8_t* d_mark;
  int32_t* d_counts;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_src));
  PQ_TRY(c->arena.get(size_t(m) * 3, &d_qry));
  PQ_TRY(c->arena.get(size_t(n), &d_mark));
  PQ_TRY(c->arena.get(size_t(m), &d_counts));
  PQ_TRY(copy_in(c, d_src, src, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_qry, qry, size_t(m) * 3));
  PQ_HIP(hipMemsetAsync(d_mark, 0, size_t(n), c->stream));
  DevGrid g;
  PQ_TRY(radius_grid(c, d_src, n, radius, &g));
  const GridParams rg = grid_params(g);
  {
    ProfScope ps(c, "radius_mark");
    int32_t* perm = nullptr;
    PQ_TRY(query_order(c, d_qry, m, rg, g.ncell, &perm));
    on_coords(g, [&](auto co) {
      hipLaunchKernelGGL(k_radius_mark<decltype(co)>, dim3(ceil_div(m, 256)), dim3(256), 0, c->stream, int(m), d_qry,
                         rg, g.start, g.order, co, radius * radius, k_cap, d_mark, d_counts,
                         static_cast<const int32_t*>(nullptr), static_cast<int32_t*>(nullptr),
                         static_cast<const int32_t*>(perm));
    });
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(download(c, mark, d_mark, size_t(n)));
  PQ_TRY(download(c, counts, d_counts, size_t(m)));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int pyqsm_radius_knn(const double* src, int64_t n, const double* qry, int64_t m, double radius,
                     int32_t k, int64_t* idx, double* dist, int32_t device) {
  PQ_API_RANGE("pyqsm_radius_knn");
  if (n < 0 || m < 0) return fail(PYQSM_EINVAL, "negative size");
  if (k <= 0 || k > kKnnCap) return fail(PYQSM_ERANGE, "k must be in [1, %d]", kKnnCap);
  if (m > 0 && (!qry || !idx || !dist)) return fail(PYQSM_EINVAL, "pyqsm_radius_knn: NULL pointer");
  if (n > 0 && !src) return fail(PYQSM_EINVAL, "pyqsm_radius_knn: NULL pointer");
  if (!(radius > 0) || !std::isfinite(radius)) return fail(PYQSM_EINVAL, "radius must be positive");
  if (m == 0) return 0;
  if (m > 0x7FFFFF00LL || n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  if (n == 0) {  // nothing to find: every slot is padding
    for (int64_t t = 0; t < m * k; ++t) {
      idx[t] = 0;
      dist[t] = HUGE_VAL;
    }
    return 0;
  }
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_src, *d_qry, *d_dist;
  int64_t* d_idx;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_src));
  PQ_TRY(c->arena.get(size_t(m) * 3, &d_qry));
  PQ_TRY(c->arena.get(size_t(m) * k, &d_idx));
  PQ_TRY(c->arena.get(size_t(m) * k, &d_dist));
  PQ_TRY(copy_in(c, d_src, src, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_qry, qry, size_t(m) * 3));
  DevGrid g;
  PQ_TRY(radius_grid(c, d_src, n, radius, &g));
  const GridParams rg = grid_params(g);
  {
    ProfScope ps(c, "radius_knn");
    on_coords(g, [&](auto co) {
      hipLaunchKernelGGL(k_radius_knn<decltype(co)>, dim3(ceil_div(m, 2)), dim3(128), 0, c->stream, int(m), d_qry, rg,
                         g.start, g.order, co, radius * radius, k, int(n), d_idx, d_dist);
    });
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(download(c, idx, d_idx, size_t(m) * k));
  PQ_TRY(download(c, dist, d_dist, size_t(m) * k));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int pyqsm_radius_reduce(const double* src, int64_t n, const double* qry, int64_t m, double radius, int32_t k,
                        const double* values, int32_t F, int32_t reducer, int64_t empty_row, double* out,
                        int32_t* counts, int32_t device) {
  PQ_API_RANGE("pyqsm_radius_reduce");
  if (n < 0 || m < 0) return fail(PYQSM_EINVAL, "negative size");
  if (k <= 0 || k > kKnnCap) return fail(PYQSM_ERANGE, "k must be in [1, %d]", kKnnCap);
  if (F < 1 || F > kReduceMaxF) return fail(PYQSM_ERANGE, "F must be in [1, %d]", kReduceMaxF);
  if (reducer != 0 && reducer != 2 && reducer != 3 && reducer != 4)
    return fail(PYQSM_EINVAL, "reducer must be 0 (mean), 2 (min), 3 (max) or 4 (first), got %d", int(reducer));
  if (!(radius > 0) || !std::isfinite(radius)) return fail(PYQSM_EINVAL, "radius must be positive");
  if (empty_row < -1 || empty_row >= n) return fail(PYQSM_EINVAL, "empty_row must be -1 or a row of values");
  if (m > 0 && (!qry || !out)) return fail(PYQSM_EINVAL, "pyqsm_radius_reduce: NULL pointer");
  if (n > 0 && (!src || !values)) return fail(PYQSM_EINVAL, "pyqsm_radius_reduce: NULL pointer");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 source points per call");
  if (m == 0) return 0;
  if (n == 0) {  // nothing to find: every neighbourhood is empty (and empty_row is -1)
    for (int64_t t = 0; t < m * F; ++t) out[t] = std::nan("");
    if (counts) memset(counts, 0, size_t(m) * 4);
    return 0;
  }
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_src, *d_val;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_src));
  PQ_TRY(c->arena.get(size_t(n) * F, &d_val));
  PQ_TRY(copy_in(c, d_src, src, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_val, values, size_t(n) * F));
  DevGrid g;
  PQ_TRY(radius_grid(c, d_src, n, radius, &g));
  const GridParams rg = grid_params(g);
  // queries per pass: about 256 MB of arena for the queries and their results, as pyqsm_forest_predict
  const size_t per_q = 24 + size_t(F) * 8 + 4;
  const int64_t chunk = std::min<int64_t>(m, std::max<int64_t>(2, int64_t((size_t(256) << 20) / per_q)));
  double *d_qry, *d_out;
  int32_t* d_cnt = nullptr;
  PQ_TRY(c->arena.get(size_t(chunk) * 3, &d_qry));
  PQ_TRY(c->arena.get(size_t(chunk) * F, &d_out));
  if (counts) PQ_TRY(c->arena.get(size_t(chunk), &d_cnt));
  for (int64_t r0 = 0; r0 < m; r0 += chunk) {
    const int64_t mc = std::min(chunk, m - r0);
    PQ_TRY(copy_in(c, d_qry, qry + size_t(r0) * 3, size_t(mc) * 3));
    {
      ProfScope ps(c, "radius_reduce");
      on_coords(g, [&](auto co) {
        hipLaunchKernelGGL(k_radius_reduce<decltype(co)>, dim3(ceil_div(mc, 2)), dim3(128), 0, c->stream, int(mc), d_qry,
                           rg, g.start, g.order, co, radius * radius, k, static_cast<const double*>(d_val), F, reducer,
                           empty_row, d_out, d_cnt);
      });
      PQ_HIP(hipGetLastError());
    }
    PQ_TRY(download(c, out + size_t(r0) * F, d_out, size_t(mc) * F));
    if (counts) PQ_TRY(download(c, counts + r0, d_cnt, size_t(mc)));
  }
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int pyqsm_radius_label(const double* src, int64_t n, const double* qry, int64_t m,
                       const int32_t* qry_label, double radius, int32_t k_cap, int32_t* label,
                       int32_t* counts, int32_t device) {
  PQ_API_RANGE("pyqsm_radius_label");
  if (n < 0 || m < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n > 0 && (!src || !label)) return fail(PYQSM_EINVAL, "pyqsm_radius_label: NULL pointer");
  if (m > 0 && (!qry || !qry_label || !counts))
    return fail(PYQSM_EINVAL, "pyqsm_radius_label: NULL pointer");
  if (!(radius > 0) || !std::isfinite(radius)) return fail(PYQSM_EINVAL, "radius must be positive");
  if (k_cap <= 0) return fail(PYQSM_EINVAL, "k must be positive");
  for (int64_t i = 0; i < n; ++i) label[i] = -1;
  if (m > 0) memset(counts, 0, size_t(m) * 4);
  if (n == 0 || m == 0) return 0;
  for (int64_t i = 0; i < m; ++i)
    if (qry_label[i] < 0) return fail(PYQSM_EINVAL, "query labels must be >= 0");
  if (m > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 query points per call");
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_src, *d_qry;
  int32_t *d_lab, *d_counts, *d_qlab;
  uint8_t* d_mark;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_src));
  PQ_TRY(c->arena.get(size_t(m) * 3, &d_qry));
  PQ_TRY(c->arena.get(size_t(n), &d_lab));
  PQ_TRY(c->arena.get(size_t(m), &d_counts));
  PQ_TRY(c->arena.get(size_t(m), &d_qlab));
  PQ_TRY(c->arena.get(1, &d_mark));
  PQ_TRY(copy_in(c, d_src, src, size_t(n) * 3));
  PQ_TRY(copy_in(c, d_qry, qry, size_t(m) * 3));
  PQ_TRY(copy_in(c, d_qlab, qry_label, size_t(m)));
  PQ_HIP(hipMemsetAsync(d_lab, 0x7F, size_t(n) * 4, c->stream));  // 0x7F7F7F7F > any label
  DevGrid g;
  PQ_TRY(radius_grid(c, d_src, n, radius, &g));
  const GridParams rg = grid_params(g);
  {
    ProfScope ps(c, "radius_label");
    int32_t* perm = nullptr;
    PQ_TRY(query_order(c, d_qry, m, rg, g.ncell, &perm));
    on_coords(g, [&](auto co) {
      hipLaunchKernelGGL(k_radius_mark<decltype(co)>, dim3(ceil_div(m, 256)), dim3(256), 0, c->stream, int(m), d_qry,
                         rg, g.start, g.order, co, radius * radius, k_cap, d_mark, d_counts, d_qlab, d_lab,
                         static_cast<const int32_t*>(perm));
    });
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(download(c, label, d_lab, size_t(n)));
  PQ_TRY(download(c, counts, d_counts, size_t(m)));
  PQ_HIP(hipStreamSynchronize(c->stream));
  for (int64_t i = 0; i < n; ++i)
    if (label[i] == 0x7F7F7F7F) label[i] = -1;
  return 0;
}

}  // extern "C"
