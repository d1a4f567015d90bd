// features.hip — the per-point neighbourhood features pyQSM labels wood, leaf and epiphyte points
// with (pyQSM/exploration.py:62-90, utils/algo.py:8-22): jakteristics' compute_features (the
// covariance of every point within a radius, its eigen-decomposition and up to 14 eigenvalue
// features, after Hackel et al. 2016) and smooth_feature (a reducer over each query's k nearest
// points). Recollected from jakteristics, parity unpinned; tests/features_restatement.py states the
// contract in NumPy/SciPy.
//
// Features. The cloud is binned into cells of the radius (grid.hpp: ball_grid); one wave per point, in
// the grid's sorted order, walks the nine stencil runs 64 candidates at a time with the pieces of
// wave_select.hpp (the count, the two bisections, the append). Candidates inside the ball (d2 <= r2,
// or the L1 distance <= r) have their offsets o = p_j - p_i staged in LDS; every 64 staged offsets
// each lane adds one neighbour's first and second moments. The moments are fixed point: every
// term o_a (and the fp64 product o_a * o_b) is scaled by a power of two that maps the largest
// possible offset to 2^61 and rounded to an integer, and summed in 128 bits, lane partials folded
// by a butterfly. The sum is then exact, so the result does not depend on the order in which the
// grid's binning left the points of a cell, nor on the order of the input (integer additions only,
// no atomics). A point with more than max_k points in its ball keeps the max_k first by (distance,
// index): the threshold distance (kth_by_bits), then the index bound among the ties at it
// (kth_index). k_feat_finish turns the moments' covariance into the
// eigenvalues and e3 (pca.hpp sym3_eigh_desc) and writes the requested features in fp64.
//
// Smoothing. The k nearest of every query, ascending by (d2, index): the exact kNN (knn.hip) when
// the queries are the points themselves; otherwise k_query_knn, one wave per query over a grid of
// cells of R: with at least k points within R the k first by (d2, index) are exact (selected and
// sorted as wave_select.hpp says, ties at the k-th distance cut by index), the others are served
// again with R doubled. The neighbour table stays in the arena; k_smooth_reduce gathers each
// row's values into LDS and reduces them (mean: fp64 sum in neighbour order over k; median: ranks by
// (value, position), the mean of the two middle values for even k; min, max), NaN propagating as in
// NumPy.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "fixed128.hpp"
#include "grid.hpp"
#include "knn.hpp"
#include "pca.hpp"
#include "wave_select.hpp"

namespace pyqsm {

// (kKnnMaxK, knn.hpp: largest k of a smoothing)
static constexpr int kFeatCount = 14;      // jakteristics' FEATURE_NAMES
static constexpr int kFeatMaxCols = 32;    // columns one call may ask for
static constexpr int kFeatWaves = 4;       // waves per block of k_feat_moments
static constexpr int kQueryCap = 512;      // (d2, index) pairs k_query_knn sorts without bisection

// ---- fixed-point moments: fixed128.hpp (I128, acc128, fold128, to_double, FeatScale, add_moments) ----

// The distance the ball is tested with: d2 = ((dx*dx) + dy*dy) + dz*dz, or (|dx| + |dy|) + |dz|.
template <class CO, bool L1>
__device__ __forceinline__ double feat_dist(const CO& co, int q, double x, double y, double z, double& a, double& b,
                                            double& c) {
  co.get(q, a, b, c);
  if (L1) return (fabs(a - x) + fabs(b - y)) + fabs(c - z);
  return sqdist3(x, y, z, a, b, c);
}

// One wave per point at sorted position p. lim: r^2 (L2) or r (L1), inclusive. Writes the
// covariance entries (c00, c01, c02, c11, c12, c22) of the neighbours kept (np.cov's N - 1 divisor;
// zeros below two), their number used[i] and the ball's count cnt_out[i] before the cap.
template <class CO, bool L1>
__global__ __launch_bounds__(64 * kFeatWaves) void k_feat_moments(
    int n, const double* __restrict__ xyz, GridParams g, const int32_t* __restrict__ start,
    const int32_t* __restrict__ order, CO co, double lim, int max_k, FeatScale sc, double* __restrict__ cov,
    int32_t* __restrict__ used, int32_t* __restrict__ cnt_out) {
  __shared__ double sb[kFeatWaves][3][128];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = blockIdx.x * kFeatWaves + w;
  if (p >= n) return;  // whole wave
  const int i = order[p];
  const double x = xyz[3 * size_t(i)], y = xyz[3 * size_t(i) + 1], z = xyz[3 * size_t(i) + 2];
  StencilRuns rr;  // clamped like the points were binned
  point_stencil_runs(g, start, x, y, z, &rr);
  // candidate q at (a, b, c): in the ball and (d < tau, or d == tau and index <= ilim)
  auto kept = [&](int q, double tau, int ilim, double& a, double& b, double& c) {
    const double d = feat_dist<CO, L1>(co, q, x, y, z, a, b, c);
    return d <= lim && (d < tau || (d == tau && order[q] <= ilim));
  };
  auto count = [&](double tau, int ilim) {
    return wave_count(rr, [&](int q) {
      double a, b, c;
      return kept(q, tau, ilim, a, b, c);
    });
  };
  const int total = count(__builtin_inf(), 0x7FFFFFFF);
  double tau = __builtin_inf();
  int ilim = 0x7FFFFFFF;
  if (total > max_k) {  // the max_k-th distance, then the index bound that completes max_k among its ties
    tau = kth_by_bits(lim, max_k, [&](double t) { return count(t, 0x7FFFFFFF); });
    ilim = kth_index(n, max_k, [&](int ib) { return count(tau, ib); });
  }
  I128 M[9];
  for (int t = 0; t < 9; ++t) M[t] = I128{0ull, 0LL};
  int have = 0, N = 0;
  wave_candidates(rr, [&](int q, bool live) {
    double a = 0.0, b = 0.0, c = 0.0;
    bool take = false;
    if (live) take = kept(q, tau, ilim, a, b, c);
    const int slot = wave_append(take, have);
    if (take) {  // have was < 64, so slot < 128
      sb[w][0][slot] = a - x;
      sb[w][1][slot] = b - y;
      sb[w][2][slot] = c - z;
    }
    if (have >= 64) {
      wave_sync();
      add_moments(M, sc, sb[w][0][lane], sb[w][1][lane], sb[w][2][lane]);
      wave_sync();
      if (lane < have - 64) {
        sb[w][0][lane] = sb[w][0][lane + 64];
        sb[w][1][lane] = sb[w][1][lane + 64];
        sb[w][2][lane] = sb[w][2][lane + 64];
      }
      wave_sync();
      have -= 64;
      N += 64;
    }
  });
  wave_sync();
  if (lane < have) add_moments(M, sc, sb[w][0][lane], sb[w][1][lane], sb[w][2][lane]);
  N += have;
  for (int off = 32; off > 0; off >>= 1)
    for (int t = 0; t < 9; ++t) fold128(M[t], off);
  if (lane == 0) {
    double* o = cov + 6 * size_t(i);
    if (N >= 2) {
      const double dn = double(N);
      double s1[3];
      for (int a = 0; a < 3; ++a) s1[a] = to_double(M[a]) * sc.u1[a];
      const int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};
      for (int e = 0; e < 6; ++e) {
        const double s2 = to_double(M[3 + e]) * sc.u2[e];
        o[e] = (s2 - s1[A[e]] * (s1[B[e]] / dn)) / (dn - 1.0);
      }
    } else {
      for (int e = 0; e < 6; ++e) o[e] = 0.0;
    }
    used[i] = N;
    cnt_out[i] = total;
  }
}

struct FeatList {
  int n;
  int id[kFeatMaxCols];
};

// One lane per point: the eigenvalues (clamped to >= 0) and e3 (e3_z >= 0), then the requested
// features in jakteristics' FEATURE_NAMES numbering; all NaN when fewer than 3 neighbours were kept
// or lambda1 == 0.
__global__ __launch_bounds__(256) void k_feat_finish(int n, const double* __restrict__ cov,
                                                     const int32_t* __restrict__ used, FeatList fl,
                                                     double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* cv = cov + 6 * size_t(i);
  double l[3] = {0.0, 0.0, 0.0}, e[3] = {0.0, 0.0, 0.0};
  bool nan = used[i] < 3;
  if (!nan) {
    sym3_eigh_desc(Sym3{cv[0], cv[1], cv[2], cv[3], cv[4], cv[5]}, l, e);
    for (int s = 0; s < 3; ++s) l[s] = l[s] > 0.0 ? l[s] : 0.0;
    nan = !(l[0] > 0.0);
    if (e[2] < 0.0) {
      e[0] = -e[0];
      e[1] = -e[1];
      e[2] = -e[2];
    }
  }
  const double S = (l[0] + l[1]) + l[2];
  double* o = out + size_t(i) * fl.n;
  for (int f = 0; f < fl.n; ++f) {
    double v = __builtin_nan("");
    if (!nan) switch (fl.id[f]) {
        case 0: v = S; break;
        case 1: v = cbrt((l[0] * l[1]) * l[2]); break;
        case 2: {
          double h = 0.0;
          for (int s = 0; s < 3; ++s)
            if (l[s] > 0.0) h = h + l[s] * log(l[s]);
          v = -h;
          break;
        }
        case 3: v = (l[0] - l[2]) / l[0]; break;
        case 4: v = (l[1] - l[2]) / l[0]; break;
        case 5: v = (l[0] - l[1]) / l[0]; break;
        case 6: v = l[0] / S; break;
        case 7: v = l[1] / S; break;
        case 8: v = l[2] / S; break;
        case 9: v = l[2] / l[0]; break;
        case 10: v = 1.0 - fabs(e[2]); break;
        case 11: v = e[0]; break;
        case 12: v = e[1]; break;
        default: v = e[2]; break;
      }
    o[f] = v;
  }
}

// ---- smoothing: the k nearest of separate queries ------------------------------------------------
__global__ __launch_bounds__(256) void k_iota(int m, int32_t* __restrict__ list) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) list[i] = i;
}

// One wave per listed query: the points with d2 <= R2 (the grid's cells are at least R). Fewer than
// k: the query goes on the next list (integer atomic; a query's result does not depend on the
// round or the slot it is served in). Otherwise the k first by (d2, index) — all of them are
// within R — into idx[q * k ...].
template <class CO>
__global__ __launch_bounds__(128) void k_query_knn(int m_list, const int32_t* __restrict__ list,
                                                   const double* __restrict__ qry, GridParams g,
                                                   const int32_t* __restrict__ start,
                                                   const int32_t* __restrict__ order, CO co, double R2, int k,
                                                   int n_src, int32_t* __restrict__ idx,
                                                   int32_t* __restrict__ next, int32_t* __restrict__ n_next) {
  __shared__ double sd[2][kQueryCap];
  __shared__ int si[2][kQueryCap];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int t = blockIdx.x * 2 + w;
  if (t >= m_list) return;  // whole wave
  const int qi = list[t];
  const double x = qry[3 * size_t(qi)], y = qry[3 * size_t(qi) + 1], z = qry[3 * size_t(qi) + 2];
  StencilRuns rr;
  point_stencil_runs(g, start, x, y, z, &rr);
  auto count = [&](double tau, int ilim) {  // d2 <= R2 and (d2 < tau, or d2 == tau and index <= ilim)
    return wave_count(rr, [=](int q) {
      const double d = co.d2(q, x, y, z);
      return d <= R2 && (d < tau || (d == tau && order[q] <= ilim));
    });
  };
  const int total = count(__builtin_inf(), 0x7FFFFFFF);
  if (total < k) {
    if (lane == 0) next[atomicAdd(n_next, 1)] = qi;
    return;
  }
  double tau = __builtin_inf();
  int ilim = 0x7FFFFFFF;
  if (total > kQueryCap) {  // exactly k survive: the k-th d2, then the index bound among its ties
    tau = kth_by_bits(R2, k, [&](double t) { return count(t, 0x7FFFFFFF); });
    ilim = kth_index(n_src, k, [&](int ib) { return count(tau, ib); });
  }
  int have = 0;  // at most kQueryCap (all of them) or exactly k (after the bisections)
  wave_candidates(rr, [=, &have](int q, bool live) {
    double d = 0.0;
    int id = 0;
    bool take = false;
    if (live) {
      d = co.d2(q, x, y, z);
      id = order[q];
      const bool in = d <= R2, below = d < tau, tie = d == tau && id <= ilim;
      take = in && (below || tie);
    }
    const int slot = wave_append(take, have);
    if (take && slot < kQueryCap) {
      sd[w][slot] = d;
      si[w][slot] = id;
    }
  });
  have = have < kQueryCap ? have : kQueryCap;
  wave_sort_pairs(sd[w], si[w], have);
  for (int u = lane; u < k; u += 64) idx[size_t(qi) * k + u] = si[w][u];
}

// ---- smoothing: the reduction over each row of the neighbour table -------------------------------
// One wave per query row; per column the k values go through LDS. reducer 0 mean, 1 median, 2 min,
// 3 max.
__global__ __launch_bounds__(128) void k_smooth_reduce(int m, const int32_t* __restrict__ idx, int k,
                                                       const double* __restrict__ vals, int F, int reducer,
                                                       double* __restrict__ out) {
  __shared__ double sv[2][kKnnMaxK];
  __shared__ double ss[2][kKnnMaxK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q = blockIdx.x * 2 + w;
  if (q >= m) return;  // whole wave
  const int32_t* row = idx + size_t(q) * k;
  for (int f = 0; f < F; ++f) {
    bool nan_here = false;
    for (int t = lane; t < k; t += 64) {
      const double v = vals[size_t(row[t]) * F + f];
      sv[w][t] = v;
      nan_here = nan_here || v != v;
    }
    const bool any_nan = __ballot(nan_here) != 0ull;
    wave_sync();
    double res = 0.0;
    if (reducer == 1) {
      if (!any_nan) {  // rank by (value, position): a permutation, so ss is the sorted row
        for (int t = lane; t < k; t += 64) {
          const double v = sv[w][t];
          int rank = 0;
          for (int u = 0; u < k; ++u) {
            const double o = sv[w][u];
            rank += (o < v || (o == v && u < t)) ? 1 : 0;
          }
          ss[w][rank] = v;
        }
        wave_sync();
        res = (k & 1) ? ss[w][k >> 1] : (ss[w][(k >> 1) - 1] + ss[w][k >> 1]) / 2.0;
      } else {
        res = __builtin_nan("");
      }
    } else if (lane == 0) {
      if (reducer == 0) {
        double s = 0.0;
        for (int t = 0; t < k; ++t) s = s + sv[w][t];
        res = s / double(k);
      } else {
        res = sv[w][0];
        for (int t = 1; t < k; ++t) {
          const double v = sv[w][t];
          if (res != res) break;  // NaN stays
          if (v != v || (reducer == 2 ? v < res : v > res)) res = v;
        }
      }
    }
    if (lane == 0) out[size_t(q) * F + f] = res;
    wave_sync();  // the next column overwrites sv and ss
  }
}

// ---- host side -----------------------------------------------------------------------------------
static int check_count(int64_t n) {
  if (n < 0) return fail(PYQSM_EINVAL, "negative size");
  if (n > 0x7FFFFF00LL) return fail(PYQSM_ERANGE, "more than 2^31 points per call");
  return 0;
}

// The k nearest of the m queries d_qry among the n points d_src into d_idx [m, k] (k <= n).
static int query_knn_device(Ctx* c, const double* d_src, int64_t n, const double* d_qry, int64_t m, int k,
                            int32_t* d_idx) {
  int32_t *list, *next, *n_next;
  PQ_TRY(c->arena.get(size_t(m), &list));
  PQ_TRY(c->arena.get(size_t(m), &next));
  PQ_TRY(c->arena.get(1, &n_next));
  hipLaunchKernelGGL(k_iota, dim3(ceil_div(m, 256)), dim3(256), 0, c->stream, int(m), list);
  PQ_HIP(hipGetLastError());
  double box[6];
  bool all_f32 = false;
  PQ_TRY(cloud_bbox(c, d_src, n, box, box + 3, &all_f32));
  const double ext = std::max({box[3] - box[0], box[4] - box[1], box[5] - box[2]});
  // a first radius that holds about k points on a surface-like cloud; doubled for the queries
  // that find fewer
  double R = 0.5 * ext * std::sqrt(double(k) / double(n));
  if (!(R > 0) || !std::isfinite(R)) R = 1.0;
  int64_t left = m;
  while (left > 0) {
    if (!std::isfinite(R * R)) return fail(PYQSM_ERANGE, "query kNN: no radius holds k points");
    const Arena::Mark mk = c->arena.mark();
    DevGrid g;
    PQ_TRY(ball_grid(c, d_src, n, R, &g));
    PQ_HIP(hipMemsetAsync(n_next, 0, 4, c->stream));
    on_coords(g, [&](auto co) {
      hipLaunchKernelGGL(k_query_knn<decltype(co)>, dim3(ceil_div(left, 2)), dim3(128), 0, c->stream, int(left),
                         static_cast<const int32_t*>(list), d_qry, grid_params(g), g.start, g.order, co, R * R, k,
                         int(n), d_idx, next, n_next);
    });
    PQ_HIP(hipGetLastError());
    int32_t nn = 0;
    PQ_TRY(fetch(c, &nn, n_next));
    c->arena.rewind(mk);
    std::swap(list, next);
    left = nn;
    R *= 2.0;
  }
  return 0;
}

}  // namespace pyqsm

using namespace pyqsm;

extern "C" {

int pyqsm_geometric_features(const double* xyz, int64_t n, double radius, int32_t max_k, int32_t metric,
                             const int32_t* feature_ids, int32_t n_features, double* out, int32_t* counts,
                             int32_t device) {
  PQ_API_RANGE("pyqsm_geometric_features");
  PQ_TRY(check_count(n));
  if (!(radius > 0) || !std::isfinite(radius)) return fail(PYQSM_EINVAL, "radius must be positive and finite");
  if (max_k < 1) return fail(PYQSM_ERANGE, "max_k must be at least 1");
  if (metric != 1 && metric != 2) return fail(PYQSM_EINVAL, "metric must be 2 (L2) or 1 (L1)");
  if (n_features < 1 || n_features > kFeatMaxCols)
    return fail(PYQSM_ERANGE, "n_features must be in [1, %d]", kFeatMaxCols);
  if (!feature_ids) return fail(PYQSM_EINVAL, "pyqsm_geometric_features: NULL pointer");
  FeatList fl;
  fl.n = n_features;
  for (int f = 0; f < kFeatMaxCols; ++f) fl.id[f] = 0;
  for (int f = 0; f < n_features; ++f) {
    if (feature_ids[f] < 0 || feature_ids[f] >= kFeatCount)
      return fail(PYQSM_EINVAL, "feature id %d is not in [0, %d)", int(feature_ids[f]), kFeatCount);
    fl.id[f] = feature_ids[f];
  }
  if (n > 0 && (!xyz || !out)) return fail(PYQSM_EINVAL, "pyqsm_geometric_features: NULL pointer");
  if (n == 0) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  const int N = int(n);
  double *d_xyz, *cov, *d_out;
  int32_t *used, *cnt;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(n) * 6, &cov));
  PQ_TRY(c->arena.get(size_t(n) * n_features, &d_out));
  PQ_TRY(c->arena.get(size_t(n), &used));
  PQ_TRY(c->arena.get(size_t(n), &cnt));
  PQ_TRY(copy_in(c, d_xyz, xyz, size_t(n) * 3));
  DevGrid g;
  double box[6];
  {
    ProfScope ps(c, "features_grid");
    PQ_TRY(ball_grid(c, d_xyz, n, radius, &g, box));
  }
  // an offset inside the ball is at most the radius (one rounding more) and at most the extent
  double bound[3];
  for (int a = 0; a < 3; ++a) bound[a] = std::min(radius * (1.0 + 1.0 / 1048576.0), box[3 + a] - box[a]);
  const FeatScale sc = feat_scale(bound);
  {
    ProfScope ps(c, "features_moments");
    const double lim = metric == 2 ? radius * radius : radius;
    on_coords(g, [&](auto co) {
      if (metric == 2)
        hipLaunchKernelGGL((k_feat_moments<decltype(co), false>), dim3(ceil_div(n, kFeatWaves)),
                           dim3(64 * kFeatWaves), 0, c->stream, N, static_cast<const double*>(d_xyz), grid_params(g),
                           static_cast<const int32_t*>(g.start), static_cast<const int32_t*>(g.order), co, lim,
                           int(max_k), sc, cov, used, cnt);
      else
        hipLaunchKernelGGL((k_feat_moments<decltype(co), true>), dim3(ceil_div(n, kFeatWaves)),
                           dim3(64 * kFeatWaves), 0, c->stream, N, static_cast<const double*>(d_xyz), grid_params(g),
                           static_cast<const int32_t*>(g.start), static_cast<const int32_t*>(g.order), co, lim,
                           int(max_k), sc, cov, used, cnt);
    });
    PQ_HIP(hipGetLastError());
  }
  {
    ProfScope ps(c, "features_finish");
    hipLaunchKernelGGL(k_feat_finish, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, N,
                       static_cast<const double*>(cov), static_cast<const int32_t*>(used), fl, d_out);
    PQ_HIP(hipGetLastError());
  }
  PQ_TRY(download(c, out, d_out, size_t(n) * n_features));
  if (counts) PQ_TRY(download(c, counts, cnt, size_t(n)));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

int pyqsm_smooth_values(const double* xyz, int64_t n, const double* qry, int64_t m, const double* values, int32_t F,
                        int32_t k, int32_t reducer, double* out, int32_t* idx, int32_t device) {
  PQ_API_RANGE("pyqsm_smooth_values");
  PQ_TRY(check_count(n));
  PQ_TRY(check_count(m));
  if (!qry && m != n) return fail(PYQSM_EINVAL, "without queries m must equal n");
  if (k < 1 || k > kKnnMaxK) return fail(PYQSM_ERANGE, "k must be in [1, %d]", kKnnMaxK);
  if (k > n) return fail(PYQSM_EINVAL, "k = %d is larger than the %lld points", int(k), (long long)n);
  if (reducer < -1 || reducer > 3) return fail(PYQSM_EINVAL, "reducer must be in [-1, 3]");
  if (reducer >= 0 && (F < 1 || !values || !out)) return fail(PYQSM_EINVAL, "pyqsm_smooth_values: values and out needed");
  if (reducer < 0 && !idx) return fail(PYQSM_EINVAL, "pyqsm_smooth_values: reducer -1 needs idx");
  if (!xyz) return fail(PYQSM_EINVAL, "pyqsm_smooth_values: NULL pointer");
  if (reducer >= 0 && int64_t(F) * std::max<int64_t>(n, m) > (int64_t(1) << 40))
    return fail(PYQSM_ERANGE, "values too large");
  if (qry)
    for (int64_t t = 0; t < 3 * m; ++t)
      if (!std::isfinite(qry[t])) return fail(PYQSM_EINVAL, "query coordinates must be finite");
  if (m == 0) return 0;
  Call call(device);
  Ctx* c = call.c;
  if (!c) return PYQSM_ENODEV;
  double *d_xyz, *d_qry = nullptr, *d_d2 = nullptr;
  int32_t* d_idx;
  PQ_TRY(c->arena.get(size_t(n) * 3, &d_xyz));
  PQ_TRY(c->arena.get(size_t(m) * k, &d_idx));
  PQ_TRY(copy_in(c, d_xyz, xyz, size_t(n) * 3));
  {
    ProfScope ps(c, "smooth_knn");
    if (!qry) {
      PQ_TRY(c->arena.get(size_t(n) * k, &d_d2));
      PQ_TRY(knn_device(c, d_xyz, n, k, 0, d_idx, d_d2));
    } else {
      PQ_TRY(upload(c, qry, size_t(m) * 3, &d_qry));
      PQ_TRY(query_knn_device(c, d_xyz, n, d_qry, m, k, d_idx));
    }
  }
  if (reducer >= 0) {
    double *d_vals, *d_out;
    PQ_TRY(c->arena.get(size_t(n) * F, &d_vals));
    PQ_TRY(c->arena.get(size_t(m) * F, &d_out));
    PQ_TRY(copy_in(c, d_vals, values, size_t(n) * F));
    ProfScope ps(c, "smooth_reduce");
    hipLaunchKernelGGL(k_smooth_reduce, dim3(ceil_div(m, 2)), dim3(128), 0, c->stream, int(m),
                       static_cast<const int32_t*>(d_idx), int(k), static_cast<const double*>(d_vals), int(F),
                       int(reducer), d_out);
    PQ_HIP(hipGetLastError());
    PQ_TRY(download(c, out, d_out, size_t(m) * F));
  }
  if (idx) PQ_TRY(download(c, idx, d_idx, size_t(m) * k));
  PQ_HIP(hipStreamSynchronize(c->stream));
  return 0;
}

}  // extern "C"
