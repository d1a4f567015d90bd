// radius_walk.hpp — the lane-per-query walk of the fixed-radius kernels: what k_radius_mark
// (radius.hip) and the region growing's frontier walk (grow.hip) share, so that both select the
// same source points to the bit — one d2 expression, one strict bound, one tau, one tie rule.
#pragma once
#include "grid.hpp"

namespace pyqsm {

// What walk<2> does with a selected source point (its SORTED position q); the counting modes take
// NoSink.
struct NoSink {
  __device__ __forceinline__ void operator()(int) const {}
};
// pyqsm_radius_mark / pyqsm_radius_label: a byte, or the smallest label, per ORIGINAL index.
struct MarkSink {
  const int32_t* __restrict__ order;
  uint8_t* __restrict__ mark;
  int32_t* __restrict__ lab_out;  // null: mark
  int lab;
  __device__ __forceinline__ void operator()(int q) const {
    if (lab_out) atomicMin(&lab_out[order[q]], lab);
    else mark[order[q]] = 1;
  }
};
// Region growing: the smallest cluster index into the candidate word of a point that is still free,
// in sorted position space (no order[q] gather); an owned point counts towards the k nearest but
// needs no atomic at all.
struct FreeMinSink {
  const int32_t* __restrict__ owner;
  int32_t* __restrict__ cand;
  int lab;
  __device__ __forceinline__ void operator()(int q) const {
    if (owner[q] < 0) atomicMin(&cand[q], lab);
  }
};

// MODE 0: count of source points with d2 < r2.  MODE 1: count with d2 <= tau.
// MODE 2: sink(q) for every source point with d2 < bound (bound = r2, or tau plus ties).
// MODE 3: as MODE 1, and *below = the largest d2 <= tau, *above = the smallest d2 > tau (both among
//         the candidates with d2 < r2; -1 / +inf when there is none).
template <int MODE, class CO, class SINK>
__device__ __forceinline__ int walk(const GridParams& g, const int32_t* __restrict__ start, CO co, double x,
                                    double y, double z, double r2, double tau, int budget, SINK sink,
                                    double* below = nullptr, double* above = nullptr) {
  // The query's cell, clamped into the grid the way the sources were binned (grid.hpp: clamped_cell):
  // the grid may cover less than the cloud (grid.hpp: radius_grid), and a clamp moves no two points
  // further apart, so whatever is within the radius of a query outside still sits in the 27 cells
  // around its clamped cell; the distance test is on the true coordinates.
  int cx, cy, cz;
  clamped_cell(g, x, y, z, &cx, &cy, &cz);
  int cnt = 0;
  double lo_v = -1.0, hi_v = __builtin_inf();
  for (int dz = -1; dz <= 1; ++dz) {
    const int zz = cz + dz;
    if (zz < 0 || zz >= g.nz) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = cy + dy;
      if (yy < 0 || yy >= g.ny) continue;
      const int x0 = cx - 1 < 0 ? 0 : cx - 1, x1 = cx + 1 >= g.nx ? g.nx - 1 : cx + 1;
      const int row = (zz * g.ny + yy) * g.nx;
      for (int q = start[row + x0]; q < start[row + x1 + 1]; ++q) {
        const double d = co.d2(q, x, y, z);
        if (MODE == 0) cnt += d < r2;
        if (MODE == 1) cnt += d < r2 && d <= tau;
        if (MODE == 3 && d < r2) {
          if (d <= tau) {
            ++cnt;
            lo_v = d > lo_v ? d : lo_v;
          } else {
            hi_v = d < hi_v ? d : hi_v;
          }
        }
        if (MODE == 2) {
          bool take = d < r2 && d < tau;
          if (!take && d < r2 && d == tau && cnt < budget) {  // ties at the k-th distance
            take = true;
            ++cnt;
          }
          if (take) sink(q);
        }
      }
    }
  }
  if (MODE == 3) {
    *below = lo_v;
    *above = hi_v;
  }
  return cnt;
}

// For a query with more than k source points inside the bound: *tau = the k-th smallest squared
// distance, *budget = how many of the points AT tau still fit (walk<2> takes them in walk order).
template <class CO>
__device__ __forceinline__ void kth_bound(const GridParams& g, const int32_t* __restrict__ start, CO co, double x,
                                          double y, double z, double r2, int k, double* tau_out, int* budget_out) {
  // k-th smallest squared distance = the smallest DATA value v with #{d2 <= v} >= k. Round 2 bisected the
  // 63-bit pattern (62 walks over ~1000 candidates for every query with more than k points in reach — half
  // of a forest's points at k = 200, radius 0.1: the branches — 8 ms per 100 k queries). Now the bisection
  // runs on VALUES and snaps to the data: a walk also returns the largest candidate <= t and the smallest
  // > t, so every walk discards half of the interval AND everything that is not a candidate's distance:
  // ~log2(candidates) walks. Same tau, to the bit.
  double L = -1.0;  // #{d2 <= L} < k
  double H = 0.0;   // a data value with #{d2 <= H} >= k: the largest candidate below r2
  {
    double b0, a0;
    (void)walk<3>(g, start, co, x, y, z, r2, __builtin_inf(), 0, NoSink{}, &b0, &a0);
    H = b0;
  }
  for (int it = 0; it < 200 && L < H; ++it) {
    double t = L + (H - L) * 0.5;
    if (!(t > L) || !(t < H)) t = L < 0.0 ? 0.0 : nextafter(L, H);  // neighbours in fp64: test L's successor
    if (!(t < H)) break;
    double b1, a1;
    const int cnt = walk<3>(g, start, co, x, y, z, r2, t, 0, NoSink{}, &b1, &a1);
    if (cnt >= k) {
      H = b1;  // the largest candidate <= t still has >= k at or below it
    } else {
      L = t;
      if (!(a1 < H)) break;  // no candidate between t and H: H is the k-th
    }
  }
  const double tau = H;
  const unsigned long long lo = (unsigned long long)__double_as_longlong(tau);
  // points strictly below tau are all taken; ties at tau fill what is left of k
  const double below = lo == 0 ? -1.0 : __longlong_as_double((long long)(lo - 1));
  const int n_below = lo == 0 ? 0 : walk<1>(g, start, co, x, y, z, r2, below, 0, NoSink{});
  *tau_out = tau;
  *budget_out = k - n_below;
}

// One query, start to end: sink(q) for its (at most k nearest) source points with d2 < r2. Returns
// how many source points lie inside the bound (the caller's count is min(that, k)).
template <class CO, class SINK>
__device__ __forceinline__ int radius_select(const GridParams& g, const int32_t* __restrict__ start, CO co, double x,
                                             double y, double z, double r2, int k, SINK sink) {
  const int c = walk<0>(g, start, co, x, y, z, r2, 0.0, 0, NoSink{});
  if (c == 0) return 0;
  double tau = __builtin_inf();
  int budget = 0;
  if (c > k) kth_bound(g, start, co, x, y, z, r2, k, &tau, &budget);
  (void)walk<2>(g, start, co, x, y, z, r2, tau, budget, sink);
  return c;
}

}  // namespace pyqsm
