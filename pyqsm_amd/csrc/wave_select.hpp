// wave_select.hpp — the wave-per-query select-and-sort of the ball kernels: what k_normal_hybrid
// (normals.hip), k_feat_moments and k_query_knn (features.hip) and radius_collect_sorted (radius.hip)
// share. One wave serves one query over the nine stencil runs of point_stencil_runs (grid.hpp), 64
// candidates per step: it counts the candidates that pass a predicate, bisects the k-th smallest
// distance (and, where ties are cut by index, the index bound) when too many pass, appends the
// survivors to LDS and sorts them by (d2, index).
//
// A caller states what is its own: the distance expression, the strictness of the bound, when the
// bisection is worth it, and the rule for ties at the k-th distance (normals: all of them, and a
// flag when they do not fit; features and k_query_knn: up to an index bound; radius: in candidate
// order up to a budget, as radius_walk.hpp's lane-per-query walk takes them).
//
// Every function here is called by the whole wave, all 64 lanes in the same control flow: they
// ballot. This is not the snapping bisection of radius_walk.hpp (kth_bound): a wave counts 64
// candidates per step and needs no minima along the way.
//
// Everything is forced inline and costs nothing (profiles/wave_select_resource_usage.txt), with one
// thing to know: a per-candidate lambda captures what its predicate compares BY VALUE ([=], and by
// reference only the counters it advances). Behind a by-reference capture `d < r2 && d <= tau`
// reads tau through a pointer the compiler will not load from speculatively, so the && stays a
// branch, one more exec-mask region per 64 candidates: 4 to 7 % on k_normal_hybrid and the radius
// kernels (profiles/wave_select_ab.txt, session 1).
#pragma once
#include "grid.hpp"

namespace pyqsm {

// What one lane wrote to LDS before, every lane of the wave may read after.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// f(q, live) on every lane for the candidates of the nine runs, 64 sorted positions per step, in run
// order; live == false on the lanes past a run's end, where q is not a position to read.
template <class F>
__device__ __forceinline__ void wave_candidates(const StencilRuns& rr, F&& f) {
  const int lane = threadIdx.x & 63;
  for (int r = 0; r < 9; ++r)
    for (int base = rr.qb[r]; base < rr.qe[r]; base += 64) {
      const int q = base + lane;
      f(q, q < rr.qe[r]);
    }
}

// The number of candidates q for which pred(q) holds.
template <class P>
__device__ __forceinline__ int wave_count(const StencilRuns& rr, P&& pred) {
  int cnt = 0;
  wave_candidates(rr, [&](int q, bool live) {
    bool in = false;
    if (live) in = pred(q);
    cnt += __popcll(__ballot(in));
  });
  return cnt;
}

// This lane's slot behind `have` entries among the lanes that take (meaningful where take holds);
// have += the number of lanes that take. Whether the slot still fits is the caller's test.
__device__ __forceinline__ int wave_append(bool take, int& have) {
  const unsigned long long kb = __ballot(take);
  const int slot = have + __popcll(kb & ((1ull << (threadIdx.x & 63)) - 1ull));
  have += __popcll(kb);
  return slot;
}

// The smallest double t in [0, bound] with count_le(t) >= k, by bisection on the bit pattern (a
// non-negative double orders as its bits); count_le(bound) >= k is the caller's.
template <class C>
__device__ __forceinline__ double kth_by_bits(double bound, int k, C&& count_le) {
  unsigned long long lo = 0, hi = (unsigned long long)__double_as_longlong(bound);
  while (lo < hi) {
    const unsigned long long mid = lo + ((hi - lo) >> 1);
    if (count_le(__longlong_as_double((long long)mid)) >= k) hi = mid;
    else lo = mid + 1;
  }
  return __longlong_as_double((long long)lo);
}

// The smallest index bound i in [0, n - 1] with count_upto(i) >= k.
template <class C>
__device__ __forceinline__ int kth_index(int n, int k, C&& count_upto) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (count_upto(mid) >= k) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// Sorts the `have` pairs (sd[t], si[t]) of this wave's LDS ascending by (d2, index): padded to the
// next power of two with (inf, 0x7FFFFFFF), which sort behind every real pair, then a bitonic
// network. sd and si hold at least that power of two. The result is visible to the whole wave.
__device__ __forceinline__ void wave_sort_pairs(double* sd, int* si, int have) {
  const int lane = threadIdx.x & 63;
  int np2 = 1;
  while (np2 < have) np2 <<= 1;
  for (int t = have + lane; t < np2; t += 64) {
    sd[t] = __builtin_inf();
    si[t] = 0x7FFFFFFF;
  }
  wave_sync();
  for (int k2 = 2; k2 <= np2; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < np2; t += 64) {
        const int u = t ^ j;
        if (u > t) {
          const double da = sd[t], db = sd[u];
          const int ia = si[t], ib = si[u];
          const bool a_gt_b = da > db || (da == db && ia > ib);
          if (a_gt_b == ((t & k2) == 0)) {
            sd[t] = db;
            si[t] = ib;
            sd[u] = da;
            si[u] = ia;
          }
        }
      }
      wave_sync();
    }
}

}  // namespace pyqsm
