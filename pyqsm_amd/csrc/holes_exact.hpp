// holes_exact.hpp — the arithmetic of the minimum-area hole patch, for the host and
// the device: the kernels of holes.hip and the stand-alone check program holes_check.cpp run this text.
//
// A loop v_0 .. v_{L-1} with points p_m (fp64). W(i, k), i < k, is the least area of a triangulation of
// the sub-polygon i .. k, S(i, k) the apex j that attains it:
//   W(i, i + 1) = 0;  W(i, k) = min over j in (i, k), ascending, of (W(i, j) + W(j, k)) + A(i, j, k),
// a later j replaces an earlier one only when strictly smaller. A is the triangle area of
// pyqsm_mesh_topology: every cross component a*b - c*d without fused multiply-adds (-ffp-contract=off).
//
// The table is stored by diagonals: entry (i, k) at fill_at(L, i, k) = off(k - i) + i with
// off(d) = (d - 1) L - (d - 1) d / 2, L (L - 1) / 2 entries in all. Along a diagonal consecutive i are
// consecutive addresses, also for the two operands of a relaxation step.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PQ_FILL_HD __host__ __device__ __forceinline__
#else
#define PQ_FILL_HD inline
#endif

namespace pyqsm {

PQ_FILL_HD int fill_table_size(int L) { return L * (L - 1) / 2; }

PQ_FILL_HD int fill_at(int L, int i, int k) {
  const int d = k - i;
  return (d - 1) * L - (d - 1) * d / 2 + i;
}

// p: three doubles per point
PQ_FILL_HD double fill_area(const double* pi, const double* pj, const double* pk) {
  const double ux = pj[0] - pi[0], uy = pj[1] - pi[1], uz = pj[2] - pi[2];
  const double vx = pk[0] - pi[0], vy = pk[1] - pi[1], vz = pk[2] - pi[2];
  const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
  return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

// The relaxation of entry (i, k), k - i >= 2, from the finished shorter diagonals. pts: [L,3].
PQ_FILL_HD void fill_relax(int L, const double* pts, const double* W, int i, int k, double* w_out, int* j_out) {
  double best = 0.0;
  int bj = -1;
  for (int j = i + 1; j < k; ++j) {
    const double w = (W[fill_at(L, i, j)] + W[fill_at(L, j, k)]) + fill_area(pts + 3 * i, pts + 3 * j, pts + 3 * k);
    if (bj < 0 || w < best) {
      best = w;
      bj = j;
    }
  }
  *w_out = best;
  *j_out = bj;
}

// Row q (0 <= q < L - 2) of the pre-order emission: emit(i, k) writes (i, S(i, k), k), then emit(i, j), then
// emit(j, k); the subtree (i, j) holds j - i - 1 rows, so the walk from the root knows where q lies.
PQ_FILL_HD void fill_row(int L, const uint8_t* S, int q, int* ri, int* rj, int* rk) {
  int i = 0, k = L - 1, p = 0;
  for (;;) {
    const int j = S[fill_at(L, i, k)];
    if (q == p) {
      *ri = i;
      *rj = j;
      *rk = k;
      return;
    }
    if (q < p + (j - i)) {
      k = j;
      p += 1;
    } else {
      p += j - i;
      i = j;
    }
  }
}

// The whole table on one thread (the check program; the kernels sweep a diagonal in parallel).
inline void fill_table(int L, const double* pts, double* W, uint8_t* S) {
  for (int i = 0; i + 1 < L; ++i) {
    W[fill_at(L, i, i + 1)] = 0.0;
    S[fill_at(L, i, i + 1)] = 0;
  }
  for (int d = 2; d < L; ++d)
    for (int i = 0; i + d < L; ++i) {
      double w;
      int j;
      fill_relax(L, pts, W, i, i + d, &w, &j);
      W[fill_at(L, i, i + d)] = w;
      S[fill_at(L, i, i + d)] = uint8_t(j);
    }
}

}  // namespace pyqsm
