// recon_exact.hpp — the integer side of the ball-pivoting predicate (recon.hip): the
// exact quantities of one oriented candidate triangle and the exact position of a point against its
// rho-ball, and the fp64 filter the kernel runs in front of it (recon_filter_setup / recon_filter).
// Host- and device-callable and free of any runtime call, so that a stand-alone host program
// (recon_check.cpp) can run it under the sanitizers and hold the filter against the integers.
//
// Bounds (L = 2 rho <= 2^12, every |e|, |u| <= L): |n_i| <= L^2 = 2^24, n2 <= L^4 = 2^48,
// |w_i| <= 2 L^5 = 2^61 (int64), E, H <= L^6 = 2^72 and |N| <= 3 L^6 < 2^74 (128 bits),
// N^2 < 2^148 and D^2 H <= 2^144 (256 bits).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PQ_HD __host__ __device__
#define PQ_FORCEINLINE inline __attribute__((always_inline))  // what __forceinline__ stands for
#else
#define PQ_HD
#define PQ_FORCEINLINE inline
#endif

namespace pyqsm {

typedef unsigned __int128 u128;
typedef __int128 i128;

struct U256 {
  uint64_t w[4];  // little endian
};

PQ_HD inline U256 mul_u128(u128 a, u128 b) {
  const uint64_t a0 = uint64_t(a), a1 = uint64_t(a >> 64), b0 = uint64_t(b), b1 = uint64_t(b >> 64);
  const u128 p00 = u128(a0) * b0, p01 = u128(a0) * b1, p10 = u128(a1) * b0, p11 = u128(a1) * b1;
  U256 r;
  r.w[0] = uint64_t(p00);
  const u128 mid = (p00 >> 64) + uint64_t(p01) + uint64_t(p10);  // three terms below 2^64 each
  r.w[1] = uint64_t(mid);
  const u128 hi = (mid >> 64) + (p01 >> 64) + (p10 >> 64) + uint64_t(p11);
  r.w[2] = uint64_t(hi);
  r.w[3] = uint64_t((hi >> 64) + (p11 >> 64));
  return r;
}

PQ_HD inline int cmp_u256(const U256& a, const U256& b) {
  for (int k = 3; k >= 0; --k)
    if (a.w[k] != b.w[k]) return a.w[k] < b.w[k] ? -1 : 1;
  return 0;
}

// An oriented candidate (a, b, c), everything relative to a.
struct ReconTri {
  int64_t e1[3], e2[3], n[3], w[3];
  int64_t n2;
  u128 H;  // 4 rho^2 n2 - E >= 0
};

// false when (a, b, c) is no candidate: an edge longer than 2 rho, a degenerate triangle, or a
// circumradius above rho (H < 0). four_r2 = 4 rho^2 <= 2^24; the edges must be checked against it
// BEFORE any product is formed, which is what keeps every product inside its type.
PQ_HD inline bool recon_setup(const int64_t a[3], const int64_t b[3], const int64_t c[3], uint64_t four_r2,
                              ReconTri* t) {
  int64_t l1 = 0, l2 = 0, l3 = 0;
  for (int k = 0; k < 3; ++k) {
    t->e1[k] = b[k] - a[k];
    t->e2[k] = c[k] - a[k];
    const int64_t cap = int64_t(1) << 13;  // anything beyond is out of reach, and its square may not fit
    if (t->e1[k] > cap || t->e1[k] < -cap || t->e2[k] > cap || t->e2[k] < -cap) return false;
    const int64_t e3 = t->e2[k] - t->e1[k];
    l1 += t->e1[k] * t->e1[k];
    l2 += t->e2[k] * t->e2[k];
    l3 += e3 * e3;
  }
  if (uint64_t(l1) > four_r2 || uint64_t(l2) > four_r2 || uint64_t(l3) > four_r2) return false;
  const int64_t* e1 = t->e1;
  const int64_t* e2 = t->e2;
  int64_t* n = t->n;
  n[0] = e1[1] * e2[2] - e1[2] * e2[1];
  n[1] = e1[2] * e2[0] - e1[0] * e2[2];
  n[2] = e1[0] * e2[1] - e1[1] * e2[0];
  t->n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  if (t->n2 == 0) return false;
  const u128 E = u128(uint64_t(l1)) * uint64_t(l2) * uint64_t(l3);
  const u128 R = u128(four_r2) * uint64_t(t->n2);
  if (R < E) return false;
  t->H = R - E;
  // w = |e1|^2 (e2 x n) + |e2|^2 (n x e1)
  t->w[0] = l1 * (e2[1] * n[2] - e2[2] * n[1]) + l2 * (n[1] * e1[2] - n[2] * e1[1]);
  t->w[1] = l1 * (e2[2] * n[0] - e2[0] * n[2]) + l2 * (n[2] * e1[0] - n[0] * e1[2]);
  t->w[2] = l1 * (e2[0] * n[1] - e2[1] * n[0]) + l2 * (n[0] * e1[1] - n[1] * e1[0]);
  return true;
}

enum { kReconOutside = 0, kReconInside = 1, kReconTieCoplanar = 2, kReconTieOffPlane = 3 };

// Where p = a + u lies against the rho-ball through a, b, c whose centre is on the +n side:
// strictly inside iff N < sqrt(H) D, on it iff N == sqrt(H) D. |u|^2 <= 4 rho^2 is the caller's.
PQ_HD inline int recon_classify(const ReconTri& t, const int64_t u[3]) {
  const int64_t D = t.n[0] * u[0] + t.n[1] * u[1] + t.n[2] * u[2];
  const int64_t u2 = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
  const i128 N = i128(u2) * t.n2 - (i128(t.w[0]) * u[0] + i128(t.w[1]) * u[1] + i128(t.w[2]) * u[2]);
  if (D == 0) return N < 0 ? kReconInside : N == 0 ? kReconTieCoplanar : kReconOutside;
  if (D > 0 && N < 0) return kReconInside;
  if (D < 0 && N > 0) return kReconOutside;
  const u128 absN = N < 0 ? u128(-N) : u128(N);
  const int cmp = cmp_u256(mul_u128(absN, absN), mul_u128(u128(D) * u128(D), t.H));  // D^2: the sign cancels
  if (cmp == 0) return kReconTieOffPlane;
  if (D > 0) return cmp < 0 ? kReconInside : kReconOutside;
  return cmp > 0 ? kReconInside : kReconOutside;
}

// ---- the fp64 filter in front of recon_classify (recon.hip, "The filter") ----------
// What one candidate keeps in fp64: n, n2 and every |D| are exact, each w_i is rounded once, H is put
// together from its two 64-bit halves before the root.
struct ReconFilterTri {
  double n[3], w[3];
  double n2, sH;
};

PQ_HD inline ReconFilterTri recon_filter_setup(const ReconTri& t) {
  ReconFilterTri f;
  f.n[0] = double(t.n[0]);
  f.n[1] = double(t.n[1]);
  f.n[2] = double(t.n[2]);
  f.w[0] = double(t.w[0]);
  f.w[1] = double(t.w[1]);
  f.w[2] = double(t.w[2]);
  f.n2 = double(t.n2);
  f.sH = sqrt(double(uint64_t(t.H >> 64)) * 0x1p64 + double(uint64_t(t.H)));
  return f;
}

enum { kReconFilterOutside = 0, kReconFilterInside = 1, kReconFilterUndecided = 2 };

// The sign of N - sqrt(H) D for u = p - a where fp64 is sure of it: |diff| > 2^-46 (M + |rhs|), eight
// times the rounding of its terms. Everything else, every exact tie among it, is recon_classify's.
// |u|^2 <= 4 rho^2 is the caller's. No fused multiply-add may be formed here (-ffp-contract=off).
PQ_HD PQ_FORCEINLINE int recon_filter(const ReconFilterTri& f, double ux, double uy, double uz) {
  const double u2 = (ux * ux + uy * uy) + uz * uz;
  const double D = (f.n[0] * ux + f.n[1] * uy) + f.n[2] * uz;
  const double t0 = u2 * f.n2, t1 = f.w[0] * ux, t2 = f.w[1] * uy, t3 = f.w[2] * uz;
  const double Nf = ((t0 - t1) - t2) - t3;
  const double rhs = f.sH * D;
  const double diff = Nf - rhs;
  const double tol = ((((fabs(t0) + fabs(t1)) + fabs(t2)) + fabs(t3)) + fabs(rhs)) * 0x1p-46;
  if (diff > tol) return kReconFilterOutside;
  if (diff < -tol) return kReconFilterInside;
  return kReconFilterUndecided;
}

// ((c - b) x (p - b)) . n < 0: p lies strictly beyond the edge b -> c of the oriented triangle, in its plane
PQ_HD inline bool recon_beyond_bc(const ReconTri& t, const int64_t u[3]) {
  int64_t f[3], g[3];
  for (int k = 0; k < 3; ++k) {
    f[k] = t.e2[k] - t.e1[k];
    g[k] = u[k] - t.e1[k];
  }
  const int64_t x = f[1] * g[2] - f[2] * g[1], y = f[2] * g[0] - f[0] * g[2], z = f[0] * g[1] - f[1] * g[0];
  return x * t.n[0] + y * t.n[1] + z * t.n[2] < 0;
}

}  // namespace pyqsm
