// alpha3_exact.hpp — both rho-balls of one triple at once (alpha3.hip), built on the
// quantities of recon_exact.hpp: with u = p - a, D = n.u and N = |u|^2 n2 - w.u of the triple oriented
// by n = (b - a) x (c - a), p is strictly inside B+ (centre on the +n side) iff N < sqrt(H) D and strictly
// inside B- iff N < -sqrt(H) D. One N, one D and one H serve both; the fp64 filter takes a sign for
// either side only beyond the same margin as recon_filter, and the integers decide the rest.
// Host- and device-callable and free of any runtime call (alpha3_check.cpp runs it under the sanitizers).
// The bounds are recon_exact.hpp's: -D has the magnitude of D, so nothing grows.
#pragma once
#include "recon_exact.hpp"

namespace pyqsm {

struct Alpha3Sides {
  int plus, minus;  // kReconFilter* from alpha3_filter, kRecon* from alpha3_classify
};

// recon_filter for +D and -D: diff+ = Nf - rhs and diff- = Nf + rhs share Nf, rhs and the margin
// 2^-46 (M + |rhs|): the rounding of either difference is bounded as §19 bounds the one. |u|^2 <= 4 rho^2
// is the caller's. No fused multiply-add may be formed here (-ffp-contract=off).
PQ_HD PQ_FORCEINLINE Alpha3Sides alpha3_filter(const ReconFilterTri& f, double ux, double uy, double uz) {
  const double u2 = (ux * ux + uy * uy) + uz * uz;
  const double D = (f.n[0] * ux + f.n[1] * uy) + f.n[2] * uz;
  const double t0 = u2 * f.n2, t1 = f.w[0] * ux, t2 = f.w[1] * uy, t3 = f.w[2] * uz;
  const double Nf = ((t0 - t1) - t2) - t3;
  const double rhs = f.sH * D;
  const double tol = ((((fabs(t0) + fabs(t1)) + fabs(t2)) + fabs(t3)) + fabs(rhs)) * 0x1p-46;
  const double dp = Nf - rhs, dm = Nf + rhs;
  Alpha3Sides s;
  s.plus = dp > tol ? kReconFilterOutside : dp < -tol ? kReconFilterInside : kReconFilterUndecided;
  s.minus = dm > tol ? kReconFilterOutside : dm < -tol ? kReconFilterInside : kReconFilterUndecided;
  return s;
}

// N against sqrt(H) d for a d of the sign sd != 0, given cmp = the order of N^2 against d^2 H
PQ_HD inline int alpha3_side(int sn, int sd, int cmp) {
  if (sd > 0 && sn < 0) return kReconInside;
  if (sd < 0 && sn > 0) return kReconOutside;
  if (cmp == 0) return kReconTieOffPlane;
  if (sd > 0) return cmp < 0 ? kReconInside : kReconOutside;
  return cmp > 0 ? kReconInside : kReconOutside;
}

// recon_classify for both balls from one evaluation: .plus equals recon_classify(t, u), .minus equals
// recon_classify of the triple (a, c, b) at the same point (its n, w.u's complement and D change sign
// together, its N and H do not).
PQ_HD inline Alpha3Sides alpha3_classify(const ReconTri& t, const int64_t u[3]) {
  const int64_t D = t.n[0] * u[0] + t.n[1] * u[1] + t.n[2] * u[2];
  const int64_t u2 = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
  const i128 N = i128(u2) * t.n2 - (i128(t.w[0]) * u[0] + i128(t.w[1]) * u[1] + i128(t.w[2]) * u[2]);
  Alpha3Sides s;
  if (D == 0) {
    s.plus = s.minus = N < 0 ? kReconInside : N == 0 ? kReconTieCoplanar : kReconOutside;
    return s;
  }
  const u128 absN = N < 0 ? u128(-N) : u128(N);
  const u128 absD = D < 0 ? u128(-i128(D)) : u128(D);
  const int cmp = cmp_u256(mul_u128(absN, absN), mul_u128(absD * absD, t.H));
  const int sn = N < 0 ? -1 : N > 0 ? 1 : 0, sd = D > 0 ? 1 : -1;
  s.plus = alpha3_side(sn, sd, cmp);
  s.minus = alpha3_side(sn, -sd, cmp);
  return s;
}

enum { kAlpha3None = 0, kAlpha3Regular = 1, kAlpha3Singular = 2 };

// The kind of a triple from what its sweep found: a ball is empty when nothing was strictly inside it;
// `unresolved` = an off-plane tie on an empty ball, `tie_drop` = a coplanar tie of a lower index than a or
// strictly beyond the edge opposite a (the fan rule of §19, which an off-plane tie overrides as there).
// *flip: the empty ball of a regular triple is B-, so the row is (a, c, b).
PQ_HD inline int alpha3_kind(bool empty_plus, bool empty_minus, bool unresolved, bool tie_drop, bool h_zero,
                             bool* flip) {
  *flip = false;
  if (!empty_plus && !empty_minus) return kAlpha3None;
  if (tie_drop && !unresolved) return kAlpha3None;
  if (h_zero) return kAlpha3None;  // one ball for both sides: never regular, and no sheet with two sides
  if (empty_plus && empty_minus) return kAlpha3Singular;
  *flip = empty_minus;
  return kAlpha3Regular;
}

}  // namespace pyqsm
