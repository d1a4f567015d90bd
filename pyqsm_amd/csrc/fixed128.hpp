// fixed128.hpp — exact fixed-point moments, shared by the geometric features (features.hip) and the
// least-squares refit of a segmented plane (ransac.hip). Every term o_a (and the fp64 product
// o_a * o_b) of an offset is scaled by a power of two that maps the largest possible offset to at
// most 2^61, rounded to an integer and summed in 128 bits. The sum is then exact: it does not depend
// on the order of the additions, and it needs no atomics (lane partials fold by a butterfly).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace pyqsm {

// A signed 128-bit integer as (low word, high word).
struct I128 {
  unsigned long long lo;
  long long hi;
};

// a += x, x an integral double with |x| <= 2^62
__device__ __forceinline__ void acc128(I128& a, double x) {
  const long long v = (long long)x;
  const unsigned long long lo = a.lo + (unsigned long long)v;
  a.hi += (v < 0 ? -1LL : 0LL) + (lo < a.lo ? 1LL : 0LL);
  a.lo = lo;
}

// a += b
__device__ __forceinline__ void add128(I128& a, const I128& b) {
  const unsigned long long lo = a.lo + b.lo;
  a.hi = a.hi + b.hi + (lo < a.lo ? 1LL : 0LL);
  a.lo = lo;
}

// a += the value lane ^ off holds
__device__ __forceinline__ void fold128(I128& a, int off) {
  const unsigned long long blo = __shfl_xor(a.lo, off, 64);
  const long long bhi = __shfl_xor(a.hi, off, 64);
  const unsigned long long lo = a.lo + blo;
  a.hi = a.hi + bhi + (lo < a.lo ? 1LL : 0LL);
  a.lo = lo;
}

// the magnitude as hi * 2^64 + lo, the sign applied after: small negative sums stay exact
__device__ __forceinline__ double to_double(I128 a) {
  const bool neg = a.hi < 0;
  if (neg) {
    a.lo = ~a.lo + 1ull;
    a.hi = ~a.hi + (a.lo == 0ull ? 1LL : 0LL);
  }
  const double v = double((unsigned long long)a.hi) * 18446744073709551616.0 + double(a.lo);
  return neg ? -v : v;
}

// Powers of two per axis: s1[a] maps the largest offset along a to at most 2^61, s2 the products
// of the pairs (00, 01, 02, 11, 12, 22); u1, u2 their inverses.
struct FeatScale {
  double s1[3], s2[6], u1[3], u2[6];
};

// The scales for offsets bounded by bound[a] along each axis (zero extents: any scale).
__host__ __device__ inline FeatScale feat_scale(const double bound[3]) {
  FeatScale sc;
  int sh[3];
  for (int a = 0; a < 3; ++a) {
    const double b = fmax(bound[a], ldexp(1.0, -400));
    int e = 0;
    frexp(b, &e);  // b < 2^e
    sh[a] = 61 - e;
    sc.s1[a] = ldexp(1.0, sh[a]);
    sc.u1[a] = ldexp(1.0, -sh[a]);
  }
  const int A[6] = {0, 0, 0, 1, 1, 2}, B[6] = {0, 1, 2, 1, 2, 2};
  for (int e = 0; e < 6; ++e) {
    sc.s2[e] = ldexp(1.0, sh[A[e]] + sh[B[e]] - 61);
    sc.u2[e] = ldexp(1.0, 61 - sh[A[e]] - sh[B[e]]);
  }
  return sc;
}

// M[0..3) += the offset's first moments, M[3..9) += its second moments (00, 01, 02, 11, 12, 22)
__device__ __forceinline__ void add_moments(I128* M, const FeatScale& sc, double ox, double oy, double oz) {
  acc128(M[0], rint(ox * sc.s1[0]));
  acc128(M[1], rint(oy * sc.s1[1]));
  acc128(M[2], rint(oz * sc.s1[2]));
  acc128(M[3], rint((ox * ox) * sc.s2[0]));
  acc128(M[4], rint((ox * oy) * sc.s2[1]));
  acc128(M[5], rint((ox * oz) * sc.s2[2]));
  acc128(M[6], rint((oy * oy) * sc.s2[3]));
  acc128(M[7], rint((oy * oz) * sc.s2[4]));
  acc128(M[8], rint((oz * oz) * sc.s2[5]));
}

}  // namespace pyqsm
