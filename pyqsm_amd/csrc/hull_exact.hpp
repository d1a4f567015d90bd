// hull_exact.hpp — the integer predicates of the exact convex hull (convex_hull.hip), shared by host and
// device and held against 128-bit evaluations by hull_check.cpp.
//
// Lattice points of one segment span at most kHullMaxExtent = 2^20 units on every axis, so every
// difference d of two of them has |d| <= 2^20 per component. Then
//   a component of d1 x d2 is a difference of two products below 2^40:  |.| <= 2^41,
//   (d1 x d2) . d3 is a sum of three products below 2^61:               |.| <= 3 * 2^61 = 6 * 2^60 < 2^63,
//   a squared length is a sum of three squares below 2^40:              |.| <= 3 * 2^40.
// Nothing here overflows int64 and nothing is floating point.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PQ_HX __host__ __device__ inline __attribute__((always_inline))
#else
#define PQ_HX inline
#endif

namespace pyqsm {
namespace hullx {

static constexpr int64_t kHullMaxExtent = int64_t(1) << 20;

struct V3 {
  int64_t x, y, z;
};

PQ_HX V3 diff(const int32_t* p, const int32_t* q) {  // p - q
  return V3{int64_t(p[0]) - q[0], int64_t(p[1]) - q[1], int64_t(p[2]) - q[2]};
}
PQ_HX V3 cross(const V3& a, const V3& b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
PQ_HX int64_t dot(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PQ_HX bool is_zero(const V3& a) { return a.x == 0 && a.y == 0 && a.z == 0; }
PQ_HX int64_t norm2(const V3& a) { return dot(a, a); }

// ((b - a) x (c - a)) . (d - a): positive when d lies on the side the normal of (a, b, c) points to
PQ_HX int64_t orient3d(const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d) {
  return dot(cross(diff(b, a), diff(c, a)), diff(d, a));
}

// the axis on which |n| is largest (the lowest axis on ties): dropping it projects the plane of normal n
// onto a coordinate plane without collapsing it
PQ_HX int dominant_axis(const V3& n) {
  const int64_t ax = n.x < 0 ? -n.x : n.x, ay = n.y < 0 ? -n.y : n.y, az = n.z < 0 ? -n.z : n.z;
  return ax >= ay && ax >= az ? 0 : (ay >= az ? 1 : 2);
}
PQ_HX int64_t comp(const V3& a, int axis) { return axis == 0 ? a.x : (axis == 1 ? a.y : a.z); }

// The 2-D orientation of (y, z, q), three points of a plane of normal n, seen from the side n points to:
// the sign of ((z - y) x (q - y)) . n. The cross product is parallel to n, so the sign is that of its
// component on n's dominant axis times the sign of n there: the projection along that axis.
// > 0: q left of y -> z (counter-clockwise), < 0: right, 0: collinear.
PQ_HX int orient2d_in_plane(const int32_t* y, const int32_t* z, const int32_t* q, int axis, bool n_positive) {
  const int64_t m = comp(cross(diff(z, y), diff(q, y)), axis);
  if (m == 0) return 0;
  return ((m > 0) == n_positive) ? 1 : -1;
}

}  // namespace hullx
}  // namespace pyqsm
