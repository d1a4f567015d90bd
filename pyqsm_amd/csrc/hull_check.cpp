// hull_check.cpp — the int64 predicates of hull_exact.hpp against 128-bit evaluations (make hull_check).
// A stand-alone host program, built with AddressSanitizer and UndefinedBehaviorSanitizer: a signed
// overflow anywhere below the bound 6 * 2^60 < 2^63 would stop it. Four points with every coordinate at
// 0 or 2^20 (all 4096 patterns, so every sign pattern of the differences), the same around a negative
// origin, and random quadruples inside the extent.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "hull_exact.hpp"

using namespace pyqsm::hullx;
typedef __int128 i128;

static i128 orient_wide(const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d) {
  i128 u[3], v[3], w[3];
  for (int k = 0; k < 3; ++k) {
    u[k] = i128(b[k]) - a[k];
    v[k] = i128(c[k]) - a[k];
    w[k] = i128(d[k]) - a[k];
  }
  return (u[1] * v[2] - u[2] * v[1]) * w[0] + (u[2] * v[0] - u[0] * v[2]) * w[1] + (u[0] * v[1] - u[1] * v[0]) * w[2];
}

static long checks = 0;

static void fail(const char* what, const int32_t (*p)[3]) {
  std::fprintf(stderr, "hull_check: %s differs at", what);
  for (int i = 0; i < 4; ++i) std::fprintf(stderr, " (%d,%d,%d)", p[i][0], p[i][1], p[i][2]);
  std::fprintf(stderr, "\n");
  std::exit(1);
}

static void check(const int32_t (*p)[3]) {
  const i128 wide = orient_wide(p[0], p[1], p[2], p[3]);
  if (i128(orient3d(p[0], p[1], p[2], p[3])) != wide) fail("orient3d", p);
  const V3 e = diff(p[1], p[0]), f = diff(p[2], p[0]), g = diff(p[3], p[0]);
  const V3 n = cross(e, f);
  const i128 nx = i128(e.y) * f.z - i128(e.z) * f.y, ny = i128(e.z) * f.x - i128(e.x) * f.z,
             nz = i128(e.x) * f.y - i128(e.y) * f.x;
  if (i128(n.x) != nx || i128(n.y) != ny || i128(n.z) != nz) fail("cross", p);
  if (i128(dot(n, g)) != wide) fail("dot", p);
  if (i128(norm2(g)) != i128(g.x) * g.x + i128(g.y) * g.y + i128(g.z) * g.z) fail("norm2", p);
  if (!is_zero(n)) {
    // inside the plane of (p0, p1, p2): the orientation of (p0, p1, p2) seen from n is positive, its
    // mirror negative, and a point of the line collinear
    const int ax = dominant_axis(n);
    const i128 c = ax == 0 ? nx : (ax == 1 ? ny : nz);
    if (c == 0 || (c < 0 ? -c : c) < (nx < 0 ? -nx : nx) || (c < 0 ? -c : c) < (ny < 0 ? -ny : ny) ||
        (c < 0 ? -c : c) < (nz < 0 ? -nz : nz))
      fail("dominant_axis", p);
    const bool pos = comp(n, ax) > 0;
    if (orient2d_in_plane(p[0], p[1], p[2], ax, pos) != 1) fail("orient2d (left)", p);
    if (orient2d_in_plane(p[0], p[2], p[1], ax, pos) != -1) fail("orient2d (right)", p);
    if (orient2d_in_plane(p[0], p[1], p[1], ax, pos) != 0) fail("orient2d (collinear)", p);
  }
  ++checks;
}

int main() {
  const int32_t L = int32_t(kHullMaxExtent);
  for (int32_t origin : {0, -L, -(1 << 30), (1 << 30) - L}) {
    for (int bits = 0; bits < 4096; ++bits) {
      int32_t p[4][3];
      for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 3; ++k) p[i][k] = origin + (((bits >> (3 * i + k)) & 1) ? L : 0);
      check(p);
    }
  }
  std::mt19937_64 rng(12345);
  for (int it = 0; it < 2000000; ++it) {
    int32_t p[4][3];
    const int32_t origin = int32_t(rng() % (1u << 30)) - (1 << 29);
    const uint64_t span = (it & 1) ? uint64_t(L) + 1 : 1 + rng() % (uint64_t(L) + 1);
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < 3; ++k) p[i][k] = origin + int32_t(rng() % span);
    check(p);
  }
  std::printf("hull_check: %ld quadruples agree with 128-bit arithmetic\n", checks);
  return 0;
}
