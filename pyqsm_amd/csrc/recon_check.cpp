// recon_check.cpp — the integer side of the ball-pivoting predicate (recon_exact.hpp) on the host, as a
// stand-alone program for AddressSanitizer and UndefinedBehaviorSanitizer (`make recon_check`):
//   mul_u128 / cmp_u256 against a schoolbook product in 32-bit limbs, operands at the bounds of §19;
//   recon_setup / recon_classify at the largest admitted radius (rho^2 = 2^22): the vertices of a
//   candidate are ties in its plane, points above and below it fall inside and outside its ball, the
//   corners of a cube are ties on and off the plane of one of its faces, and signed overflow anywhere
//   would stop the run;
//   recon_filter, the fp64 filter the kernel runs first, against recon_classify: a sign it takes is the
//   integers' side, on a million random configurations at the bound, on lattice points of two spheres
//   with rho^2 = r^2 just below 2^22 (half of all tests exact ties), on coplanar ties and H == 0 at the
//   bound, and one lattice unit around every tie. Built with -ffp-contract=off, as the library is.
#include <cstdio>
#include <cstdlib>

#include "recon_exact.hpp"

using namespace pyqsm;

static int failures = 0;
#define CHECK(cond)                                           \
  do {                                                        \
    if (!(cond)) {                                            \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                             \
    }                                                         \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

static U256 schoolbook(u128 a, u128 b) {
  uint32_t x[4], y[4];
  uint64_t acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) {
    x[k] = uint32_t(a >> (32 * k));
    y[k] = uint32_t(b >> (32 * k));
  }
  uint32_t limb[8];
  for (int k = 0; k < 8; ++k) {
    // column k: at most four products below 2^64 each, summed in two halves to stay inside 64 bits
    uint64_t lo = acc[k], hi = 0;
    for (int i = 0; i < 4; ++i) {
      const int j = k - i;
      if (j < 0 || j > 3) continue;
      const uint64_t p = uint64_t(x[i]) * y[j];
      lo += p & 0xFFFFFFFFull;
      hi += p >> 32;
    }
    limb[k] = uint32_t(lo);
    acc[k + 1] += (lo >> 32) + hi;
  }
  U256 r;
  for (int k = 0; k < 4; ++k) r.w[k] = uint64_t(limb[2 * k]) | (uint64_t(limb[2 * k + 1]) << 32);
  return r;
}

// ---- the fp64 filter against the integers. The property, on every input: whenever recon_filter takes
// a sign, recon_classify is on that side; hence every exact tie comes back undecided.
struct Tally {
  long inside = 0, outside = 0, undecided = 0, ties = 0, ties_decided = 0, wrong = 0;
  long tests() const { return inside + outside + undecided; }
};
static Tally tally;

// what the integers say of u, or -1 when |u|^2 > 4 rho^2 (the kernel skips such a point before the filter)
static int check_point(const ReconTri& t, const ReconFilterTri& f, const int64_t u[3], uint64_t four_r2) {
  if (uint64_t(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) > four_r2) return -1;
  const int side = recon_filter(f, double(u[0]), double(u[1]), double(u[2]));
  const int where = recon_classify(t, u);
  const bool tie = where == kReconTieCoplanar || where == kReconTieOffPlane;
  tally.inside += side == kReconFilterInside;
  tally.outside += side == kReconFilterOutside;
  tally.undecided += side == kReconFilterUndecided;
  tally.ties += tie;
  tally.ties_decided += tie && side != kReconFilterUndecided;
  const bool sound = side == kReconFilterUndecided || (side == kReconFilterInside && where == kReconInside) ||
                     (side == kReconFilterOutside && where == kReconOutside);
  if (!sound && tally.wrong++ < 10)
    std::printf("FAILED filter: side %d against the integers' %d, u = (%lld, %lld, %lld), n2 = %lld\n", side, where,
                (long long)u[0], (long long)u[1], (long long)u[2], (long long)t.n2);
  return where;
}

// the point, and where it ties its six neighbours one lattice unit away on one axis
static int check_point_and_around(const ReconTri& t, const ReconFilterTri& f, const int64_t u[3], uint64_t four_r2) {
  const int where = check_point(t, f, u, four_r2);
  if (where == kReconTieCoplanar || where == kReconTieOffPlane)
    for (int d = 0; d < 3; ++d)
      for (int s = -1; s <= 1; s += 2) {
        int64_t v[3] = {u[0], u[1], u[2]};
        v[d] += s;
        check_point(t, f, v, four_r2);
      }
  return where;
}

// every triple i < j < k of pts in both orientations against every other point of pts (and around the ties)
static void check_all_triples(const int64_t (*pts)[3], int n, uint64_t four_r2) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      for (int k = j + 1; k < n; ++k)
        for (int flip = 0; flip < 2; ++flip) {
          ReconTri t;
          if (!recon_setup(pts[i], pts[flip ? k : j], pts[flip ? j : k], four_r2, &t)) continue;
          const ReconFilterTri f = recon_filter_setup(t);
          for (int p = 0; p < n; ++p) {
            if (p == i || p == j || p == k) continue;
            const int64_t u[3] = {pts[p][0] - pts[i][0], pts[p][1] - pts[i][1], pts[p][2] - pts[i][2]};
            check_point_and_around(t, f, u, four_r2);
          }
        }
}

// 24 of the integer points of the sphere x^2 + y^2 + z^2 = r2, rho^2 = r2: one orientation of every triple
// rests on the sphere itself, where every other point ties off its plane (or in it)
static void check_lattice_sphere(int64_t r2, long expected_points) {
  static int64_t all[16384][3];
  long count = 0;
  int64_t r = 0;
  while ((r + 1) * (r + 1) <= r2) ++r;
  for (int64_t x = -r; x <= r; ++x)
    for (int64_t y = -r; y <= r; ++y) {
      const int64_t rest = r2 - x * x - y * y;
      if (rest < 0) continue;
      int64_t z = int64_t(std::sqrt(double(rest)));
      while (z * z > rest) --z;
      while ((z + 1) * (z + 1) <= rest) ++z;
      if (z * z != rest) continue;
      for (int s = 0; s < (z ? 2 : 1) && count < 16384; ++s, ++count) {
        all[count][0] = x;
        all[count][1] = y;
        all[count][2] = s ? -z : z;
      }
    }
  CHECK(count == expected_points);
  if (count < 24) return;
  int64_t pts[24][3];
  for (int k = 0; k < 24; ++k) {  // a fixed choice without repeats: the chosen point swaps with the last
    const long at = long(rng() % uint64_t(count - k));
    for (int d = 0; d < 3; ++d) {
      pts[k][d] = all[at][d];
      all[at][d] = all[count - 1 - k][d];
    }
  }
  const Tally before = tally;
  const uint64_t four_r2 = 4 * uint64_t(r2);
  long direct = 0, direct_undecided = 0;  // the 2 * C(24, 3) * 21 tests themselves, without the neighbours
  for (int i = 0; i < 24; ++i)
    for (int j = i + 1; j < 24; ++j)
      for (int k = j + 1; k < 24; ++k)
        for (int flip = 0; flip < 2; ++flip) {
          ReconTri t;
          const bool cand = recon_setup(pts[i], pts[flip ? k : j], pts[flip ? j : k], four_r2, &t);
          CHECK(cand);  // three points of a sphere of radius rho
          if (!cand) continue;
          const ReconFilterTri f = recon_filter_setup(t);
          for (int p = 0; p < 24; ++p) {
            if (p == i || p == j || p == k) continue;
            const int64_t u[3] = {pts[p][0] - pts[i][0], pts[p][1] - pts[i][1], pts[p][2] - pts[i][2]};
            const long und = tally.undecided;
            check_point(t, f, u, four_r2);
            ++direct;
            direct_undecided += tally.undecided - und;
          }
        }
  CHECK(direct == 2 * 2024 * 21);
  CHECK(3 * direct_undecided >= direct);
  CHECK(tally.ties - before.ties >= direct / 2);  // the orientation that rests on the sphere
  // once more with the neighbours of every tie
  static int64_t chosen[24][3];
  for (int k = 0; k < 24; ++k)
    for (int d = 0; d < 3; ++d) chosen[k][d] = pts[k][d];
  check_all_triples(chosen, 24, four_r2);
}

int main() {
  // ---- wide products
  for (int it = 0; it < 20000; ++it) {
    u128 a = (u128(rng()) << 64) | rng(), b = (u128(rng()) << 64) | rng();
    a >>= rng() % 128;
    b >>= rng() % 128;
    CHECK(cmp_u256(mul_u128(a, b), schoolbook(a, b)) == 0);
  }
  const u128 ones = ~u128(0);
  CHECK(cmp_u256(mul_u128(ones, ones), schoolbook(ones, ones)) == 0);
  CHECK(cmp_u256(mul_u128(0, ones), schoolbook(0, ones)) == 0);
  {
    const U256 lo = mul_u128(u128(1) << 74, u128(1) << 73), hi = mul_u128(u128(1) << 74, u128(1) << 74);
    CHECK(cmp_u256(lo, hi) < 0 && cmp_u256(hi, lo) > 0 && cmp_u256(hi, hi) == 0);
  }

  // ---- the predicate near the bound: rho^2 = 2^22, a triangle with edges of 3000 in the plane z = 5
  // (circumradius 1732, the ball's centre 1093 above the plane)
  const uint64_t four_r2 = 4ull << 22;
  const int64_t a[3] = {1000000, -2000000, 5}, b[3] = {a[0] + 3000, a[1], a[2]}, c[3] = {a[0] + 1500, a[1] + 2598, a[2]};
  ReconTri t;
  CHECK(recon_setup(a, b, c, four_r2, &t));
  CHECK(t.n[0] == 0 && t.n[1] == 0 && t.n[2] == 3000 * 2598);
  const int64_t zero[3] = {0, 0, 0};
  CHECK(recon_classify(t, zero) == kReconTieCoplanar);
  CHECK(recon_classify(t, t.e1) == kReconTieCoplanar);
  CHECK(recon_classify(t, t.e2) == kReconTieCoplanar);
  const int64_t centroid[3] = {1500, 866, 0}, above[3] = {1500, 866, 700}, below[3] = {1500, 866, -1000};
  CHECK(recon_classify(t, centroid) == kReconInside);
  CHECK(recon_classify(t, above) == kReconInside);
  CHECK(recon_classify(t, below) == kReconOutside);   // 2093 from the centre
  const int64_t far_in_plane[3] = {-4000, 0, 0};
  CHECK(recon_classify(t, far_in_plane) == kReconOutside);
  CHECK(!recon_beyond_bc(t, zero) && !recon_beyond_bc(t, centroid));
  const int64_t beyond[3] = {3000, 2598, 0};
  CHECK(recon_beyond_bc(t, beyond));
  {
    // the largest equilateral candidate: edges of 3546, circumradius 2047.3 <= rho = 2048
    const int64_t b2[3] = {a[0] + 3546, a[1], a[2]}, c2[3] = {a[0] + 1773, a[1] + 3071, a[2]};
    ReconTri big;
    CHECK(recon_setup(a, b2, c2, four_r2, &big));
    CHECK(recon_classify(big, big.e1) == kReconTieCoplanar && recon_classify(big, big.e2) == kReconTieCoplanar);
    const int64_t b3[3] = {a[0] + 3548, a[1], a[2]}, c3[3] = {a[0] + 1774, a[1] + 3073, a[2]};
    CHECK(!recon_setup(a, b3, c3, four_r2, &big));     // circumradius 2048.6
  }
  // no candidate: an edge out of reach (also far beyond what a square could hold), a degenerate triple,
  // a circumradius above rho
  const int64_t far[3] = {a[0] + (int64_t(1) << 33), a[1], a[2]}, mid[3] = {a[0] + 1500, a[1], a[2]};
  CHECK(!recon_setup(a, far, c, four_r2, &t));
  CHECK(!recon_setup(a, b, mid, four_r2, &t));
  const int64_t flat[3] = {a[0] + 1500, a[1] + 1, a[2]};
  CHECK(!recon_setup(a, b, flat, four_r2, &t));

  // ---- an exactly cospherical configuration: the unit-cube corners scaled by 1000, rho^2 = 3 * 500^2.
  // Four corners of one face are a coplanar tie for each other; the opposite face is an off-plane tie.
  {
    const uint64_t r2 = 3 * 500 * 500;
    const int64_t p0[3] = {0, 0, 0}, p1[3] = {1000, 0, 0}, p2[3] = {0, 1000, 0};
    ReconTri q;
    CHECK(recon_setup(p0, p1, p2, 4 * r2, &q));
    const int64_t same_face[3] = {1000, 1000, 0}, up[3] = {0, 0, 1000}, up2[3] = {1000, 1000, 1000};
    const int64_t in[3] = {500, 500, 500}, down[3] = {0, 0, -1};
    CHECK(recon_classify(q, same_face) == kReconTieCoplanar);
    CHECK(recon_classify(q, up) == kReconTieOffPlane);
    CHECK(recon_classify(q, up2) == kReconTieOffPlane);
    CHECK(recon_classify(q, in) == kReconInside);
    CHECK(recon_classify(q, down) == kReconOutside);
    CHECK(recon_beyond_bc(q, same_face));
  }

  // ---- random triples at the bound: they simply have to run clean under the sanitizers
  int inside = 0, outside = 0;
  for (int it = 0; it < 20000; ++it) {
    int64_t v[4][3];
    for (int k = 0; k < 4; ++k)
      for (int d = 0; d < 3; ++d) v[k][d] = int64_t(rng() % 4730) - 2365;  // |difference| <= 4729 per axis
    ReconTri q;
    if (!recon_setup(v[0], v[1], v[2], four_r2, &q)) continue;
    const int64_t u[3] = {v[3][0] - v[0][0], v[3][1] - v[0][1], v[3][2] - v[0][2]};
    if (uint64_t(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) > four_r2) continue;
    const int w = recon_classify(q, u);
    inside += w == kReconInside;
    outside += w == kReconOutside;
  }
  CHECK(inside > 0 && outside > 0);

  // ---- the filter, random at the bound: the same coordinates, each candidate in both orientations
  // against eight points, until a million configurations have been through filter and integers
  {
    long configs = 0;
    for (long it = 0; it < 40000000 && configs < 1000000; ++it) {
      int64_t v[3][3];
      for (int k = 0; k < 3; ++k)
        for (int d = 0; d < 3; ++d) v[k][d] = int64_t(rng() % 4730) - 2365;
      for (int flip = 0; flip < 2; ++flip) {
        ReconTri q;
        if (!recon_setup(v[0], v[flip ? 2 : 1], v[flip ? 1 : 2], four_r2, &q)) break;
        const ReconFilterTri f = recon_filter_setup(q);
        for (int p = 0; p < 8; ++p) {
          int64_t u[3];
          for (int d = 0; d < 3; ++d) u[d] = int64_t(rng() % 4730) - 2365 - v[0][d];
          configs += check_point(q, f, u, four_r2) >= 0;
        }
      }
    }
    CHECK(configs >= 1000000);
    CHECK(tally.inside > 0 && tally.outside > 0);
  }

  // ---- the filter on exactly cospherical families at the bound
  check_lattice_sphere(4191372, 6368);   // 3 * 1182^2: the circumsphere of a cube of edge 2364
  check_lattice_sphere(4194301, 14376);  // three below 2^22

  // ---- the filter on coplanar ties at the bound, and around them
  {
    // the corners of that cube, rho its circumradius: the other corners of a face tie in its plane,
    // the opposite face off it, and a plane through the centre has H == 0
    int64_t cube[8][3];
    for (int k = 0; k < 8; ++k)
      for (int d = 0; d < 3; ++d) cube[k][d] = ((k >> d) & 1) * 2364 + (d == 0 ? -7 : d == 1 ? 1000003 : -2000001);
    const long ties = tally.ties;
    check_all_triples(cube, 8, 4ull * 4191372);
    CHECK(tally.ties > ties);
    ReconTri q;
    CHECK(recon_setup(cube[0], cube[1], cube[6], 4ull * 4191372, &q) && q.H == 0);  // an edge and the edge across
    // the largest equilateral candidate and its own vertices
    const int64_t b2[3] = {a[0] + 3546, a[1], a[2]}, c2[3] = {a[0] + 1773, a[1] + 3071, a[2]};
    ReconTri big;
    CHECK(recon_setup(a, b2, c2, four_r2, &big));
    const ReconFilterTri fb = recon_filter_setup(big);
    CHECK(check_point_and_around(big, fb, zero, four_r2) == kReconTieCoplanar);
    CHECK(check_point_and_around(big, fb, big.e1, four_r2) == kReconTieCoplanar);
    CHECK(check_point_and_around(big, fb, big.e2, four_r2) == kReconTieCoplanar);
    // a right triangle whose hypotenuse is exactly 2 rho (legs 2454 and 3272, rho = 2045): H == 0, one ball
    // for both orientations, its centre in the plane; the fourth corner of the rectangle ties in the
    // plane, the two poles of the ball off it
    const uint64_t four_h = 4ull * 2045 * 2045;
    const int64_t rb[3] = {a[0] + 2454, a[1], a[2]}, rc[3] = {a[0], a[1] + 3272, a[2]};
    for (int flip = 0; flip < 2; ++flip) {
      ReconTri rt;
      CHECK(recon_setup(a, flip ? rc : rb, flip ? rb : rc, four_h, &rt));
      CHECK(rt.H == 0);
      const ReconFilterTri fr = recon_filter_setup(rt);
      CHECK(fr.sH == 0.0);
      const int64_t fourth[3] = {2454, 3272, 0}, north[3] = {1227, 1636, 2045}, south[3] = {1227, 1636, -2045};
      const int64_t centre[3] = {1227, 1636, 0};
      CHECK(check_point_and_around(rt, fr, zero, four_h) == kReconTieCoplanar);
      CHECK(check_point_and_around(rt, fr, rt.e1, four_h) == kReconTieCoplanar);
      CHECK(check_point_and_around(rt, fr, rt.e2, four_h) == kReconTieCoplanar);
      CHECK(check_point_and_around(rt, fr, fourth, four_h) == kReconTieCoplanar);
      CHECK(check_point_and_around(rt, fr, north, four_h) == kReconTieOffPlane);
      CHECK(check_point_and_around(rt, fr, south, four_h) == kReconTieOffPlane);
      CHECK(check_point_and_around(rt, fr, centre, four_h) == kReconInside);
    }
  }
  CHECK(tally.ties_decided == 0);  // every exact tie came back undecided
  CHECK(tally.wrong == 0);

  if (failures) {
    std::printf("recon_check: %d check(s) failed; filter: %ld tests, %ld disagreements, %ld of %ld ties decided\n",
                failures, tally.tests(), tally.wrong, tally.ties_decided, tally.ties);
    return 1;
  }
  std::printf("recon_check: ok (%d inside, %d outside at the bound; filter: %ld inside, %ld outside, %ld undecided, "
              "%ld exact ties among them, 0 disagreements)\n",
              inside, outside, tally.inside, tally.outside, tally.undecided, tally.ties);
  return 0;
}
