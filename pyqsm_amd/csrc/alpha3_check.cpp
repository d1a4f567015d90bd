// alpha3_check.cpp — the two-sided predicate of the 3-D alpha shape (alpha3_exact.hpp) on the host, as a
// stand-alone program for AddressSanitizer and UndefinedBehaviorSanitizer (`make alpha3_check`):
//   alpha3_classify against recon_classify of the triple in both orientations, on every input below;
//   alpha3_filter against alpha3_classify: whenever it takes a sign for B+ or for B-, the integers are on
//   that side, hence every exact tie comes back undecided on the side it ties; its + side is recon_filter;
//   on a million random configurations at rho^2 = 2^22, on lattice points of two spheres with
//   rho^2 = r^2 just below 2^22, on the corners of a cube at its circumradius (coplanar and off-plane ties,
//   a plane through the centre with H == 0), on a right triangle whose hypotenuse is exactly 2 rho
//   (H == 0, one ball for both sides), and one lattice unit around every tie: the configurations §19 lists;
//   alpha3_kind on the cases of its table. Built with -ffp-contract=off, as the library is.
#include <cstdio>
#include <cstdlib>

#include "alpha3_exact.hpp"

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

struct Tally {
  long inside = 0, outside = 0, undecided = 0, ties = 0, ties_decided = 0, wrong = 0, mismatched = 0;
  long tests() const { return inside + outside + undecided; }
};
static Tally tally;  // both sides of every test counted, so two entries per point

static void count_side(int side, int where) {
  const bool tie = where == kReconTieCoplanar || where == kReconTieOffPlane;
  tally.inside += side == kReconFilterInside;
  tally.outside += side == kReconFilterOutside;
  tally.undecided += side == kReconFilterUndecided;
  tally.ties += tie;
  tally.ties_decided += tie && side != kReconFilterUndecided;
  const bool sound = side == kReconFilterUndecided || (side == kReconFilterInside && where == kReconInside) ||
                     (side == kReconFilterOutside && where == kReconOutside);
  if (!sound && tally.wrong++ < 10) std::printf("FAILED filter: side %d against the integers' %d\n", side, where);
}

// t: (a, b, c); r: (a, c, b), the same a. What the integers say of u for B+ of t, or -1 when |u|^2 > 4 rho^2.
static int check_point(const ReconTri& t, const ReconTri& r, const ReconFilterTri& f, const int64_t u[3],
                       uint64_t four_r2) {
  if (uint64_t(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) > four_r2) return -1;
  const Alpha3Sides where = alpha3_classify(t, u);
  if (where.plus != recon_classify(t, u) || where.minus != recon_classify(r, u)) ++tally.mismatched;
  const Alpha3Sides side = alpha3_filter(f, double(u[0]), double(u[1]), double(u[2]));
  if (side.plus != recon_filter(f, double(u[0]), double(u[1]), double(u[2]))) ++tally.mismatched;
  count_side(side.plus, where.plus);
  count_side(side.minus, where.minus);
  return where.plus;
}

static int check_point_and_around(const ReconTri& t, const ReconTri& r, const ReconFilterTri& f, const int64_t u[3],
                                  uint64_t four_r2) {
  const int where = check_point(t, r, f, u, four_r2);
  if (where == kReconTieCoplanar || where == kReconTieOffPlane)
    for (int d = 0; d < 3; ++d)
      for (int s = -1; s <= 1; s += 2) {
        int64_t v[3] = {u[0], u[1], u[2]};
        v[d] += s;
        check_point(t, r, f, v, four_r2);
      }
  return where;
}

// every triple i < j < k of pts against every other point of pts (and around the ties)
static void check_all_triples(const int64_t (*pts)[3], int n, uint64_t four_r2) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      for (int k = j + 1; k < n; ++k) {
        ReconTri t, r;
        if (!recon_setup(pts[i], pts[j], pts[k], four_r2, &t)) continue;
        CHECK(recon_setup(pts[i], pts[k], pts[j], four_r2, &r));
        const ReconFilterTri f = recon_filter_setup(t);
        for (int p = 0; p < n; ++p) {
          if (p == i || p == j || p == k) continue;
          const int64_t u[3] = {pts[p][0] - pts[i][0], pts[p][1] - pts[i][1], pts[p][2] - pts[i][2]};
          check_point_and_around(t, r, f, u, four_r2);
        }
      }
}

// 24 of the integer points of the sphere x^2 + y^2 + z^2 = r2, rho^2 = r2: one ball of every triple is the
// sphere itself, where every other point ties
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
  static int64_t pts[24][3];
  for (int k = 0; k < 24; ++k) {  // a fixed choice without repeats: the chosen point swaps with the last
    const long at = long(rng() % uint64_t(count - k));
    for (int d = 0; d < 3; ++d) {
      pts[k][d] = all[at][d];
      all[at][d] = all[count - 1 - k][d];
    }
  }
  const long ties = tally.ties;
  check_all_triples(pts, 24, 4 * uint64_t(r2));
  CHECK(tally.ties - ties >= 2024 * 21);  // one side of every test at the least
}

int main() {
  const uint64_t four_r2 = 4ull << 22;

  // ---- random at the bound: each candidate against eight points, a million configurations
  {
    long configs = 0;
    for (long it = 0; it < 40000000 && configs < 1000000; ++it) {
      int64_t v[3][3];
      for (int k = 0; k < 3; ++k)
        for (int d = 0; d < 3; ++d) v[k][d] = int64_t(rng() % 4730) - 2365;
      ReconTri q, r;
      if (!recon_setup(v[0], v[1], v[2], four_r2, &q)) continue;
      CHECK(recon_setup(v[0], v[2], v[1], four_r2, &r));
      const ReconFilterTri f = recon_filter_setup(q);
      for (int p = 0; p < 8; ++p) {
        int64_t u[3];
        for (int d = 0; d < 3; ++d) u[d] = int64_t(rng() % 4730) - 2365 - v[0][d];
        configs += check_point(q, r, f, u, four_r2) >= 0;
      }
    }
    CHECK(configs >= 1000000);
    CHECK(tally.inside > 0 && tally.outside > 0);
  }

  // ---- exactly cospherical families at the bound
  check_lattice_sphere(4191372, 6368);   // 3 * 1182^2: the circumsphere of a cube of edge 2364
  check_lattice_sphere(4194301, 14376);  // three below 2^22

  // ---- coplanar ties and H == 0 at the bound, and around them
  {
    int64_t cube[8][3];
    for (int k = 0; k < 8; ++k)
      for (int d = 0; d < 3; ++d) cube[k][d] = ((k >> d) & 1) * 2364 + (d == 0 ? -7 : d == 1 ? 1000003 : -2000001);
    const long ties = tally.ties;
    check_all_triples(cube, 8, 4ull * 4191372);
    CHECK(tally.ties > ties);
    ReconTri q;
    CHECK(recon_setup(cube[0], cube[1], cube[6], 4ull * 4191372, &q) && q.H == 0);  // an edge and the edge across
    // a face of the cube: the fourth corner ties in the plane on both balls, the opposite face off the
    // plane on one ball and lies outside the other
    ReconTri face;
    CHECK(recon_setup(cube[0], cube[1], cube[2], 4ull * 4191372, &face));
    const int64_t fourth[3] = {2364, 2364, 0}, up[3] = {0, 0, 2364}, down[3] = {0, 0, -2364};
    Alpha3Sides s = alpha3_classify(face, fourth);
    CHECK(s.plus == kReconTieCoplanar && s.minus == kReconTieCoplanar);
    s = alpha3_classify(face, up);
    CHECK(s.plus == kReconTieOffPlane && s.minus == kReconOutside);
    s = alpha3_classify(face, down);
    CHECK(s.plus == kReconOutside && s.minus == kReconTieOffPlane);
    // a right triangle whose hypotenuse is exactly 2 rho (legs 2454 and 3272, rho = 2045): H == 0, B+ = B-
    const uint64_t four_h = 4ull * 2045 * 2045;
    const int64_t a[3] = {1000000, -2000000, 5}, rb[3] = {a[0] + 2454, a[1], a[2]}, rc[3] = {a[0], a[1] + 3272, a[2]};
    ReconTri rt, rr;
    CHECK(recon_setup(a, rb, rc, four_h, &rt) && recon_setup(a, rc, rb, four_h, &rr));
    CHECK(rt.H == 0);
    const ReconFilterTri fr = recon_filter_setup(rt);
    const int64_t zero[3] = {0, 0, 0}, corner[3] = {2454, 3272, 0}, north[3] = {1227, 1636, 2045};
    const int64_t south[3] = {1227, 1636, -2045}, centre[3] = {1227, 1636, 0};
    CHECK(check_point_and_around(rt, rr, fr, zero, four_h) == kReconTieCoplanar);
    CHECK(check_point_and_around(rt, rr, fr, rt.e1, four_h) == kReconTieCoplanar);
    CHECK(check_point_and_around(rt, rr, fr, corner, four_h) == kReconTieCoplanar);
    CHECK(check_point_and_around(rt, rr, fr, north, four_h) == kReconTieOffPlane);
    CHECK(check_point_and_around(rt, rr, fr, south, four_h) == kReconTieOffPlane);
    CHECK(check_point_and_around(rt, rr, fr, centre, four_h) == kReconInside);
    s = alpha3_classify(rt, north);
    CHECK(s.plus == kReconTieOffPlane && s.minus == kReconTieOffPlane);  // one ball: both sides tie
    s = alpha3_classify(rt, centre);
    CHECK(s.plus == kReconInside && s.minus == kReconInside);
  }
  CHECK(tally.ties_decided == 0);  // every exact tie came back undecided on its side
  CHECK(tally.wrong == 0);
  CHECK(tally.mismatched == 0);

  // ---- the kinds
  {
    bool flip = true;
    CHECK(alpha3_kind(false, false, false, false, false, &flip) == kAlpha3None);
    CHECK(alpha3_kind(true, false, false, false, false, &flip) == kAlpha3Regular && !flip);
    CHECK(alpha3_kind(false, true, false, false, false, &flip) == kAlpha3Regular && flip);
    CHECK(alpha3_kind(true, true, false, false, false, &flip) == kAlpha3Singular && !flip);
    CHECK(alpha3_kind(true, true, false, false, true, &flip) == kAlpha3None);   // H == 0: one ball
    CHECK(alpha3_kind(true, false, false, true, false, &flip) == kAlpha3None);  // the fan rule drops it
    CHECK(alpha3_kind(true, false, true, true, false, &flip) == kAlpha3Regular);  // an off-plane tie keeps it
  }

  if (failures) {
    std::printf("alpha3_check: %d check(s) failed; filter: %ld sides, %ld disagreements, %ld of %ld ties decided, "
                "%ld mismatches with recon_exact.hpp\n",
                failures, tally.tests(), tally.wrong, tally.ties_decided, tally.ties, tally.mismatched);
    return 1;
  }
  std::printf("alpha3_check: ok (filter: %ld inside, %ld outside, %ld undecided, %ld exact ties among them, "
              "0 disagreements)\n",
              tally.inside, tally.outside, tally.undecided, tally.ties);
  return 0;
}
