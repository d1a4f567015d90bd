// recon_check.cpp — the integer side of the ball-pivoting predicate (recon_exact.hpp) on the host, as a
// stand-alone program for AddressSanitizer and UndefinedBehaviorSanitizer (`make recon_check`):
//   mul_u128 / cmp_u256 against a schoolbook product in 32-bit limbs, operands at the bounds of §19;
//   recon_setup / recon_classify at the largest admitted radius (rho^2 = 2^22): the vertices of a
//   candidate are ties in its plane, points above and below it fall inside and outside its ball, the
//   corners of a cube are ties on and off the plane of one of its faces, and signed overflow anywhere
//   would stop the run.
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

  if (failures) {
    std::printf("recon_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("recon_check: ok (%d inside, %d outside at the bound)\n", inside, outside);
  return 0;
}
