// color_check.cpp — the colour contract (color_exact.hpp) on the host, as a stand-alone program for
// AddressSanitizer and UndefinedBehaviorSanitizer (`make color_check`). The inputs follow from integer
// rules, so that tests/test_color_host.py builds the same rows in NumPy:
//   all (i/16, j/16, k/16), i outermost, i, j, k = 0 .. 16;
//   32 768 rows (a/255, b/255, c/255) with a, b, c = (state >> 33) % 256 drawn in this order from
//   state = state * 6364136223846793005 + 1442695040888963407 (mod 2^64), state = 1 at the start;
//   the hue-wrap and extreme rows.
// It prints a 64-bit FNV-1a hash of each stage's output bytes: the hsv rows, the corrected rgb at the default
// lift (min_s = 0.2, lift_div = 3), the class bytes under pyQSM's seven rules in table order, and the
// (16, 8, 8) histogram of the hsv rows as int64. The test compares them with the restatement's, which is
// pinned to matplotlib's bits: this ties the device header to matplotlib without a GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "color_exact.hpp"

using namespace pyqsm;

static uint64_t fnv1a(const void* p, size_t bytes) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < bytes; ++i) {
    h ^= b[i];
    h *= 0x100000001b3ull;
  }
  return h;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> rgb;
  for (int i = 0; i <= 16; ++i)
    for (int j = 0; j <= 16; ++j)
      for (int k = 0; k <= 16; ++k) {
        rgb.push_back(i / 16.0);
        rgb.push_back(j / 16.0);
        rgb.push_back(k / 16.0);
      }
  uint64_t state = 1;
  for (int t = 0; t < 3 * 32768; ++t) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    rgb.push_back(double((state >> 33) % 256) / 255.0);
  }
  const double wrap[7][3] = {{1.0, 0.5, 0.5 + std::ldexp(1.0, -53)}, {1.0, 0.25, 0.25 + std::ldexp(1.0, -54)},
                             {1.0, 0.0, 1e-300},                     {0.0, 0.0, 0.0},
                             {1.0, 1.0, 1.0},                        {1.0, 0.5 + std::ldexp(1.0, -53), 0.5},
                             {std::ldexp(1.0, -1074), 0.0, 0.0}};
  for (const auto& w : wrap)
    for (double v : w) rgb.push_back(v);
  const size_t n = rgb.size() / 3;

  // pyQSM's table: white, pink, blues, subblue, greens, light_greens, red_yellow
  ColorRules R;
  std::memset(&R, 0, sizeof(R));
  R.K = 7;
  const double hb[7][2] = {{.5, 5.0 / 6}, {.7, inf}, {.4, .7}, {.4, .4}, {2.0 / 9, .5}, {2.0 / 9, .5}, {-inf, 2.0 / 9}};
  const int hclosed[7] = {0, 1, 0, 0, 2, 2, 2};
  const double vlo[7] = {.5, .3, .4, .3, .2, .5, .3};
  for (int k = 0; k < 7; ++k) {
    R.closed[k] = hclosed[k];
    R.b[k][0] = hb[k][0];
    R.b[k][1] = hb[k][1];
    R.b[k][2] = -inf;
    R.b[k][3] = inf;
    R.b[k][4] = vlo[k];
    R.b[k][5] = inf;
  }

  std::vector<double> hsv(3 * n), corrected(3 * n);
  std::vector<unsigned char> cls(n);
  std::vector<int64_t> hist(16 * 8 * 8, 0);
  int wraps = 0;
  for (size_t i = 0; i < n; ++i) {
    double* h = &hsv[3 * i];
    rgb_to_hsv_exact(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], h[0], h[1], h[2]);
    wraps += h[0] == 1.0;
    double h2[3];
    cls[i] = (unsigned char)color_segment_row(R, 0.2, 3.0, rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2],
                                              &corrected[3 * i], h2);
    ++hist[(color_bin(h[0], 16) * 8 + color_bin(h[1], 8)) * 8 + color_bin(h[2], 8)];
  }
  std::printf("rows %zu wraps %d\n", n, wraps);
  std::printf("hsv %016llx\n", (unsigned long long)fnv1a(hsv.data(), hsv.size() * 8));
  std::printf("corrected %016llx\n", (unsigned long long)fnv1a(corrected.data(), corrected.size() * 8));
  std::printf("class %016llx\n", (unsigned long long)fnv1a(cls.data(), cls.size()));
  std::printf("hist %016llx\n", (unsigned long long)fnv1a(hist.data(), hist.size() * 8));
  std::printf("color_check: ok\n");
  return 0;
}
