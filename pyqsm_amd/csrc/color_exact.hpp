// color_exact.hpp — the colour contract of color.hip, one statement for the kernels, the
// host-side input check and the stand-alone sanitizer program (color_check.cpp).
//
// Everything is fp64, one operation at a time, in the order written here, without contraction
// (-ffp-contract=off): the conversions reproduce matplotlib.colors.rgb_to_hsv / hsv_to_rgb bit for bit.
//
// rgb -> hsv, (r, g, b) in [0, 1]:
//   mx = max, mn = min, d = mx - mn;  v = mx;  s = mx > 0 ? d / mx : 0
//   d > 0: the LAST line that holds wins:  r == mx: x = (g - b) / d
//                                          g == mx: x = 2.0 + (b - r) / d
//                                          b == mx: x = 4.0 + (r - g) / d      otherwise x = 0
//   y = x / 6.0 (a division);  h = y < 0 ? y + 1.0 : y   (a tiny negative y gives h == 1.0, as NumPy's % 1.0)
// hsv -> rgb:
//   h6 = h * 6.0;  i = (int64) h6;  f = h6 - i
//   p = v * (1.0 - s);  q = v * (1.0 - (s * f));  t = v * (1.0 - (s * (1.0 - f)))
//   i % 6: 0 (v,t,p)  1 (q,v,p)  2 (p,v,t)  3 (p,q,v)  4 (t,p,v)  5 (v,p,q);  h == 1.0 is case 0
//   s == 0 gives (v, v, v)
// lift: s' = s < min_s ? s + (1.0 - s) / lift_div : s. lift_div = +inf is the identity: no lift and no round
//   trip, the corrected colour is the input's bits and its hsv the first conversion (the round trip through
//   hsv moves last bits even with s' == s, so "unchanged" has to be said, it does not follow).
// rule k: (h_lo, h_hi, s_lo, s_hi, v_lo, v_hi), ±inf for "unbounded"; bit 2c of closed[k] makes the lower
//   bound of channel c inclusive, bit 2c + 1 the upper one. The class of a row is the first rule that
//   holds on rgb_to_hsv(hsv_to_rgb(h, s', v)), kColorNone when none does.
// bin of x among b bins: min(searchsorted(linspace(0, 1, b + 1), x, 'right') - 1, b - 1), the edges being
//   j * (1.0 / b) for j < b and 1.0 for j == b, as NumPy builds them.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PQ_COLOR_HD __host__ __device__ __forceinline__
#else
#define PQ_COLOR_HD inline
#endif

namespace pyqsm {

static constexpr int kColorMaxRules = 16;   // PYQSM_COLOR_MAX_RULES
static constexpr int kColorNone = 255;

// by value in the kernels' arguments: 16 * 6 * 8 + 16 * 4 + 4 bytes
struct ColorRules {
  int32_t K;
  int32_t closed[kColorMaxRules];
  double b[kColorMaxRules][6];
};

PQ_COLOR_HD bool color_in_range(double x) { return x >= 0.0 && x <= 1.0; }  // false for a NaN

PQ_COLOR_HD void rgb_to_hsv_exact(double r, double g, double b, double& h, double& s, double& v) {
  const double mx = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const double mn = r < g ? (r < b ? r : b) : (g < b ? g : b);
  const double d = mx - mn;
  v = mx;
  s = mx > 0.0 ? d / mx : 0.0;
  double x = 0.0;
  if (d > 0.0) {
    if (r == mx) x = (g - b) / d;
    if (g == mx) x = 2.0 + (b - r) / d;
    if (b == mx) x = 4.0 + (r - g) / d;
  }
  const double y = x / 6.0;
  h = y < 0.0 ? y + 1.0 : y;
}

PQ_COLOR_HD void hsv_to_rgb_exact(double h, double s, double v, double& r, double& g, double& b) {
  const double h6 = h * 6.0;
  // h in [0, 1]; anything else (a refused input whose outputs are unspecified) takes case 0
  const int64_t i = (h6 >= 0.0 && h6 <= 6.0) ? int64_t(h6) : 0;
  const double f = h6 - double(i);
  const double p = v * (1.0 - s);
  const double q = v * (1.0 - (s * f));
  const double t = v * (1.0 - (s * (1.0 - f)));
  const int c = int(i % 6);
  r = c == 0 ? v : c == 1 ? q : c == 2 ? p : c == 3 ? p : c == 4 ? t : v;
  g = c == 0 ? t : c == 1 ? v : c == 2 ? v : c == 3 ? q : c == 4 ? p : p;
  b = c == 0 ? p : c == 1 ? p : c == 2 ? t : c == 3 ? v : c == 4 ? v : q;
  if (s == 0.0) r = g = b = v;
}

PQ_COLOR_HD double lift_saturation(double s, double min_s, double lift_div) {
  return s < min_s ? s + (1.0 - s) / lift_div : s;
}

PQ_COLOR_HD bool color_bound_holds(double x, double lo, double hi, int bits) {
  const bool a = (bits & 1) ? x >= lo : x > lo;
  const bool b = (bits & 2) ? x <= hi : x < hi;
  return a && b;
}

PQ_COLOR_HD int color_class(const ColorRules& R, double h, double s, double v) {
  int cls = kColorNone;
  for (int k = 0; k < R.K; ++k) {
    const int cl = R.closed[k];
    const bool ok = color_bound_holds(h, R.b[k][0], R.b[k][1], cl) &&
                    color_bound_holds(s, R.b[k][2], R.b[k][3], cl >> 2) &&
                    color_bound_holds(v, R.b[k][4], R.b[k][5], cl >> 4);
    if (ok && cls == kColorNone) cls = k;
  }
  return cls;
}

// the whole segmentation of one row: corrected rgb, the hsv of the corrected rgb, the class
PQ_COLOR_HD int color_segment_row(const ColorRules& R, double min_s, double lift_div, double r, double g, double b,
                                  double out_rgb[3], double out_hsv[3]) {
  double h, s, v;
  rgb_to_hsv_exact(r, g, b, h, s, v);
  if (lift_div > 1.7976931348623157e308) {  // +inf: the identity
    out_rgb[0] = r, out_rgb[1] = g, out_rgb[2] = b;
    out_hsv[0] = h, out_hsv[1] = s, out_hsv[2] = v;
    return color_class(R, h, s, v);
  }
  hsv_to_rgb_exact(h, lift_saturation(s, min_s, lift_div), v, out_rgb[0], out_rgb[1], out_rgb[2]);
  rgb_to_hsv_exact(out_rgb[0], out_rgb[1], out_rgb[2], out_hsv[0], out_hsv[1], out_hsv[2]);
  return color_class(R, out_hsv[0], out_hsv[1], out_hsv[2]);
}

PQ_COLOR_HD double color_edge(int j, int b, double step) { return j >= b ? 1.0 : double(j) * step; }

// always inside [0, b - 1], also for a NaN or a value outside [0, 1] (refused inputs)
PQ_COLOR_HD int color_bin(double x, int b) {
  const double step = 1.0 / double(b);
  int j = (x > 0.0 && x <= 1.0) ? int(x * double(b)) : 0;
  if (j > b) j = b;
  while (j < b && color_edge(j + 1, b, step) <= x) ++j;   // edges <= x: j + 1 of them
  while (j > 0 && color_edge(j, b, step) > x) --j;
  return j < b - 1 ? j : b - 1;
}

// PYQSM_MASK_SUM_GT / PYQSM_MASK_GREEN
PQ_COLOR_HD bool color_mask_row(int kind, double param, double r, double g, double b) {
  if (kind == 0) return ((0.0 + r) + g) + b > param;
  const double q = r / b;   // b == 0: inf or NaN, false either way
  return g > r && g > b && 0.5 < q && q < 2.0;
}

}  // namespace pyqsm
