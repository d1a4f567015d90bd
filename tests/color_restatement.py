"""Plain NumPy statements of the colour contract (include/pyqsm_hip.h "colours"): the two
conversions in matplotlib's operation order, the saturation lift, the rules and first match, the CSR by
class, the histogram by searchsorted, the two masks, homog_colors by brute-force neighbours, and the
clouds segment_hues builds from labels. Nothing here imports the product or matplotlib."""
import numpy as np

INF = float("inf")
NONE = 255

# name -> ((h_lo, h_hi, s_lo, s_hi, v_lo, v_hi), closed): pyQSM's color_conds, in its order
COLOR_CONDS = {
    "white": ((.5, 5 / 6, -INF, INF, .5, INF), 0),
    "pink": ((.7, INF, -INF, INF, .3, INF), 1),
    "blues": ((.4, .7, -INF, INF, .4, INF), 0),
    "subblue": ((.4, .4, -INF, INF, .3, INF), 0),
    "greens": ((2 / 9, .5, -INF, INF, .2, INF), 2),
    "light_greens": ((2 / 9, .5, -INF, INF, .5, INF), 2),
    "red_yellow": ((-INF, 2 / 9, -INF, INF, .3, INF), 2),
}
DEFAULT_HUES = ("white", "blues", "pink", "red_yellow", "greens")

EXTREME_ROWS = np.array([
    [1.0, 0.5, 0.5 + 2.0 ** -53],       # y a tiny negative: h == 1.0
    [1.0, 0.25, 0.25 + 2.0 ** -54],
    [1.0, 0.0, 1e-300],
    [0.0, 0.0, 0.0],
    [1.0, 1.0, 1.0],
    [1.0, 0.5 + 2.0 ** -53, 0.5],       # the same distance on the other side: h tiny and positive
    [2.0 ** -1074, 0.0, 0.0],           # the smallest subnormal
])


def rules_of(names):
    r = np.array([COLOR_CONDS[k][0] for k in names], np.float64).reshape(-1, 6)
    return r, np.array([COLOR_CONDS[k][1] for k in names], np.int32)


def rgb_to_hsv(rgb):
    a = np.asarray(rgb, np.float64).reshape(-1, 3)
    r, g, b = a[:, 0], a[:, 1], a[:, 2]
    mx, mn = a.max(axis=1), a.min(axis=1)
    d = mx - mn
    s = np.zeros_like(mx)
    pos = mx > 0
    s[pos] = d[pos] / mx[pos]
    x = np.zeros_like(mx)
    for sel, val in (((r == mx) & (d > 0), lambda m: (g[m] - b[m]) / d[m]),
                     ((g == mx) & (d > 0), lambda m: 2.0 + (b[m] - r[m]) / d[m]),
                     ((b == mx) & (d > 0), lambda m: 4.0 + (r[m] - g[m]) / d[m])):
        x[sel] = val(sel)                      # the last line that holds wins
    y = x / 6.0
    h = np.where(y < 0, y + 1.0, y)
    return np.stack([h, s, mx], axis=1)


def hsv_to_rgb(hsv):
    a = np.asarray(hsv, np.float64).reshape(-1, 3)
    h, s, v = a[:, 0], a[:, 1], a[:, 2]
    h6 = h * 6.0
    i = h6.astype(np.int64)
    f = h6 - i
    p = v * (1.0 - s)
    q = v * (1.0 - (s * f))
    t = v * (1.0 - (s * (1.0 - f)))
    table = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))
    out = np.empty_like(a)
    for c, cols in enumerate(table):
        m = i % 6 == c
        for ch in range(3):
            out[m, ch] = cols[ch][m]
    grey = s == 0
    out[grey] = v[grey, None]
    return out


def lift(s, min_s=.2, lift_div=3.0):
    s = np.asarray(s, np.float64)
    low = s < min_s
    out = s.copy()
    out[low] = s[low] + (1.0 - s[low]) / lift_div
    return out


def holds(hsv, rule, closed):
    ok = np.ones(len(hsv), bool)
    for c in range(3):
        x, lo, hi = hsv[:, c], rule[2 * c], rule[2 * c + 1]
        ok &= (x >= lo) if closed >> (2 * c) & 1 else (x > lo)
        ok &= (x <= hi) if closed >> (2 * c + 1) & 1 else (x < hi)
    return ok


def classify(hsv, rules, closed):
    cls = np.full(len(hsv), NONE, np.uint8)
    for k in range(len(rules) - 1, -1, -1):     # descending: the first rule that holds is written last
        cls[holds(hsv, rules[k], int(closed[k]))] = k
    return cls


def segment(rgb, rules, closed, min_s=.2, lift_div=3.0):
    """(cls u8 [n], counts i64 [K + 1], members i64 [n], corrected rgb, hsv of the corrected rgb)."""
    rgb = np.asarray(rgb, np.float64).reshape(-1, 3)
    rules = np.asarray(rules, np.float64).reshape(-1, 6)
    hsv = rgb_to_hsv(rgb)
    if lift_div == INF:                         # the identity: no lift, no round trip
        corrected, hsv2 = rgb.copy(), hsv
    else:
        corrected = hsv_to_rgb(np.stack([hsv[:, 0], lift(hsv[:, 1], min_s, lift_div), hsv[:, 2]], axis=1))
        hsv2 = rgb_to_hsv(corrected)
    cls = classify(hsv2, rules, closed)
    K = len(rules)
    codes = list(range(K)) + [NONE]
    counts = np.array([(cls == c).sum() for c in codes], np.int64)
    members = np.concatenate([np.nonzero(cls == c)[0] for c in codes]).astype(np.int64)
    return cls, counts, members, corrected, hsv2


def cascade(hsv2, rules, closed):
    """The reference's loop: every rule on what the rules before it left; the same classes as classify."""
    cls = np.full(len(hsv2), NONE, np.uint8)
    left = np.arange(len(hsv2))
    for k in range(len(rules)):
        hit = holds(hsv2[left], rules[k], int(closed[k]))
        cls[left[hit]] = k
        left = left[~hit]
    return cls


def bin_of(x, b):
    edges = np.linspace(0, 1, b + 1)
    return np.minimum(np.searchsorted(edges, x, "right") - 1, b - 1)


def histogram(hsv, bins, cls=None, which=-1):
    hsv = np.asarray(hsv, np.float64).reshape(-1, 3)
    if which >= 0:
        hsv = hsv[np.asarray(cls) == which]
    flat = (bin_of(hsv[:, 0], bins[0]) * bins[1] + bin_of(hsv[:, 1], bins[1])) * bins[2] + bin_of(hsv[:, 2], bins[2])
    return np.bincount(flat, minlength=bins[0] * bins[1] * bins[2]).astype(np.int64).reshape(bins)


def edge_values(bins):
    """Every edge of every channel's bins, and one ulp to either side, inside [0, 1]."""
    v = np.concatenate([np.linspace(0, 1, b + 1) for b in bins])
    v = np.concatenate([v, np.nextafter(v, 2.0), np.nextafter(v, -1.0)])
    return np.unique(v[(v >= 0) & (v <= 1)])


def mask_sum_gt(rgb, param=2.7):
    rgb = np.asarray(rgb, np.float64).reshape(-1, 3)
    return np.nonzero(((0.0 + rgb[:, 0]) + rgb[:, 1]) + rgb[:, 2] > param)[0].astype(np.int64)


def mask_green(rgb):
    rgb = np.asarray(rgb, np.float64).reshape(-1, 3)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = r / b
    return np.nonzero((g > r) & (g > b) & (0.5 < q) & (q < 2))[0].astype(np.int64)


def homog_colors(points, colors, k=30, white_sum=2.7):
    """The colours after homog_colors: a white point takes the mean colour of its min(k, count) nearest
    non-white points, neighbours ordered by (d2, index), summed in that order in fp64, divided by k."""
    points = np.asarray(points, np.float64)
    out = np.array(colors, np.float64)
    white = mask_sum_gt(out, white_sum)
    rest = np.setdiff1d(np.arange(len(out)), white)
    if len(white) == 0 or len(rest) == 0:
        return out
    kk = min(k, len(rest))
    src, src_col = points[rest], out[rest].copy()
    for w in white:
        dx, dy, dz = (points[w, a] - src[:, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        order = np.lexsort((np.arange(len(src)), d2))[:kk]
        acc = np.zeros(3)
        for j in order:
            acc = acc + src_col[j]
        out[w] = acc / kk
    return out


def segment_hues_layout(points, labels, corrected, n_hues):
    """What segment_hues returns, from labels (-1: none): lists of (points, colors). Entry 0 is the corrected
    cloud; then one entry per hue with members, the hue's rows and what is left after it, original order."""
    labels = np.asarray(labels)
    hue, rest = [(points, corrected)], [(points, corrected)]
    left = np.ones(len(labels), bool)
    for k in range(n_hues):
        m = labels == k
        if not m.any():
            continue
        left &= ~m
        hue.append((points[m], corrected[m]))
        rest.append((points[left], corrected[left]))
    return hue, rest


# ---- the inputs csrc/color_check.cpp generates, and its hash

def check_inputs():
    g = np.arange(17) / 16.0
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    state, vals = 1, []
    for _ in range(3 * 32768):
        state = (state * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        vals.append((state >> 33) % 256)
    lcg = np.array(vals, np.float64).reshape(-1, 3) / 255.0
    return np.concatenate([grid, lcg, EXTREME_ROWS])


def fnv1a(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for byte in data:
        h = ((h ^ byte) * 0x100000001b3) % (1 << 64)
    return h


# ---- the base set of the GPU tests

def base_set():
    rng = np.random.default_rng(7)
    rgb = rng.integers(0, 256, (6000, 3)) / 255.0
    rgb[:300] = np.clip(.9 + .1 * rng.random((300, 3)), 0, 1)
    rgb[300:400] = rng.integers(0, 256, (100, 1)) / 255.0
    return rgb
