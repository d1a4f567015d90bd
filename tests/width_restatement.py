"""The contract of the stem-width measurement (pyqsm_pdist_select and geometry/stem_width.py), stated
with NumPy and SciPy only: the sorted pdist of every segment, numpy's percentile rule on it, the slab
rule and the farthest pair. Nothing here imports the project."""
import math

import numpy as np
from scipy.spatial.distance import pdist

KINDS = ("normal", "lattice", "logspread", "equal")


def make_points(kind, n, dim, seed):
    """The four input kinds of the tests: float64 [n, dim]."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.normal(size=(n, dim))
    if kind == "lattice":                   # a few dozen distinct points: long runs of equal keys, many zeros
        return rng.integers(0, 6, size=(n, dim)).astype(np.float64)
    if kind == "logspread":                 # distances over 30 binary exponents
        return rng.choice([-1.0, 1.0], size=(n, dim)) * 10.0 ** rng.uniform(-6, 3, size=(n, dim))
    if kind == "equal":
        return np.tile(rng.normal(size=(1, dim)), (n, 1))
    raise ValueError(kind)


def sorted_pdist(P):
    """sort(pdist(P)); empty for fewer than two points."""
    P = np.asarray(P, dtype=np.float64)
    if len(P) < 2:
        return np.zeros(0)
    return np.sort(pdist(P))


def squared_keys(P):
    """d2 of every pair i < j in pdist's order, (dx*dx) + (dy*dy) [+ (dz*dz)], and the pairs."""
    P = np.asarray(P, dtype=np.float64)
    i, j = np.triu_indices(len(P), k=1)
    d = P[i] - P[j]
    d2 = (d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])
    if P.shape[1] == 3:
        d2 = d2 + (d[:, 2] * d[:, 2])
    return d2, i, j


def farthest_pair(P):
    """(i, j), i < j, with the largest d2, of equal ones the smallest in lexicographic order; (-1, -1)
    for fewer than two points."""
    if len(P) < 2:
        return (-1, -1)
    d2, i, j = squared_keys(P)
    k = int(np.argmax(d2))                  # the first maximum in pdist's order, which is lexicographic
    return (int(i[k]), int(j[k]))


def percentile(dsorted, q):
    """np.percentile(d, q), method 'linear', restated on the sorted values; 0.0 for no values."""
    m = len(dsorted)
    if m == 0:
        return 0.0
    v = (m - 1) * np.true_divide(q, 100)
    lo = math.floor(v)
    hi = min(lo + 1, m - 1)
    t = v - lo
    a, b = dsorted[lo], dsorted[hi]
    if t == 0:
        return float(a)
    if t >= 0.5:
        return float(b - (b - a) * (1 - t))
    return float(a + (b - a) * t)


def slab(points, height, tolerance, axis=2):
    """Indices of the points within ground + height ± tolerance along axis, both ends included."""
    pts = np.asarray(points, dtype=np.float64)
    if len(pts) == 0:
        return np.zeros(0, np.int64)
    ground = np.min(pts[:, axis])
    lo, hi = ground + height - tolerance, ground + height + tolerance
    return np.array([k for k in range(len(pts)) if lo <= pts[k, axis] <= hi], np.int64)


def widths(points, kept, axis=2):
    """Every field of width_at_height except the seed, for the points ``kept`` (indices into points)."""
    pts = np.asarray(points, dtype=np.float64)
    kept = np.asarray(kept, np.int64)
    plane = pts[kept][:, [a for a in range(3) if a != axis]]
    d = sorted_pdist(plane)
    far = farthest_pair(plane)
    p95 = percentile(d, 95)
    return {
        'width': p95,
        'bounds': pts[kept].max(axis=0) - pts[kept].min(axis=0) if len(kept) else np.zeros(3),
        'p90': percentile(d, 90),
        'p95': p95,
        'median': float(np.median(d)) if len(d) else 0.0,
        'max_width': float(d[-1]) if len(d) else 0.0,
        'max_pair': (int(kept[far[0]]), int(kept[far[1]])) if len(d) else (-1, -1),
        'n_points': len(kept),
        'n_pairs': len(d),
    }


def cylinder(n=3000, radius=0.15, sigma=0.005, top=3.0, seed=5):
    """A noisy vertical cylinder standing on z = 0: float64 [n,3]."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n)
    r = radius + rng.normal(0, sigma, n)
    z = rng.uniform(0, top, n)
    z[0] = 0.0
    return np.stack([r * np.cos(ang), r * np.sin(ang), z], axis=1)
