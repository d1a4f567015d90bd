"""The radius graph's contract on the CPU, by brute force in NumPy (tests/test_density_host.py pins it
to SciPy's cKDTree; tests/test_gpu_density.py compares the GPU with it, exactly).

{i, j}, i != j, is an edge when d2 = ((dx*dx) + dy*dy) + dz*dz <= r*r, everything in fp64 with
separately rounded products, the bound inclusive, coincident points joined. degree[i] is the number
of edges at i, the pair list holds every edge once as (i, j), i < j, ascending by (i, j), and the
components are ranked by (size descending, smallest member ascending).

Every point is tested against the points of the nine columns around its own that lie in its block's
height window: the points are binned in x and y into columns of edge w = r (1 + 2^-20), a column's
points are taken in ascending z, BLOCK at a time, and a block meets the points of the nine columns
whose z lies within w of the block's range. A pair with d2 <= r*r has fl(dx*dx) <= d2 (a rounded sum
of non-negative terms is no smaller than either term), so |dx| <= r (1 + 2^-52), likewise |dy| and
|dz|: the true column coordinates of the two points differ by less than 1 - 2^-21, the computed ones,
floor((x - min x) / w), carry an error below 2^-51 times their size, so up to 2^29 columns per axis
(asserted, also for |z| / w) the two floors differ by at most one and the rounded window bounds keep
every such z. The columns and windows leave no edge out, and inside them the test is the contract's own.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

BLOCK = 64


def _blocks(P, rmax):
    """(rows, candidates) index arrays covering every pair within rmax."""
    P = np.asarray(P, dtype=np.float64)
    w = rmax * (1.0 + 2.0 ** -20)
    cx = np.floor((P[:, 0] - P[:, 0].min()) / w).astype(np.int64)
    cy = np.floor((P[:, 1] - P[:, 1].min()) / w).astype(np.int64)
    z = P[:, 2]
    assert cx.max() < 2 ** 29 and cy.max() < 2 ** 29 and np.abs(z).max() / w < 2 ** 29
    key = cx * 2 ** 30 + cy
    order = np.lexsort((z, key))
    keys, start, count = np.unique(key[order], return_index=True, return_counts=True)
    where = {int(k): (int(s), int(c)) for k, s, c in zip(keys, start, count)}
    for k, (s, c) in where.items():
        near = [where.get(k + dx * 2 ** 30 + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]
        cand = np.concatenate([order[a:a + m] for a, m in (q for q in near if q is not None)])
        zc = z[cand]
        for b in range(s, s + c, BLOCK):
            rows = order[b:min(b + BLOCK, s + c)]             # ascending z
            yield rows, cand[(zc >= z[rows[0]] - w) & (zc <= z[rows[-1]] + w)]


def _d2(P, rows, cand):
    d = P[rows][:, None, :] - P[cand][None, :, :]
    return ((d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def degrees(P, radii):
    """(degree int32 [R, n], n_pairs int64 [R])."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    radii = np.atleast_1d(np.asarray(radii, dtype=np.float64))
    deg = np.zeros((len(radii), len(P)), dtype=np.int64)
    if len(P):
        for rows, cand in _blocks(P, radii.max()):
            d2 = _d2(P, rows, cand)
            for k, r in enumerate(radii):
                deg[k, rows] = (d2 <= r * r).sum(1) - 1        # the point itself, at d2 = 0
    return deg.astype(np.int32), deg.sum(1) // 2


def pairs(P, r):
    """int32 [m, 2]: i < j, ascending by (i, j)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    out = [np.zeros((0, 2), dtype=np.int64)]
    if len(P):
        for rows, cand in _blocks(P, r):
            a, b = np.nonzero(_d2(P, rows, cand) <= r * r)
            i, j = rows[a], cand[b]
            keep = i < j
            out.append(np.stack([i[keep], j[keep]], 1))
    p = np.concatenate(out)
    return p[np.lexsort((p[:, 1], p[:, 0]))].astype(np.int32)


def rank_components(labels):
    """(component int32 [n], sizes int32 [c]) from any labelling of the components: ranks by
    (size descending, smallest member ascending)."""
    labels = np.asarray(labels)
    n = len(labels)
    if n == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    _, first, inv, counts = np.unique(labels, return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((first, -counts))
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    return rank[inv].astype(np.int32), counts[order].astype(np.int32)


def components(P, r, pair_list=None):
    """(component int32 [n], sizes int32 [c]) of the graph at r."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    p = pairs(P, r) if pair_list is None else pair_list
    n = len(P)
    g = coo_matrix((np.ones(len(p), dtype=np.int8), (p[:, 0], p[:, 1])), shape=(n, n))
    _, lab = connected_components(g, directed=False)
    return rank_components(lab)


# ---- the families of points the tests share ------------------------------------------------------

def lattice(seed=0):
    """A shuffled 16^3 lattice of spacing 1/64 (every d2 exact: ties on the bound are real ties)."""
    g = np.arange(16)
    L = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) / 64.0
    return L[np.random.default_rng(seed).permutation(len(L))]


LATTICE_RADII = (3 / 64, 1 / 64, np.sqrt(2) / 64, np.sqrt(3) / 64)
LATTICE_PAIRS = (199572, 11520, 33120, 33120)   # sqrt(3)/64: the rounded r*r falls below 3/4096


def chain(n=2000, h=2.0 ** -5):
    C = np.zeros((n, 3))
    C[:, 0] = np.arange(n) * h
    return C


def uniform(n, seed=1):
    return np.random.default_rng(seed).random((n, 3))


def fp32_valued(n=5000, seed=2, scale=10.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)).astype(np.float32) * np.float32(scale)).astype(np.float64)


def ball(m, r, seed=3):
    """m points inside a ball of diameter below r: one clique, all in one cell or its neighbours."""
    rng = np.random.default_rng(seed + m)
    v = rng.standard_normal((m, 3))
    v *= (0.49 * r * rng.random((m, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
    return v + np.array([0.5, 0.5, 0.5])


def small_components(seed=5):
    """Many two-point and three-point components (and single points), far apart, in shuffled order:
    the ranking's ties are decided by the smallest member. Returns (points, radius)."""
    rng = np.random.default_rng(seed)
    centres = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(6), indexing="ij"), -1).reshape(-1, 3) * 1.0
    pts = []
    for k, c in enumerate(centres):
        for q in range(1 + k % 3):
            pts.append(c + 0.05 * q * np.array([1.0, 0.0, 0.0]))
    pts = np.array(pts)
    return pts[rng.permutation(len(pts))], 0.06


# ---- the host statements of the analysis layer --------------------------------------------------------

def get_pairs(P, r):
    """pyQSM's get_pairs by its own recipe: the degree from a count over the pair list."""
    p = pairs(P, r)
    deg = np.bincount(p.ravel(), minlength=len(P))
    return deg, np.unique(deg, return_counts=True)[1], p


def degree_split(P, r, pct):
    deg = degrees(P, [r])[0][0]
    cut = np.percentile(deg, pct)
    return np.where(deg < cut)[0], np.where(deg >= cut)[0], deg

