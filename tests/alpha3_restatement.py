"""The 3-D alpha-shape contract of pyqsm_alpha_shape3 restated on the CPU, twice.

``brute``      the definition: every triple of points of one segment with a circumradius of at most rho,
               BOTH its balls against every other point of the segment, the tie rule, the kinds, the
               orientation and six times the volume. The ball B- of (a, b, c) is evaluated as the ball B+
               of (a, c, b), from that triple's own quantities: nothing is shared between the two sides.
``delaunay``   an independent route for clouds in general position (asserted): scipy's Delaunay tetrahedra,
               kept when their exact circumradius is below rho; the faces that belong to exactly one kept
               tetrahedron, oriented away from it, and the volume as the sum of the kept tetrahedra.

Every decision is an evaluation in Python integers (``setup`` / ``classify`` / ``beyond_bc`` of
tests/recon_restatement.py). ``brute`` first orders its work with fp64: a point whose fp64 value of
N -+ sqrt(H) D is beyond 2^-30 of the magnitude of its terms (2^18 times the rounding error of that
evaluation) is taken at that sign; everything closer, hence every tie, is classified by the integers.
"""
import functools
import math

import numpy as np

from tests.recon_restatement import (INSIDE, TIE_COPLANAR, TIE_OFF_PLANE, as_ints, beyond_bc, classify, cross, dot,
                                     setup)

REGULAR, SINGULAR = 1, 2


def det3(a, b, c):
    return dot(a, cross(b, c))


def six_volume(P, rows, origin):
    """The sum of det(a - o, b - o, c - o) over the regular rows, in Python integers."""
    o = P[origin]
    total = 0
    for a, b, c, kind in rows:
        if kind == REGULAR:
            total += det3(*(tuple(x - y for x, y in zip(P[q], o)) for q in (a, b, c)))
    return total


def _sweep(t, Pl, a, near_points):
    """(blocked, off-plane tie, fan-rule drop) of the ball B+ of the oriented triple t over the given points."""
    off = drop = False
    for p in near_points:
        u = tuple(x - y for x, y in zip(Pl[p], Pl[a]))
        w = classify(t, u)
        if w == INSIDE:
            return True, off, drop
        if w == TIE_OFF_PLANE:
            off = True
        elif w == TIE_COPLANAR and (p < a or beyond_bc(t, u)):
            drop = True
    return False, off, drop


def _candidates(P, Pl, near, i, rho2):
    """The candidate pairs (j, k), i < j < k, of point i with their int64 / fp64 quantities, or None: both within
    2 rho of i and of each other, not collinear with it, circumradius at most rho (H >= 0)."""
    nb = np.asarray([j for j in np.nonzero(near[i])[0].tolist() if j > i], dtype=np.int64)
    if len(nb) < 2:
        return None
    x, y = np.triu_indices(len(nb), 1)
    J, K = nb[x], nb[y]
    e1, e2 = P[J] - P[i], P[K] - P[i]
    nn = np.cross(e1, e2)
    l1, l2, l3 = (e1 * e1).sum(axis=1), (e2 * e2).sum(axis=1), ((e2 - e1) ** 2).sum(axis=1)
    n2 = (nn * nn).sum(axis=1)
    big, small = 4.0 * rho2 * n2.astype(np.float64), l1.astype(np.float64) * l2 * l3
    maybe = near[J, K] & (n2 > 0) & (big - small >= -1e-9 * small)
    # the circumradius in Python integers where fp64 is not sure of it
    unsure = maybe & (np.abs(big - small) <= 1e-9 * small)
    for q in np.nonzero(unsure)[0].tolist():
        maybe[q] = setup(Pl[i], Pl[int(J[q])], Pl[int(K[q])], rho2) is not None
    if not maybe.any():
        return None
    return tuple(v[maybe] for v in (J, K, e1, e2, nn, l1, l2, n2, big, small))


def work(P, rho2, seg_start=None):
    """(candidate triples, ball tests) as the library counts them: a candidate is tested against every other
    point of its segment within 2 rho of its lowest vertex."""
    P = np.asarray(P, dtype=np.int64).reshape(-1, 3)
    cands = tests = 0
    for lo, hi in _segments(len(P), seg_start):
        Q = P[lo:hi]
        Ql = as_ints(Q)
        near = ((Q[:, None, :] - Q[None, :, :]) ** 2).sum(axis=2) <= 4 * rho2
        for i in range(len(Q)):
            got = _candidates(Q, Ql, near, i, rho2)
            if got is not None:
                cands += len(got[0])
                tests += len(got[0]) * (int(near[i].sum()) - 1)
    return cands, tests


def brute_segment(P, rho2):
    """[(a, b, c, kind, kept with an off-plane tie)] of one segment, unsorted."""
    P = np.asarray(P, dtype=np.int64).reshape(-1, 3)
    n = len(P)
    Pf, Pl = P.astype(np.float64), as_ints(P)
    d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    near = d2 <= 4 * rho2
    rows = []
    for i in range(n):
        got = _candidates(P, Pl, near, i, rho2)
        if got is None:
            continue
        J, K, e1, e2, nn, l1, l2, n2, big, small = got
        if len(J) == 0:
            continue
        H = np.maximum(big - small, 0.0)
        w = l1[:, None] * np.cross(e2, nn) + l2[:, None] * np.cross(nn, e1)      # exact: below 2^61
        # fp64 only to order the work (module docstring): one column per candidate, one row per point
        U = Pf - Pf[i]
        D = U @ nn.astype(np.float64).T
        t0 = (U * U).sum(axis=1)[:, None] * n2.astype(np.float64)
        Nf = t0 - U @ w.astype(np.float64).T
        rhs = D * np.sqrt(H)
        scale = (t0 + np.abs(U) @ np.abs(w.astype(np.float64)).T + np.abs(rhs)) * 2.0 ** -30
        cols = np.arange(len(J))
        own = np.zeros_like(Nf, dtype=bool)
        own[i, :] = True
        own[J, cols] = True
        own[K, cols] = True
        sides = []
        for val in (Nf - rhs, Nf + rhs):
            clearly = ((val < -scale) & ~own).any(axis=0)
            close = (np.abs(val) <= scale) & ~own
            sides.append((clearly, close))
        for q in cols.tolist():
            j, k = int(J[q]), int(K[q])
            res = []
            for (clearly, close), (b, c) in zip(sides, ((j, k), (k, j))):
                if clearly[q]:
                    res.append((True, False, False))
                    continue
                pts = np.nonzero(close[:, q])[0].tolist()
                res.append(_sweep(setup(Pl[i], Pl[b], Pl[c], rho2), Pl, i, pts) if pts else (False, False, False))
            (bp, op, dp), (bm, om, dm) = res
            if bp and bm:
                continue
            unres = (not bp and op) or (not bm and om)
            if (dp or dm) and not unres:
                continue
            if setup(Pl[i], Pl[j], Pl[k], rho2)["H"] == 0:
                continue
            if not bp and not bm:
                rows.append((i, j, k, SINGULAR, bool(unres)))
            else:
                rows.append((i, j, k, REGULAR, bool(unres)) if not bp else (i, k, j, REGULAR, bool(unres)))
    return rows


def _segments(n, seg_start):
    seg = [0, n] if seg_start is None else [int(v) for v in seg_start]
    return list(zip(seg[:-1], seg[1:]))


def brute(P, rho2, seg_start=None, faces="all"):
    """(rows int32 [R,4] ascending by (a, b, c), vol6 per segment as Python integers, listed rows kept with an
    off-plane tie). With faces="regular" the singular rows are left out."""
    P = np.asarray(P, dtype=np.int64).reshape(-1, 3)
    Pl = as_ints(P)
    rows, vol6, unresolved = [], [], 0
    for lo, hi in _segments(len(P), seg_start):
        seg_rows = [(a + lo, b + lo, c + lo, kind, unres) for a, b, c, kind, unres in brute_segment(P[lo:hi], rho2)
                    if faces == "all" or kind == REGULAR]
        vol6.append(six_volume(Pl, [r[:4] for r in seg_rows], lo) if hi > lo else 0)
        rows += [r[:4] for r in seg_rows]
        unresolved += sum(r[4] for r in seg_rows)
    return np.array(sorted(rows), np.int32).reshape(-1, 4), vol6, unresolved


def circumsphere(p0, p1, p2, p3):
    """(x, det) of a tetrahedron in Python integers: the circumcentre is p0 + x / (2 det), the squared
    circumradius |x|^2 / (4 det^2)."""
    r = [tuple(a - b for a, b in zip(p, p0)) for p in (p1, p2, p3)]
    s = [dot(v, v) for v in r]
    det = det3(*r)
    c12, c20, c01 = cross(r[1], r[2]), cross(r[2], r[0]), cross(r[0], r[1])
    x = tuple(s[0] * c12[k] + s[1] * c20[k] + s[2] * c01[k] for k in range(3))
    return x, det


def delaunay_segment(P, rho2):
    """The regular rows of one segment in general position and six times the volume of the kept tetrahedra."""
    from scipy.spatial import Delaunay
    P = np.asarray(P, dtype=np.int64).reshape(-1, 3)
    Pl = as_ints(P)
    if len(P) < 4:
        return [], 0
    tri = Delaunay(P.astype(np.float64))
    assert tri.coplanar.size == 0, "qhull left points out (coincident points?): not in general position"
    kept, spheres = [], []
    for s in tri.simplices.tolist():
        x, det = circumsphere(*(Pl[q] for q in s))
        assert det != 0, "a flat tetrahedron: not in general position"
        lhs, rhs = dot(x, x), 4 * det * det * rho2
        assert lhs != rhs, "a circumradius equal to alpha: not in general position"
        kept.append(lhs < rhs)
        spheres.append((x, det))
    for si, (s, nbrs) in enumerate(zip(tri.simplices.tolist(), tri.neighbors.tolist())):
        x, det = spheres[si]
        for k, other in enumerate(nbrs):                     # the apex across facet k is not on this sphere
            if other < 0:
                continue
            apex = [q for q in tri.simplices[other].tolist() if q not in s]
            assert len(apex) == 1
            d = tuple(2 * det * (a - b) - c for a, b, c in zip(Pl[apex[0]], Pl[s[0]], x))
            assert dot(d, d) != dot(x, x), "five cospherical points: not in general position"
    count, apex_of = {}, {}
    vol6 = 0
    for s, keep in zip(tri.simplices.tolist(), kept):
        if not keep:
            continue
        vol6 += abs(circumsphere(*(Pl[q] for q in s))[1])
        for q in range(4):
            f = tuple(sorted(s[:q] + s[q + 1:]))
            count[f] = count.get(f, 0) + 1
            apex_of[f] = s[q]
    rows = []
    for (i, j, k), c in count.items():
        if c != 1:
            continue
        e1, e2, ed = (tuple(a - b for a, b in zip(Pl[q], Pl[i])) for q in (j, k, apex_of[(i, j, k)]))
        side = dot(cross(e1, e2), ed)
        assert side != 0
        rows.append((i, j, k, REGULAR) if side < 0 else (i, k, j, REGULAR))
    return rows, vol6


def delaunay(P, rho2, seg_start=None):
    """(regular rows int32 [R,4] ascending, vol6 per segment from the kept tetrahedra)."""
    P = np.asarray(P, dtype=np.int64).reshape(-1, 3)
    rows, vol6 = [], []
    for lo, hi in _segments(len(P), seg_start):
        seg_rows, v = delaunay_segment(P[lo:hi], rho2)
        rows += [(a + lo, b + lo, c + lo, kind) for a, b, c, kind in seg_rows]
        vol6.append(v)
    return np.array(sorted(rows), np.int32).reshape(-1, 4), vol6


# ---- fixtures ------------------------------------------------------------------------------------

# seed, n, ext, rho2 -> regular rows, singular rows, six-volume: the CPU trial the contract was settled on
TABLE = {
    (0, 70, 100, 900): (112, 1, 2839594),
    (1, 70, 100, 900): (112, 2, 2032942),
    (2, 70, 100, 900): (108, 1, 2549488),
    (3, 70, 100, 900): (104, 1, 2751862),
    (9, 60, 64, 400): (116, 1, 562894),
    (10, 80, 128, 2500): (100, 0, 6077995),
}


def table_cloud(seed, n, ext):
    return np.unique(np.random.default_rng(seed).integers(0, ext, (n, 3)), axis=0).astype(np.int32)


@functools.lru_cache(maxsize=None)
def table_reference(key):
    seed, n, ext, rho2 = key
    return brute(table_cloud(seed, n, ext), rho2)


def regular_only(ref):
    rows, vol6, _ = ref
    return rows[rows[:, 3] == REGULAR], vol6


R2_SPHERE = 1000 * 1000


@functools.lru_cache(maxsize=None)
def lattice_sphere(r2=R2_SPHERE):
    """Every integer point of x^2 + y^2 + z^2 = r2, in lexicographic order (750 of them for 10^6)."""
    r = math.isqrt(r2)
    out = []
    for x in range(-r, r + 1):
        for y in range(-r, r + 1):
            rest = r2 - x * x - y * y
            if rest < 0:
                continue
            z = math.isqrt(rest)
            if z * z == rest:
                out += [(x, y, z), (x, y, -z)] if z else [(x, y, 0)]
    return np.array(sorted(out), np.int32)


@functools.lru_cache(maxsize=None)
def sphere_points(n=300, seed=4):
    """n points EXACTLY on the sphere of radius 1000 units about (1000, 1000, 1000), shuffled: rounding a random
    direction would leave near-cocircular quadruples as sliver tetrahedra of any circumradius; these are exactly
    cospherical (every tetrahedron has circumradius 1000) and, being lattice points, rich in exactly cocircular
    polygons, which the fan rule must cut into triangles."""
    all_ = lattice_sphere()
    pick = np.random.default_rng(seed).permutation(len(all_))[:n]
    return all_[pick] + 1000


def tie_lattice(pitch, perm_seed=None, shift=(0, 0, 0)):
    """The 27 sites of a 3^3 box at the given pitch, permuted and translated on request."""
    g = np.stack(np.meshgrid(*(np.arange(3),) * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64) * pitch
    if perm_seed is not None:
        g = g[np.random.default_rng(perm_seed).permutation(len(g))]
    return (g + np.asarray(shift, dtype=np.int64)).astype(np.int32)


def tie_radii(pitch):
    """rho^2 at which cube corners sit exactly on balls: the circumradius of a cell (3 pitch^2 / 4, rounded
    up) and of the whole box."""
    return (-(-3 * pitch * pitch // 4), 3 * pitch * pitch)


def cube_corners(edge=1000):
    """The eight corners of a cube, shuffled."""
    g = np.array([[(k >> d) & 1 for d in range(3)] for k in range(8)], np.int32) * edge
    return g[np.random.default_rng(8).permutation(8)]


def cube_rho2(edge=1000):
    return 3 * (edge // 2) ** 2


def cospherical_set(n=40):
    """n of the lattice points of the sphere of radius 1000: at alpha = 1000 one ball of EVERY triple is that
    sphere, empty, with every other point exactly on it."""
    return np.ascontiguousarray(lattice_sphere()[::19][:n]) + 1000


@functools.lru_cache(maxsize=None)
def solid_cloud(n=400, seed=12):
    """(points float64 [n,3] in the unit cube on the lattice of pitch 2^-12, alpha, that pitch): a solid blob at
    alpha = 0.3, a little over two mean spacings."""
    q = 2.0 ** -12
    ijk = np.unique(np.random.default_rng(seed).integers(0, 4096, (n, 3)), axis=0)
    ijk = ijk[np.random.default_rng(seed + 1).permutation(len(ijk))]
    return ijk.astype(np.float64) * q, 0.3, q


def tie_census(P, rho2):
    """(coplanar, off-plane) ties over all candidate triples and all other points, both balls."""
    Pl = as_ints(P)
    n = len(Pl)
    coplanar = off = 0
    for i in range(n):
        for j in range(i + 1, n):
            for k in range(j + 1, n):
                for b, c in ((j, k), (k, j)):
                    t = setup(Pl[i], Pl[b], Pl[c], rho2)
                    if t is None:
                        break
                    for p in range(n):
                        if p in (i, j, k):
                            continue
                        u = tuple(x - y for x, y in zip(Pl[p], Pl[i]))
                        if dot(u, u) > 4 * rho2:
                            continue
                        w = classify(t, u)
                        coplanar += w == TIE_COPLANAR
                        off += w == TIE_OFF_PLANE
    return coplanar, off


@functools.lru_cache(maxsize=None)
def nested_shells(n_outer=1900, n_inner=1100, rho=300, seed=21):
    """About 3 000 points in general position FILLING two nested shells (radii 3.0 to 3.1 rho and 0.6 to 0.95 rho)
    with a gap wider than a ball between them and an empty core: four grid cells of edge 2 rho + 1 per axis,
    cells with far more points than one work item's slice, empty cells, stencils that reach the border, and,
    the inner shell being narrower than 2 rho, more neighbours within 2 rho of each of its points than one LDS
    chunk holds."""
    rng = np.random.default_rng(seed)
    out = []
    for n, lo, hi in ((n_outer, 3.0 * rho, 3.1 * rho), (n_inner, 0.6 * rho, 0.95 * rho)):
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = rng.uniform(lo ** 3, hi ** 3, n) ** (1.0 / 3.0)
        out.append(d * r[:, None])
    P = np.rint(np.concatenate(out) + rng.uniform(-0.4, 0.4, (n_outer + n_inner, 3))).astype(np.int64)
    P -= P.min(axis=0)
    first = np.sort(np.unique(P, axis=0, return_index=True)[1])
    return P[first].astype(np.int32), rho * rho


@functools.lru_cache(maxsize=None)
def nested_shells_reference():
    P, rho2 = nested_shells()
    return delaunay(P, rho2)


def geometric_set(P, rows):
    """The rows as a set of oriented geometric triangles, free of the points' numbering: each rotated so that
    its lexicographically smallest vertex comes first."""
    P = np.asarray(P, dtype=np.int64)
    out = set()
    for a, b, c, kind in np.asarray(rows).tolist():
        v = [tuple(P[a].tolist()), tuple(P[b].tolist()), tuple(P[c].tolist())]
        if kind == SINGULAR:
            out.add((tuple(sorted(v)), kind))
            continue
        k = v.index(min(v))
        out.add((tuple(v[k:] + v[:k]), kind))
    return out
