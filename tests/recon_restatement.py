"""The ball-pivoting contract of pyqsm_ball_pivot restated on the CPU, twice.

``brute``      the definition: every triple of points with edges of at most 2 rho, a circumradius of at
               most rho and agreeing normals, against EVERY other point of the cloud, with the tie rule.
``delaunay``   an independent route for clouds in general position: the facets of scipy's Delaunay
               triangulation, each tested against the apexes of its (at most) two tetrahedra only.

Every decision is an evaluation in Python integers (``setup`` / ``classify``). ``brute`` first orders
its work with fp64: a point whose fp64 value of N - sqrt(H) D is beyond 2^-30 of the magnitude of its
terms (2^18 times the rounding error of that evaluation) is taken at that sign; everything closer,
hence every tie, is classified by the integers. Both routes share ``combine``, the rule for several radii.
"""
import functools
import math

import numpy as np

INSIDE, OUTSIDE, TIE_COPLANAR, TIE_OFF_PLANE = 1, 0, 2, 3


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def setup(a, b, c, rho2):
    """The exact quantities of the oriented candidate (a, b, c), tuples of Python integers, or None
    when it is none."""
    e1 = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
    e2 = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
    e3 = (e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2])
    l1, l2, l3 = dot(e1, e1), dot(e2, e2), dot(e3, e3)
    if max(l1, l2, l3) > 4 * rho2:
        return None
    n = cross(e1, e2)
    n2 = dot(n, n)
    if n2 == 0:
        return None
    H = 4 * rho2 * n2 - l1 * l2 * l3
    if H < 0:
        return None
    x, y = cross(e2, n), cross(n, e1)
    w = (l1 * x[0] + l2 * y[0], l1 * x[1] + l2 * y[1], l1 * x[2] + l2 * y[2])
    return dict(e1=e1, e2=e2, n=n, n2=n2, H=H, w=w)


def classify(t, u):
    D = dot(t["n"], u)
    N = dot(u, u) * t["n2"] - dot(t["w"], u)
    if D == 0:
        return INSIDE if N < 0 else TIE_COPLANAR if N == 0 else OUTSIDE
    if D > 0 and N < 0:
        return INSIDE
    if D < 0 and N > 0:
        return OUTSIDE
    lhs, rhs = N * N, D * D * t["H"]
    if lhs == rhs:
        return TIE_OFF_PLANE
    if D > 0:
        return INSIDE if lhs < rhs else OUTSIDE
    return INSIDE if lhs > rhs else OUTSIDE


def beyond_bc(t, u):
    f = tuple(t["e2"][k] - t["e1"][k] for k in range(3))
    g = tuple(u[k] - t["e1"][k] for k in range(3))
    return dot(cross(f, g), t["n"]) < 0


def orient(P, Nr, i, j, k, rho2):
    """(a, b, c, quantities) of the triple i < j < k oriented by its normals, or None. P, Nr: lists
    of tuples of Python integers (``as_ints``)."""
    t = setup(P[i], P[j], P[k], rho2)
    if t is None:
        return None
    d = [dot(t["n"], Nr[q]) for q in (i, j, k)]
    if all(v > 0 for v in d):
        return i, j, k, t
    if all(v < 0 for v in d):
        return i, k, j, setup(P[i], P[k], P[j], rho2)
    return None


def as_ints(A):
    return [tuple(int(v) for v in row) for row in np.asarray(A).tolist()]


def exposed_brute(P, Nr, rho2, allowed=None):
    """{(a, b, c)} exposed at rho^2 with the tie rule, and those of them kept with an off-plane tie.
    ``allowed``: bool [n], vertices a triangle may use (the others still block)."""
    P = np.asarray(P, dtype=np.int64)
    n = len(P)
    ok = np.ones(n, bool) if allowed is None else np.asarray(allowed, bool)
    Pf, Ni = P.astype(np.float64), np.asarray(Nr, dtype=np.int64)
    Pl, Nl = as_ints(P), as_ints(Nr)
    d2 = ((P[:, None, :] - P[None, :, :]) ** 2).sum(axis=2)
    near = d2 <= 4 * rho2
    out, unresolved = set(), set()
    for i in range(n):
        if not ok[i]:
            continue
        nb = [j for j in np.nonzero(near[i])[0].tolist() if j > i and ok[j]]
        if len(nb) < 2:
            continue
        # pairs j < k of neighbours; int64 and fp64 discard only what is clearly no candidate (the third
        # edge, the side of the normals: exact; a circumradius above rho by more than 1e-9: fp64), the
        # Python integers of orient() decide the rest
        x, y = np.triu_indices(len(nb), 1)
        J, K = np.asarray(nb)[x], np.asarray(nb)[y]
        e1, e2 = P[J] - P[i], P[K] - P[i]
        nn = np.cross(e1, e2)
        l1, l2, l3 = (e1 * e1).sum(axis=1), (e2 * e2).sum(axis=1), ((e2 - e1) ** 2).sum(axis=1)
        n2 = (nn * nn).sum(axis=1)
        big, small = 4.0 * rho2 * n2.astype(np.float64), l1.astype(np.float64) * l2 * l3
        da, db, dc = nn @ Ni[i], (nn * Ni[J]).sum(axis=1), (nn * Ni[K]).sum(axis=1)
        sides = ((da > 0) & (db > 0) & (dc > 0)) | ((da < 0) & (db < 0) & (dc < 0))
        keep = near[J, K] & (n2 > 0) & sides & (big - small >= -1e-9 * small)
        cands = [got for got in (orient(Pl, Nl, i, j, k, rho2) for j, k in zip(J[keep].tolist(), K[keep].tolist()))
                 if got is not None]
        if not cands:
            continue
        # fp64 only to order the work (module docstring): one column per candidate, one row per point
        U = Pf - Pf[i]
        nf = np.array([t["n"] for *_, t in cands], np.float64).T
        wf = np.array([[float(v) for v in t["w"]] for *_, t in cands]).T
        D = U @ nf
        t0 = (U * U).sum(axis=1)[:, None] * np.array([float(t["n2"]) for *_, t in cands])
        rhs = D * np.array([math.sqrt(float(t["H"])) for *_, t in cands])
        val = t0 - U @ wf - rhs
        scale = (t0 + np.abs(U) @ np.abs(wf) + np.abs(rhs)) * 2.0 ** -30
        for col, (a, b, c, t) in enumerate(cands):
            v, sc = val[:, col], scale[:, col]
            v[[a, b, c]] = np.inf
            clearly = np.nonzero(v < -sc)[0]
            if len(clearly):
                p = int(clearly[np.argmin(v[clearly])])
                assert classify(t, tuple(x - y for x, y in zip(Pl[p], Pl[a]))) == INSIDE
                continue
            blocked, off_plane, drop = False, False, False
            for p in np.nonzero(np.abs(v) <= sc)[0].tolist():
                u = tuple(x - y for x, y in zip(Pl[p], Pl[a]))
                w = classify(t, u)
                if w == INSIDE:
                    blocked = True
                    break
                if w == TIE_OFF_PLANE:
                    off_plane = True
                elif w == TIE_COPLANAR and (p < a or beyond_bc(t, u)):
                    drop = True
            if blocked or (drop and not off_plane):
                continue
            out.add((a, b, c))
            if off_plane:
                unresolved.add((a, b, c))
    return out, unresolved


def exposed_delaunay(P, Nr, rho2, allowed=None):
    """The same set for a cloud in general position (no point exactly on the ball of a candidate:
    asserted), from the facets of the Delaunay triangulation and their apexes."""
    from scipy.spatial import Delaunay
    P = np.asarray(P, dtype=np.int64)
    ok = np.ones(len(P), bool) if allowed is None else np.asarray(allowed, bool)
    Pl, Nl = as_ints(P), as_ints(Nr)
    tri = Delaunay(P.astype(np.float64))
    assert tri.coplanar.size == 0, "qhull left points out (coincident points?): not in general position"
    apexes = {}
    for s in tri.simplices.tolist():
        for q in range(4):
            f = tuple(sorted(s[:q] + s[q + 1:]))
            apexes.setdefault(f, []).append(s[q])
    out = set()
    for (i, j, k), ap in apexes.items():
        if not (ok[i] and ok[j] and ok[k]):
            continue
        got = orient(Pl, Nl, i, j, k, rho2)
        if got is None:
            continue
        a, b, c, t = got
        where = [classify(t, tuple(x - y for x, y in zip(Pl[p], Pl[a]))) for p in ap]
        assert TIE_COPLANAR not in where and TIE_OFF_PLANE not in where, "not in general position"
        if INSIDE not in where:
            out.add((a, b, c))
    return out, set()


def inner_vertices(tris, n):
    """bool [n]: has triangles, and every incident half-edge has its reverse."""
    half = set()
    for a, b, c in tris:
        half.update(((a, b), (b, c), (c, a)))
    has, open_ = np.zeros(n, bool), np.zeros(n, bool)
    for u, v in half:
        has[u] = has[v] = True
        if (v, u) not in half:
            open_[u] = open_[v] = True
    return has & ~open_, half


def combine(P, Nr, rho2_list, exposed):
    """The rule for several radii over ``exposed(P, Nr, rho2, allowed)``: (triangles int32 [T,3]
    sorted by (a, b, c), levels int32 [T], unresolved ties)."""
    n = len(P)
    level_of, unresolved = {}, 0
    for lv, rho2 in enumerate(sorted(int(r) for r in rho2_list)):
        if lv == 0:
            tris, unres = exposed(P, Nr, rho2, None)
        else:
            inner, half = inner_vertices(level_of, n)
            tris, unres = exposed(P, Nr, rho2, ~inner)
            tris = {t for t in tris if (t[0], t[1]) not in half and (t[1], t[2]) not in half
                    and (t[2], t[0]) not in half}
        for t in tris:
            level_of[t] = lv
        unresolved += len(unres & tris)
    keys = sorted(level_of)
    T = np.array(keys, np.int32).reshape(-1, 3)
    return T, np.array([level_of[k] for k in keys], np.int32), unresolved


def brute(P, Nr, rho2_list):
    return combine(P, Nr, rho2_list, exposed_brute)


def delaunay(P, Nr, rho2_list):
    return combine(P, Nr, rho2_list, exposed_delaunay)


# ---- what the tests ask of a result ------------------------------------------------------------

def half_edges(T):
    T = np.asarray(T)
    return [(int(t[k]), int(t[(k + 1) % 3])) for t in T for k in range(3)]


def open_half_edges(T):
    """The half-edges without their reverse."""
    h = half_edges(T)
    s = set(h)
    return [e for e in h if (e[1], e[0]) not in s]


def loops(edges):
    """Number of closed loops the given directed edges form (every vertex once in, once out)."""
    nxt = {}
    for u, v in edges:
        assert u not in nxt
        nxt[u] = v
    seen, count = set(), 0
    for u in nxt:
        if u in seen:
            continue
        count += 1
        while u not in seen:
            seen.add(u)
            u = nxt[u]
    return count


def twice_area(P, T):
    P = np.asarray(P, dtype=np.int64)
    T = np.asarray(T)
    n = np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]])
    return np.sqrt((n.astype(np.float64) ** 2).sum(axis=1)).sum()


# ---- fixtures ------------------------------------------------------------------------------------

R_SPHERE = 2048
RHO2_SMALL = int(math.floor((0.35 * R_SPHERE) ** 2))
RHO2_LARGE = int(math.floor((0.8 * R_SPHERE) ** 2))


def snap(unit):
    return np.rint(np.asarray(unit) * (1 << 14)).astype(np.int16)


def _sphere_dirs(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def sphere(n=400, seed=5):
    """n random points on a sphere of R_SPHERE lattice units, outward normals; rho = 0.35 R."""
    d = _sphere_dirs(n, seed)
    return np.rint(d * R_SPHERE).astype(np.int32) + R_SPHERE, snap(d), (RHO2_SMALL,)


@functools.lru_cache(maxsize=None)
def fibonacci_sphere(n=400):
    """n evenly spread points on the same sphere (a golden-angle spiral): float64 [n,3] lattice values."""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    d = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    return np.rint(d * R_SPHERE) + R_SPHERE


@functools.lru_cache(maxsize=None)
def holed_sphere(n=500, seed=9):
    """The same recipe without the cap within 0.6 rad of the +z pole; radii 0.35 R and 0.8 R."""
    d = _sphere_dirs(n, seed)
    d = d[np.arccos(np.clip(d[:, 2], -1, 1)) > 0.6]
    return np.rint(d * R_SPHERE).astype(np.int32) + R_SPHERE, snap(d), (RHO2_SMALL, RHO2_LARGE)


@functools.lru_cache(maxsize=None)
def plane_grid(m=7, pitch=100, seed=3):
    """A shuffled m x m grid in the plane z = 0, normals +z; rho = 150 (every square is cocircular)."""
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), axis=-1).reshape(-1, 2) * pitch
    P = np.concatenate([g, np.zeros((m * m, 1), np.int64)], axis=1).astype(np.int32)
    P = P[np.random.default_rng(seed).permutation(m * m)]
    Nr = np.tile(np.array([0, 0, 1 << 14], np.int16), (m * m, 1))
    return P, Nr, (150 * 150,)


@functools.lru_cache(maxsize=None)
def nested_surfaces(n_outer=1800, n_inner=1200, rho=300, seed=11):
    """Two nested bumpy spheres of radii about 3 rho (normals outward) and 2.2 rho (normals inward):
    the whole cloud spans four cells of edge 2 rho + 1 per axis, so the stencil of a middle cell holds
    most of the cloud (more than one LDS chunk), cells hold far more points than one block's slice,
    and the cells around the centre are empty."""
    out = []
    for n, radius, sign, s in ((n_outer, 3.0 * rho, 1.0, seed), (n_inner, 2.2 * rho, -1.0, seed + 1)):
        d = _sphere_dirs(n, s)
        bump = 1.0 + 0.04 * np.sin(3.0 * np.arctan2(d[:, 1], d[:, 0])) * np.cos(2.0 * np.arccos(np.clip(d[:, 2], -1, 1)))
        out.append((d * (radius * bump)[:, None], sign * d))
    pts = np.concatenate([o[0] for o in out])
    P = np.rint(pts).astype(np.int32)
    P -= P.min(axis=0)
    first = np.sort(np.unique(P, axis=0, return_index=True)[1])      # points that snap to one node: the first stays
    return P[first], snap(np.concatenate([o[1] for o in out]))[first], (rho * rho,)


def cospherical_five():
    """Five corners of a cube of edge 1000, normals +z, rho the cube's circumradius: the ball on the
    upper side of the triple in the plane z = 0 is the cube's circumsphere, and the two corners above
    lie exactly on it, off the triple's plane."""
    P = np.array([[0, 0, 0], [1000, 0, 0], [0, 1000, 0], [0, 0, 1000], [1000, 1000, 1000]], np.int32)
    return P, np.tile(np.array([0, 0, 1 << 14], np.int16), (5, 1)), (3 * 500 * 500,)


@functools.lru_cache(maxsize=None)
def holed_sphere_late():
    """The holed sphere with two radii in front (2 and 3 lattice units, where the points are hundreds
    apart) at which no ball finds three points: the first two levels are empty."""
    P, Nr, rho2 = holed_sphere()
    return P, Nr, (4, 9) + rho2


GENERAL_POSITION = {"sphere": sphere, "holed_sphere": holed_sphere, "holed_sphere_late": holed_sphere_late}
