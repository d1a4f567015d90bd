"""Inputs shared by tests/test_recon_host.py (the CPU proof that every input has the property its GPU test
depends on) and tests/test_gpu_recon.py (pyqsm_ball_pivot against tests/recon_restatement.py::brute, the
only reference). What they are after is the hand-over between the fp64 filter of the ball test and the
integer predicate behind it (recon_exact.hpp: recon_filter, recon_classify): random clouds
never come near it, lattice clouds sit on it.

  tie_lattice(seed, m, pitch, radii, flat)   36 points on the sites of an m^3 box, three of them copies of
                        others, five normals exactly along an axis; TIE_TABLE holds the pitches and radii.
  lattice_sphere(r2, n, inward)   n integer points of the sphere |x|^2 = r2, rho^2 = r2: with inward
                        normals every triple rests on the sphere itself and every other point ties.
  rectangle_h0(height)  a 60 x 80 rectangle at rho = 50 (H = 0: the ball's centre in the plane) and a
                        fifth point `height` above the centre: 50 ties off the plane, 49 is inside.
  dense_box()           1 100 of the 12^3 sites at pitch 1, ten of them coincident: one stencil holds the
                        whole cloud (more than one LDS chunk), every cell more points than a block's slice.
  far_apart(low)        two tie lattices 2^31 - 1 lattice units apart along x, from `low`.

Every case is (P int32 [n,3], Nr int16 [n,3], rho2 tuple), built once per process from fixed seeds and
read-only; reference() keeps brute's answer so that tests which share an input share it."""
import functools

import numpy as np

from tests import recon_restatement as R

NORMAL_SCALE = 1 << 14                       # hip.RECON_NORMAL_SCALE (test_recon_host.py holds them equal)
R2_CUBE = 3 * 1182 * 1182                    # 4 191 372: the circumsphere of a cube of edge 2 * 1182
R2_TOP = 4194301                             # three below the bound of 2^22
SPHERE_POINTS = {R2_CUBE: 6368, R2_TOP: 14376}
TIE_TABLE = ((1, (1, 2, 3)), (7, (2 * 49, 3 * 49)), (500, (2 * 500 ** 2, 5 * 500 ** 2)),
             (1182, (2 * 1182 ** 2, R2_CUBE)))
TIE_SEEDS = (1, 2)
TIE_SIZES = (3, 4, 5)
N_TIE_LATTICE = 36


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def snap(v):
    """int16 normals of the directions v (not necessarily unit), as hip.snap_normals gives them."""
    v = np.asarray(v, np.float64)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.rint(v * NORMAL_SCALE).astype(np.int16)


@functools.lru_cache(maxsize=None)
def tie_lattice(seed, m, pitch, radii, flat):
    rng = np.random.default_rng([seed, m, pitch, int(flat)])
    n = N_TIE_LATTICE
    sites = rng.choice(m ** 3, n, replace=m ** 3 < n)
    S = np.stack([sites % m, (sites // m) % m, sites // (m * m)], axis=1).astype(np.int64)
    if flat:
        S[: n // 2, 2] = 0                                    # half the cloud in one plane
    who = rng.permutation(n)[:6]
    S[who[:3]] = S[who[3:]]                                   # coincident points
    d = S - (m - 1) / 2.0 + rng.normal(0.0, 0.3, (n, 3))      # radial, jittered in site units
    d[np.linalg.norm(d, axis=1) < 1e-6] = (0.0, 0.0, 1.0)
    axes = rng.permutation(n)[:5]
    d[axes] = 0.0
    d[axes, rng.integers(0, 3, 5)] = rng.choice([-1.0, 1.0], 5)   # exactly perpendicular to lattice directions
    offset = rng.integers(-(1 << 20), (1 << 20) + 1, 3)
    return frozen((S * pitch + offset).astype(np.int32)), frozen(snap(d)), tuple(radii)


def tie_lattice_keys():
    """The 48 cases of the table: (seed, m, pitch, radii, flat)."""
    return [(seed, m, pitch, radii, flat) for pitch, radii in TIE_TABLE for m in TIE_SIZES for seed in TIE_SEEDS
            for flat in (False, True)]


@functools.lru_cache(maxsize=None)
def sphere_points(r2):
    """Every integer point of the sphere x^2 + y^2 + z^2 = r2, int64 [k,3], in a fixed order."""
    r = int(np.floor(np.sqrt(r2)))
    y = np.arange(-r, r + 1, dtype=np.int64)
    rows = []
    for x in range(-r, r + 1):
        rest = r2 - x * x - y * y
        ok = rest >= 0
        z = np.rint(np.sqrt(rest[ok].astype(np.float64))).astype(np.int64)   # exact: rest < 2^23
        hit = z * z == rest[ok]
        for sign in (1, -1):
            keep = hit & ((z > 0) | (sign > 0))
            rows.append(np.stack([np.full(keep.sum(), x, np.int64), y[ok][keep], sign * z[keep]], axis=1))
    return frozen(np.concatenate(rows))


@functools.lru_cache(maxsize=None)
def _sphere_choice(r2, n, seed):
    rng = np.random.default_rng([seed, r2, n])
    Q = sphere_points(r2)
    return Q[rng.choice(len(Q), n, replace=False)], rng.integers(-(1 << 20), (1 << 20) + 1, 3)


def lattice_sphere_centre(r2, n=18, seed=0):
    return _sphere_choice(r2, n, seed)[1]


@functools.lru_cache(maxsize=None)
def lattice_sphere(r2, n=18, inward=True, seed=0):
    Q, centre = _sphere_choice(r2, n, seed)
    return frozen((Q + centre).astype(np.int32)), frozen(snap(-Q if inward else Q)), (r2,)


@functools.lru_cache(maxsize=None)
def rectangle_h0(height):
    P = np.array([[0, 0, 0], [60, 0, 0], [60, 80, 0], [0, 80, 0], [30, 40, height]], np.int32)
    return frozen(P), frozen(np.tile(np.array([0, 0, NORMAL_SCALE], np.int16), (5, 1))), (2500,)


@functools.lru_cache(maxsize=None)
def dense_box(seed=4, m=12, n=1100):
    rng = np.random.default_rng(seed)
    sites = rng.choice(m ** 3, n, replace=False)
    S = np.stack([sites % m, (sites // m) % m, sites // (m * m)], axis=1).astype(np.int64)
    who = rng.permutation(n)[:20]
    S[who[:10]] = S[who[10:]]
    return frozen(S.astype(np.int32)), frozen(snap(S - (m - 1) / 2.0)), (1, 2)


FAR_HALVES = ((1, 4, 1182, TIE_TABLE[3][1], False), (2, 5, 1182, TIE_TABLE[3][1], True))


@functools.lru_cache(maxsize=None)
def far_apart(low):
    """The two tie lattices of FAR_HALVES, each moved along x only: the cloud's x range is exactly
    [low, low + 2^31 - 1], the largest admitted span (y and z differ by 2^21 at most, so brute's int64
    squared distances stay below 2^63)."""
    (P0, N0, rho2), (P1, N1, _) = (tie_lattice(*k) for k in FAR_HALVES)
    A, B = P0.astype(np.int64), P1.astype(np.int64)
    A[:, 0] += low - A[:, 0].min()
    B[:, 0] += low + (1 << 31) - 1 - B[:, 0].max()
    return frozen(np.concatenate([A, B]).astype(np.int32)), frozen(np.concatenate([N0, N1])), rho2


FAR_LOWS = (-(1 << 30), -(1 << 31))

CASES = {"tie_lattice": tie_lattice, "lattice_sphere": lattice_sphere, "rectangle_h0": rectangle_h0,
         "dense_box": dense_box, "far_apart": far_apart}


def brute_with_census(P, Nr, rho2):
    """brute's answer, and how many points it found tied in the plane and off it over the candidates no
    point blocks: what makes a result depend on the numbering of the points."""
    seen = {R.TIE_COPLANAR: 0, R.TIE_OFF_PLANE: 0, R.INSIDE: 0, R.OUTSIDE: 0}
    classify = R.classify

    def counting(t, u):
        w = classify(t, u)
        seen[w] += 1
        return w

    R.classify = counting                    # exposed_brute looks the name up when it runs
    try:
        T, lv, unresolved = R.brute(P, Nr, rho2)
    finally:
        R.classify = classify
    return (frozen(T), frozen(lv), unresolved), (seen[R.TIE_COPLANAR], seen[R.TIE_OFF_PLANE])


@functools.lru_cache(maxsize=None)
def _solved(name, *args):
    return brute_with_census(*CASES[name](*args))


def reference(name, *args):
    """brute's (triangles, levels, unresolved ties) of CASES[name](*args), kept."""
    return _solved(name, *args)[0]


def census(name, *args):
    """(ties in the plane, ties off it) of the same run."""
    return _solved(name, *args)[1]


def far_apart_from_halves():
    """What far_apart must give: the halves by themselves, the second renumbered behind the first."""
    (T0, l0, u0), (T1, l1, u1) = (reference("tie_lattice", *k) for k in FAR_HALVES)
    return np.concatenate([T0, T1 + N_TIE_LATTICE]), np.concatenate([l0, l1]), u0 + u1


def triangle_cap(n):
    return 8 * n + 1024


def perpendicular_normals(P, Nr, rho2):
    """How many (candidate triple at rho2, vertex of it) have a vertex normal exactly perpendicular to the
    triangle's normal: such a triple has no orientation and is no candidate for the ball."""
    P, Nr = np.asarray(P, np.int64), np.asarray(Nr, np.int64)
    n = len(P)
    i, j, k = (np.array(v) for v in zip(*[(a, b, c) for a in range(n) for b in range(a + 1, n) for c in range(b + 1, n)]))
    e1, e2 = P[j] - P[i], P[k] - P[i]
    nn = np.cross(e1, e2)
    short = np.maximum.reduce([(e1 * e1).sum(axis=1), (e2 * e2).sum(axis=1), ((e2 - e1) ** 2).sum(axis=1)]) <= 4 * rho2
    dots = np.stack([(nn * Nr[v]).sum(axis=1) for v in (i, j, k)], axis=1)
    Pl, count = R.as_ints(P), 0
    for t in np.nonzero(short & (nn != 0).any(axis=1) & (dots == 0).any(axis=1))[0].tolist():
        if R.setup(Pl[i[t]], Pl[j[t]], Pl[k[t]], rho2) is not None:      # the circumradius, in Python integers
            count += int((dots[t] == 0).sum())
    return count
