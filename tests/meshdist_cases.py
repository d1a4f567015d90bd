"""Input families and comparison helpers shared by tests/test_meshdist_host.py (the mirror oracle on
the CPU) and tests/test_gpu_meshdist.py (the HIP kernel): point-to-mesh distance, closest triangle
and inside/outside sign against the INDEPENDENT fp64 references of oracle/meshdist_f64.c.

Bounds (none of them fitted to what the code under test returns):
  distance  |d - d64| <= T_RTOL * max(d64, NEAR * diag), diag = bounding-box diagonal of the vertices.
            T_RTOL and NEAR are those of tests/test_gpu_rays_f64.py (north_star's 1e-5; an fp32
            evaluation resolves a distance no better than ~eps32 * |coordinates| however small it is).
  triangle  the fp64 distance from the query to the REPORTED triangle is <= d64 + the same bound
            (ids need not be equal: triangles that share an edge tie).
  sign      on every query further than SIGN_MIN * diag from the surface (fp64):
            signed distance < 0 exactly where |winding number| > 0.5.
Every family is built once per process (seeds fixed here), coordinates cast to float32 first; the
fp64 references are computed once per family and shared."""
import functools

import numpy as np

import oracle
from pyqsm_amd import synth

T_RTOL = 1e-5
NEAR = 0.05
SIGN_MIN = 1e-4
MAX_EXCLUDED = 0.02          # share of a sphere / random query set that may lie within SIGN_MIN * diag

THIN_H = (1e-2, 1e-4, 1e-5, 3e-6, 1e-6, 1e-7, 0.0)
THIN_BASE = (1.0, 0.05)

CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
CUBE_T = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7],
                   [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def diagonal(verts):
    v = np.asarray(verts, dtype=np.float64)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


# ------------------------------------------------------------------ meshes

def _perp(u, rng):
    """a unit vector across each row of u"""
    r = rng.normal(size=u.shape)
    r -= (r * u).sum(1, keepdims=True) * u
    return r / np.linalg.norm(r, axis=1, keepdims=True)


def thin_triangles(n, base, h, seed):
    """n triangles of base length `base`; the third vertex at a random point of the base plus
    h * base across it. With h at or below fp32 resolution the three vertices are collinear up to
    the rounding of their coordinates (an edge-midpoint vertex, a T-junction repair, a sliver)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (n, 3))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    b = a + base * u
    c = a + rng.uniform(0, 1, (n, 1)) * base * u + h * base * _perp(u, rng)
    verts = _f32(np.stack([a, b, c], axis=1).reshape(-1, 3))
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def single_thin_triangle(h):
    a, b = np.zeros(3), np.array([1.0, 0.3, 0.2])
    u = (b / np.linalg.norm(b))[None]
    c = 0.5 * (a + b) + h * np.linalg.norm(b) * _perp(u, np.random.default_rng(17))[0]
    return _f32([a, b, c]), np.array([[0, 1, 2]], np.int32)


def degenerate_triangles(seed=23):
    """Exactly degenerate triangles: integer-coordinate collinear ones (every product exact),
    repeated vertices in each position, all three indices equal."""
    rng = np.random.default_rng(seed)
    n = 40
    a = rng.integers(-3, 4, (n, 3))
    d = rng.integers(-2, 3, (n, 3))
    d[(d == 0).all(1)] = (1, 0, 0)
    k1, k2 = rng.integers(-3, 4, (n, 1)), rng.integers(-3, 4, (n, 1))
    verts = _f32(np.stack([a, a + k1 * d, a + k2 * d], axis=1).reshape(-1, 3))
    col = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    i, j = col[:, 0], col[:, 1]
    rep = np.concatenate([np.stack(s, 1) for s in ((i, j, j), (i, i, j), (i, j, i), (i, i, i))])
    return verts, np.concatenate([col, rep]).astype(np.int32)


def join(*meshes):
    vs, ts, off = [], [], 0
    for v, t in meshes:
        vs.append(v)
        ts.append(t + off)
        off += len(v)
    return _f32(np.concatenate(vs)), np.concatenate(ts).astype(np.int32)


def uv_sphere(n_lat, n_lon, radius=1.0, centre=(0, 0, 0), rotation=None):
    """Closed sphere, outward orientation: 2 poles + (n_lat - 1) rings of n_lon vertices."""
    th = np.pi * np.arange(1, n_lat) / n_lat
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph), np.sin(th)[:, None] * np.sin(ph),
                     np.cos(th)[:, None] * np.ones(n_lon)], axis=-1).reshape(-1, 3)
    v = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * radius
    if rotation is not None:
        v = v @ np.asarray(rotation).T
    south = len(v) - 1
    idx = lambda r, k: 1 + r * n_lon + k % n_lon
    t = []
    for k in range(n_lon):
        t.append((0, idx(0, k), idx(0, k + 1)))
        t.append((south, idx(n_lat - 2, k + 1), idx(n_lat - 2, k)))
        for r in range(n_lat - 2):
            t.append((idx(r, k), idx(r + 1, k), idx(r + 1, k + 1)))
            t.append((idx(r, k), idx(r + 1, k + 1), idx(r, k + 1)))
    return _f32(v + np.asarray(centre, dtype=np.float64)), np.array(t, np.int32)


def fixed_rotation(seed=5):
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q *= np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def l_prism():
    """Closed NON-CONVEX mesh: three unit cubes joined into an L (an L-shaped hexagon in xy,
    extruded over z in [0, 1]); outward orientation, no T-junctions."""
    xy = np.array([(0, 0), (1, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2), (0, 1)], np.float64)
    v = np.concatenate([np.c_[xy, np.zeros(8)], np.c_[xy, np.ones(8)]])
    t = []
    for s in ((0, 1, 4, 7), (1, 2, 3, 4), (7, 4, 5, 6)):          # counter-clockwise unit squares
        a, b, c, d = s
        t += [(a, c, b), (a, d, c)]                                # bottom, normal -z
        t += [(a + 8, b + 8, c + 8), (a + 8, c + 8, d + 8)]        # top, normal +z
    for k in range(8):                                             # sides along the outline
        a, b = k, (k + 1) % 8
        t += [(a, b, b + 8), (a, b + 8, a + 8)]
    return _f32(v), np.array(t, np.int32)


def box_lattice(verts, grid):
    """The lattice `mri` queries: `grid` points per axis spanning the mesh's own bounding box."""
    rng = np.linspace(verts.min(0), verts.max(0), num=grid)
    return _f32(np.stack(np.meshgrid(*rng.T), axis=-1).reshape(-1, 3))


# ------------------------------------------------------------------ distance families

def _canopy():
    return synth.canopy_mesh(600, seed=3, side=0.4)


def _surface_samples(verts, tris):
    """vertices, edge midpoints and face centroids (rounded to fp32: on the surface up to that)"""
    tv = verts[tris].astype(np.float64)
    mid = 0.5 * (tv + np.roll(tv, -1, axis=1))
    return _f32(np.concatenate([tv.reshape(-1, 3), mid.reshape(-1, 3), tv.mean(1)]))


def _family_a():
    v, t = _canopy()
    lo, hi = v.min(0) - 1, v.max(0) + 1
    return v, t, _f32(np.random.default_rng(101).uniform(lo, hi, (4000, 3)))


def _family_b():
    v, t = _canopy()
    rng = np.random.default_rng(102)
    w = rng.dirichlet((1, 1, 1), 4000)
    tv = v[t[rng.integers(0, len(t), 4000)]].astype(np.float64)
    return v, t, _f32((w[:, :, None] * tv).sum(1) + rng.normal(0, 1e-3, (4000, 3)))


def _family_c():
    v, t = _canopy()
    centre = 0.5 * (v.min(0) + v.max(0))
    return v, t, _f32(centre + np.random.default_rng(103).normal(0, 300, (4000, 3)))


def _family_d():
    v, t = synth.canopy_mesh(600, seed=4, side=0.05)
    v = _f32(v + np.float32([500, -300, 100]))
    lo, hi = v.min(0) - 1, v.max(0) + 1
    return v, t, _f32(np.random.default_rng(104).uniform(lo, hi, (4000, 3)))


def _thin(base, h):
    v, t = thin_triangles(300, base, h, seed=31)
    return v, t, _f32(np.random.default_rng(105).uniform(-2, 2, (3000, 3)))


def _thin_single(h):
    v, t = single_thin_triangle(h)
    return v, t, _f32(np.random.default_rng(106).uniform(-1, 2, (5000, 3)))


def _degenerate(mixed):
    v, t = degenerate_triangles()
    if mixed:
        cv, ct = synth.canopy_mesh(100, seed=6, side=1.5)
        cv = _f32((cv - np.float32([0, 0, 9])))
        order = np.random.default_rng(107).permutation(len(t) + len(ct))
        v, t = join((v, t), (cv, ct))
        t = t[order]
    return v, t, _f32(np.random.default_rng(108).uniform(-6, 6, (3000, 3)))


def _on_surface(which):
    if which == "canopy":
        v, t = _canopy()
    elif which == "cube":
        v, t = CUBE_V, CUBE_T
    elif which == "cube-slivers":
        # degenerate triangles lying ON the cube's edges and face diagonals, before, between and
        # after the faces they tie with exactly (distance 0): the lowest index must win either way
        extra = np.array([[0, 1, 1], [0, 3, 0], [4, 4, 4]], np.int32)
        v, t = CUBE_V, np.concatenate([extra[:1], CUBE_T[:6], extra[1:2], CUBE_T[6:], extra[2:]])
    elif which == "thin":
        v, t = join(thin_triangles(150, 1.0, 1e-6, seed=32), thin_triangles(150, 0.05, 0.0, seed=33),
                    thin_triangles(100, 1.0, 1e-2, seed=34))
    else:
        v, t = _degenerate(True)[:2]
    q = _surface_samples(v, t)
    return v, t, q[:5000]


def mixed_mesh():
    """Every kind of triangle in one mesh, shuffled: leaves, slivers above and below fp32
    resolution, exactly degenerate ones."""
    v, t = join(synth.canopy_mesh(200, seed=9, side=0.4), thin_triangles(60, 1.0, 1e-3, seed=35),
                thin_triangles(60, 0.05, 1e-6, seed=36), thin_triangles(60, 1.0, 0.0, seed=37),
                degenerate_triangles())
    return v, t[np.random.default_rng(109).permutation(len(t))]


DISTANCE_FAMILIES = {
    "a-canopy": _family_a,
    "b-near-surface": _family_b,
    "c-far": _family_c,
    "d-small-leaves-off-origin": _family_d,
    **{f"e-thin-base{b:g}-h{h:g}": functools.partial(_thin, b, h) for b in THIN_BASE for h in THIN_H},
    **{f"e-single-h{h:g}": functools.partial(_thin_single, h) for h in THIN_H},
    "f-degenerate-mixed": functools.partial(_degenerate, True),
    "f-degenerate-only": functools.partial(_degenerate, False),
    **{f"g-on-{w}": functools.partial(_on_surface, w) for w in ("canopy", "cube", "cube-slivers", "thin", "degenerate")},
}


@functools.lru_cache(maxsize=None)
def distance_case(name):
    """(verts, tris, queries, d64, p64) — read-only, shared between tests."""
    v, t, q = DISTANCE_FAMILIES[name]()
    d64, p64 = oracle.point_mesh_distance_f64(v, t, q)
    out = (_f32(v), np.ascontiguousarray(t, dtype=np.int32), q, d64, p64)
    for a in out:
        a.setflags(write=False)
    return out


def check_distance(name, dist, prim):
    """Assert the distance and closest-triangle bounds of family `name`; returns the measured
    maximum of |d - d64| / max(d64, NEAR * diag)."""
    v, t, q, d64, _ = distance_case(name)
    dist = np.asarray(dist, dtype=np.float64)
    assert dist.shape == d64.shape and np.isfinite(dist).all(), name
    scale = np.maximum(d64, NEAR * diagonal(v))
    rel = np.abs(dist - d64) / scale
    worst = float(rel.max())
    d_rep = oracle.point_tri_pairs_f64(v, t, q, np.asarray(prim).astype(np.int64))
    excess = float(np.nanmax((d_rep - d64) / scale)) if not np.isnan(d_rep).all() else np.inf
    print(f"{name}: max |d-d64|/max(d64,{NEAR}*diag) = {worst:.3g} over {len(q)} queries; "
          f"reported triangle beyond the minimum by {excess:.3g}")
    assert worst <= T_RTOL, (name, worst, int(rel.argmax()))
    assert not np.isnan(d_rep).any(), (name, "a reported triangle id is outside the mesh")
    assert excess <= T_RTOL, (name, excess)
    return worst


# ------------------------------------------------------------------ sign families

def _random_box(v, pad, n, seed):
    return _f32(np.random.default_rng(seed).uniform(v.min(0) - pad, v.max(0) + pad, (n, 3)))


def _sign_mesh(which):
    if which == "cube":
        return CUBE_V, CUBE_T
    if which == "sphere":
        return uv_sphere(12, 16, 0.7, (3, -2, 5))
    if which == "sphere-rotated":
        return uv_sphere(12, 16, 0.7, (3, -2, 5), fixed_rotation())
    if which == "sphere-centred":
        return uv_sphere(8, 8)
    return l_prism()


# name -> (mesh, queries, kind): "lattice" = bounding-box lattice (points ON the surface are
# excluded by construction, so no limit on their share), "set" = at most MAX_EXCLUDED excluded
SIGN_FAMILIES = {
    "h-cube-lattice16": ("cube", lambda v: box_lattice(v, 16), "lattice"),
    "h-cube-lattice24": ("cube", lambda v: box_lattice(v, 24), "lattice"),
    "h-cube-random": ("cube", lambda v: _random_box(v, 0.5, 5000, 201), "set"),
    "h-sphere-random": ("sphere", lambda v: _random_box(v, 0.5, 5000, 202), "set"),
    "h-sphere-rotated-random": ("sphere-rotated", lambda v: _random_box(v, 0.5, 5000, 203), "set"),
    "h-sphere-centred-lattice17": ("sphere-centred", lambda v: box_lattice(v, 17), "set"),
    "h-sphere-centred-random": ("sphere-centred", lambda v: _random_box(v, 0.5, 5000, 204), "set"),
    "h-lprism-lattice13": ("lprism", lambda v: box_lattice(v, 13), "lattice"),
    "h-lprism-random": ("lprism", lambda v: _random_box(v, 0.5, 5000, 205), "set"),
}

CUBE_INTERIOR = {"h-cube-lattice16": 14 ** 3, "h-cube-lattice24": 22 ** 3}


@functools.lru_cache(maxsize=None)
def sign_case(name):
    """(verts, tris, queries, d64, winding number) — read-only, shared between tests."""
    which, make, _ = SIGN_FAMILIES[name]
    v, t = _sign_mesh(which)
    q = make(v)
    d64, _ = oracle.point_mesh_distance_f64(v, t, q)
    wn = oracle.inside_closed_mesh_f64(v, t, q)
    out = (_f32(v), np.ascontiguousarray(t, dtype=np.int32), q, d64, wn)
    for a in out:
        a.setflags(write=False)
    return out


def check_sign(name, signed, dist):
    """`signed` against the winding number, `abs(signed)` bit-equal to `dist`; returns
    (queries checked, queries excluded as near-surface)."""
    v, t, q, d64, wn = sign_case(name)
    signed, dist = np.asarray(signed).reshape(-1), np.asarray(dist).reshape(-1)
    assert signed.dtype == np.float32 and np.array_equal(np.abs(signed), dist), name
    far = d64 > SIGN_MIN * diagonal(v)
    inside = np.abs(wn) > 0.5
    # a closed, consistently oriented mesh: the winding number is an integer away from the surface
    assert np.abs(wn[far] - np.round(wn[far])).max() < 1e-6, name
    wrong = far & ((signed < 0) != inside)
    print(f"{name}: {int(far.sum())} queries checked ({int(inside[far].sum())} inside), "
          f"{int((~far).sum())} within {SIGN_MIN} * diag of the surface excluded, {int(wrong.sum())} wrong signs")
    assert not wrong.any(), (name, int(wrong.sum()), q[wrong][:5])
    if SIGN_FAMILIES[name][2] == "set":
        assert (~far).sum() <= MAX_EXCLUDED * len(q), (name, int((~far).sum()))
    if name in CUBE_INTERIOR:
        interior = ((q > 0) & (q < 1)).all(1)
        assert interior.sum() == CUBE_INTERIOR[name] and far[interior].all(), name
        assert (signed[interior] < 0).all(), name
    return int(far.sum()), int((~far).sum())
