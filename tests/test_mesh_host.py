"""The mesh-check restatement (tests/mesh_restatement.py) against independent routes, without a GPU:
clusters against SciPy's connected components, the tri-tri decision against exact rational
clipping, and the named meshes against the answers known for them."""
from fractions import Fraction

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from pyqsm_amd.geometry import mesh_processing as mp
from pyqsm_amd.geometry.cloud import TriangleMesh
from tests import mesh_restatement as mr


# ---------------------------------------------------------------- clusters against SciPy

def _scipy_clusters(tris):
    t = np.asarray(tris, dtype=np.int64)
    nt = len(t)
    by_edge = {}
    for ti, (a, b, c) in enumerate(t):
        for u, w in ((a, b), (b, c), (c, a)):
            by_edge.setdefault((min(u, w), max(u, w)), []).append(ti)
    rows, cols = [], []
    for members in by_edge.values():
        for m in members[1:]:
            rows.append(members[0])
            cols.append(m)
    g = coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nt, nt))
    lab = connected_components(g, directed=False)[1]
    # renumber by ascending smallest member triangle
    smallest = np.full(lab.max() + 1, nt, np.int64)
    np.minimum.at(smallest, lab, np.arange(nt))
    return np.argsort(np.argsort(smallest))[lab]


@pytest.mark.parametrize("name", sorted(mr.NAMED))
def test_clusters_equal_scipy_components(name):
    verts, tris = mr.NAMED[name]()
    got = mr.topology(tris, len(verts), verts)
    want = _scipy_clusters(tris)
    assert np.array_equal(got["tri_cluster"], want)
    assert np.array_equal(got["cluster_n"], np.bincount(want))
    assert got["summary"][5] == want.max() + 1


# ---------------------------------------------------------------- tri-tri against exact rationals

def _cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _clip_polygon(poly, inside_value):
    """Sutherland-Hodgman against the closed half-plane inside_value(p) >= 0 (exact)."""
    out = []
    n = len(poly)
    for k in range(n):
        p, q = poly[k], poly[(k + 1) % n]
        sp, sq = inside_value(p), inside_value(q)
        if sp >= 0:
            out.append(p)
        if n > 1 and ((sp > 0 and sq < 0) or (sp < 0 and sq > 0)):
            s = Fraction(sp) / Fraction(sp - sq)
            out.append(tuple(a + s * (b - a) for a, b in zip(p, q)))
    return out


def rational_tri_tri(a, b) -> bool:
    """Clip triangle a by b's plane to a segment and the segment by b's three edge half-planes; a
    polygon clip in 2-D when the triangles are coplanar. False when either is degenerate."""
    a = [tuple(Fraction(int(x)) for x in v) for v in a]
    b = [tuple(Fraction(int(x)) for x in v) for v in b]
    na = _cross(_sub(a[1], a[0]), _sub(a[2], a[0]))
    nb = _cross(_sub(b[1], b[0]), _sub(b[2], b[0]))
    if not any(na) or not any(nb):
        return False
    d = [_dot(nb, _sub(v, b[0])) for v in a]
    # inward side of b's edge k, within b's plane: (nb x edge) . (x - b_k) >= 0
    inward = [(_cross(nb, _sub(b[(k + 1) % 3], b[k])), b[k]) for k in range(3)]
    if all(x == 0 for x in d):
        poly = list(a)
        for m, base in inward:
            poly = _clip_polygon(poly, lambda p, m=m, base=base: _dot(m, _sub(p, base)))
            if not poly:
                return False
        return True
    if all(x > 0 for x in d) or all(x < 0 for x in d):
        return False
    pts = [a[k] for k in range(3) if d[k] == 0]
    for k in range(3):
        k1 = (k + 1) % 3
        if (d[k] > 0 and d[k1] < 0) or (d[k] < 0 and d[k1] > 0):
            s = d[k] / (d[k] - d[k1])
            pts.append(tuple(p + s * (q - p) for p, q in zip(a[k], a[k1])))
    x0, x1 = min(pts), max(pts)          # collinear points: the lexicographic extremes are the ends
    lo, hi = Fraction(0), Fraction(1)    # Liang-Barsky on x0 + s (x1 - x0)
    for m, base in inward:
        f0, f1 = _dot(m, _sub(x0, base)), _dot(m, _sub(x1, base))
        if f0 < 0 and f1 < 0:
            return False
        if f0 < 0:
            lo = max(lo, f0 / (f0 - f1))
        elif f1 < 0:
            hi = min(hi, f0 / (f0 - f1))
    return lo <= hi


def _random_pairs(rng, n, span):
    return rng.integers(0, span + 1, (n, 3, 3)), rng.integers(0, span + 1, (n, 3, 3))


def _check_pairs(a, b):
    deg = mr.degenerate(a) | mr.degenerate(b)
    got = np.zeros(len(a), bool)
    got[~deg] = mr.tri_tri(a[~deg], b[~deg])
    want = np.array([rational_tri_tri(x, y) for x, y in zip(a, b)])
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (a[bad[0]].tolist(), b[bad[0]].tolist(), bool(want[bad[0]]))
    return deg, want


def test_tri_tri_equals_rational_clipping_on_small_lattice():
    rng = np.random.default_rng(11)
    a, b = _random_pairs(rng, 6000, 6)
    b[:1500, :, 2] = 3                     # coplanar families: both in z = 3, or sharing a plane x = y
    a[:1500, :, 2] = 3
    a[1500:2200, :, 1] = a[1500:2200, :, 0]
    b[1500:2200, :, 1] = b[1500:2200, :, 0]
    deg, want = _check_pairs(a, b)
    # the sample is not trivial: hits, misses and degenerate triangles are all common
    assert want.sum() > 1000 and (~want & ~deg).sum() > 500 and deg.sum() > 100


def test_tri_tri_equals_rational_clipping_at_full_extent():
    rng = np.random.default_rng(12)
    a, b = _random_pairs(rng, 600, 1)
    a, b = a * mr.MAX_EXTENT, b * mr.MAX_EXTENT          # corners of the 2^20 cube: the largest determinants
    a2, b2 = _random_pairs(rng, 600, mr.MAX_EXTENT)
    deg, want = _check_pairs(np.concatenate([a, a2]), np.concatenate([b, b2]))
    assert want.sum() > 100 and (~want & ~deg).sum() > 100


def test_touching_cases_by_hand():
    t = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]])
    cases = [
        ([[1, 1, 0], [1, 1, 3], [2, 1, 3]], True),      # a vertex on the face
        ([[1, 1, 1], [1, 1, 3], [2, 1, 3]], False),     # one unit above it
        ([[2, -1, -1], [2, 1, 1], [2, -1, 1]], True),   # an edge crossing the edge y = 0 at (2, 0, 0)
        ([[1, 1, 0], [2, 1, 0], [1, 2, 0]], True),      # coplanar, inside
        ([[5, 5, 0], [6, 5, 0], [5, 6, 0]], False),     # coplanar, apart
        ([[4, 0, 0], [8, 0, 0], [6, -3, 0]], True),     # collinear edges touching at (4, 0, 0)
        ([[5, 0, 0], [8, 0, 0], [6, -3, 0]], False),    # collinear edges one unit apart
    ]
    for other, want in cases:
        o = np.array(other)
        assert bool(mr.tri_tri(t[None], o[None])[0]) is want, other
        assert bool(mr.tri_tri(o[None], t[None])[0]) is want, other
        assert rational_tri_tri(t, o) is want, other


# ---------------------------------------------------------------- the named meshes

def _summary(name):
    verts, tris = mr.NAMED[name]()
    return mr.topology(tris, len(verts), verts)


def test_cube_is_closed_and_orientable():
    for name, n_edges in (("tetrahedron", 6), ("octahedron", 12), ("cube", 18)):
        s = _summary(name)["summary"]
        assert s.tolist() == [n_edges, 0, 0, 0, 0, 1, 1, 0], name


def test_flipped_triangle_shows_as_same_direction_edges():
    top = _summary("cube_flipped")
    assert top["summary"].tolist() == [18, 0, 0, 3, 0, 1, 1, 0]     # still orientable: flip it back


def test_sheet_has_a_boundary():
    s = _summary("sheet")["summary"]
    assert s[1] == 4 * 7 and s[2] == 0 and s[4] == 0 and s[5] == 1 and s[6] == 1


def test_moebius_is_edge_manifold_and_not_orientable():
    s = _summary("moebius")["summary"]
    assert s[2] == 0 and s[4] == 0 and s[5] == 1 and s[6] == 0 and s[1] == 32


def test_two_tetrahedra_at_one_vertex():
    top = _summary("two_tets_one_vertex")
    assert top["summary"][5] == 2 and top["summary"][4] == 1
    assert top["vertex_flags"].tolist() == [1, 0, 0, 0, 0, 0, 0]


def test_three_triangles_on_one_edge():
    top = _summary("three_on_an_edge")
    assert top["edges"][0].tolist() == [0, 1] and top["edge_count"][0] == 3 and top["edge_flags"][0] == 2
    assert top["summary"][2] == 1 and top["summary"][6] == 0


def test_many_tets_and_strip():
    top = _summary("many_tets")
    assert top["summary"][5] == 300 and (top["cluster_n"] == 4).all() and top["summary"][6] == 1
    assert top["tri_cluster"][0] == 0
    top = _summary("shuffled_strip")
    assert top["summary"][5] == 1 and top["summary"][6] == 1 and top["summary"][3] == 0


def test_areas_follow_the_formula():
    verts, tris = mr.cube()
    top = mr.topology(tris, len(verts), verts)
    assert top["tri_area"].tolist() == [0.5] * 12 and top["cluster_area"].tolist() == [6.0]


# ---------------------------------------------------------------- host-side wrappers

def test_host_side_removals():
    mesh = TriangleMesh(np.zeros((4, 3)), [[0, 1, 2], [1, 1, 3], [2, 3, 0]])
    assert mesh.remove_degenerate_triangles().triangles.tolist() == [[0, 1, 2], [2, 3, 0]]
    assert mesh.remove_triangles_by_mask([True, False]).triangles.tolist() == [[2, 3, 0]]
    ijk, q, origin = mp.quantize_mesh(np.array([[0.0, 0, 0], [50.0, 1, 2]]))
    assert q == 2.0 ** -14 and ijk.max() == 50 * 2 ** 14 and origin.tolist() == [0, 0, 0]


def test_binding_constants_equal_the_header():
    import os
    import re
    from pyqsm_amd import hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pyqsm_hip.h")).read()
    value = lambda name: int(re.search(rf"#define {name} (-?\d+)", text).group(1))
    assert hip.MESH_DEFAULT_MAX_TESTS == value("PYQSM_MESH_DEFAULT_MAX_TESTS")
    assert hip.MESH_TILE_ROWS == value("PYQSM_MESH_TILE_ROWS") and hip.MESH_PAIRS == value("PYQSM_MESH_PAIRS")
