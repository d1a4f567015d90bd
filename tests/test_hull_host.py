"""The hull contract and the box rule on the host: the restatement of tests/hull_restatement.py against
scipy.spatial.ConvexHull and against shapes with known answers, and the host side of geometry.hull.
No GPU."""
import numpy as np
import pytest

from tests import hull_restatement as hr


def _no_fourth_point(ijk, rows):
    p = ijk.astype(np.int64)
    a = p[rows[:, 0]]
    n = np.cross(p[rows[:, 1]] - a, p[rows[:, 2]] - a)
    on = (np.einsum("tj,mj->tm", n, p) == np.einsum("tj,tj->t", n, a)[:, None]).sum(axis=1)
    return bool((on == 3).all())


@pytest.mark.parametrize("case", range(3))
def test_restatement_equals_qhull_in_general_position(case):
    from scipy.spatial import ConvexHull
    from pyqsm_amd.geometry.hull import six_volume
    ijk = hr.random_cloud(*hr.RANDOM_CASES[case])
    rows, dim = hr.hull_by_definition(ijk)
    assert dim == 3
    assert _no_fourth_point(ijk, rows), "the comparison needs general position"
    q = ConvexHull(ijk.astype(np.float64))
    assert {frozenset(r) for r in rows.tolist()} == {frozenset(r) for r in q.simplices.tolist()}
    assert len(rows) == len(q.simplices)
    assert np.array_equal(np.unique(rows), np.sort(q.vertices))
    hr.certificate(ijk, rows)
    assert six_volume(ijk, rows) == hr.RANDOM_SIX_VOLUMES[case]
    for origin in ([0, 0, 0], ijk[0].tolist()):            # the same sum in Python integers, from two origins
        P = [[int(v) - int(o) for v, o in zip(r, origin)] for r in ijk.tolist()]
        det = lambda a, b, c: (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])
                               + a[2] * (b[0] * c[1] - b[1] * c[0]))
        assert sum(det(P[a], P[b], P[c]) for a, b, c in rows.tolist()) == hr.RANDOM_SIX_VOLUMES[case]
    assert six_volume(ijk, rows) / 6.0 == pytest.approx(q.volume, rel=1e-12)


def test_cube_is_eight_vertices_twelve_triangles():
    from pyqsm_amd.geometry.hull import six_volume
    cube = hr.cube444()
    rows, dim = hr.hull_by_definition(cube)
    assert dim == 3 and len(rows) == 12 and len(np.unique(rows)) == 8
    assert six_volume(cube, rows) == 162
    hr.certificate(cube, rows)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_fan_apex_follows_the_index(seed):
    shapes = hr.fixed_shapes()
    cube = shapes[f"cube444_perm{seed}"]
    rows, _ = hr.hull_by_definition(cube)
    assert len(rows) == 12
    hr.certificate(cube, rows)
    p = cube.astype(np.int64)
    for axis in range(3):
        for side in (0, 3):
            corners = [i for i in np.unique(rows) if p[i, axis] == side]
            face = [r for r in rows.tolist() if all(p[v, axis] == side for v in r)]
            assert len(corners) == 4 and len(face) == 2
            assert all(r[0] == min(corners) for r in face)


def test_octahedron_ignores_edge_midpoints():
    octa = hr.fixed_shapes()["octahedron_midpoints"]
    rows, dim = hr.hull_by_definition(octa)
    assert dim == 3 and len(rows) == 8
    assert sorted(np.unique(rows).tolist()) == list(range(5, 11))      # the six corners
    hr.certificate(octa, rows)


def test_prism_over_a_lattice_twelve_gon():
    from pyqsm_amd.geometry.hull import six_volume
    prism = hr.fixed_shapes()["prism12"]
    rows, dim = hr.hull_by_definition(prism)
    assert dim == 3 and len(rows) == 2 * 10 + 12 * 2 and len(np.unique(rows)) == 24
    hr.certificate(prism, rows)
    g = hr._gon12()
    twice_area = abs(int(np.sum(g[:, 0] * np.roll(g[:, 1], -1) - np.roll(g[:, 0], -1) * g[:, 1])))
    assert six_volume(prism, rows) == 3 * twice_area * 5


def test_duplicates_merge_to_the_lowest_index():
    dup = hr.fixed_shapes()["duplicates"]
    rows, dim = hr.hull_by_definition(dup)
    assert dim == 3
    first = {tuple(p): i for i, p in reversed(list(enumerate(dup.tolist())))}
    assert all(first[tuple(dup[v])] == v for v in np.unique(rows))
    base_rows, _ = hr.hull_by_definition(np.unique(dup, axis=0))
    assert len(rows) == len(base_rows)
    hr.certificate(dup, rows)


@pytest.mark.parametrize("name", sorted(hr.EXPECTED_DIM))
def test_segments_without_a_hull(name):
    rows, dim = hr.hull_by_definition(hr.fixed_shapes()[name])
    assert dim == hr.EXPECTED_DIM[name] and rows.shape == (0, 3)


def test_certificate_rejects_a_wrong_fan():
    """The face x = 0 cut along its other diagonal is still the hull, but not the canonical fan."""
    cube = hr.cube444()
    rows, _ = hr.hull_by_definition(cube)
    face = [i for i, r in enumerate(rows.tolist()) if all(cube[v, 0] == 0 for v in r)]
    r1, r2 = rows[face[0]].tolist(), rows[face[1]].tolist()
    v0 = r1[0]
    (y,), (x,), (z,) = set(r1) & set(r2) - {v0}, set(r1) - set(r2), set(r2) - set(r1)
    ring = [v0, x, y, z] if r1 == [v0, x, y] else [v0, z, y, x]

    def canon(t):
        k = t.index(min(t))
        return t[k:] + t[:k]

    bad = rows.copy()
    bad[face[0]] = canon([ring[1], ring[2], ring[3]])
    bad[face[1]] = canon([ring[0], ring[1], ring[3]])
    bad = bad[np.lexsort((bad[:, 2], bad[:, 1], bad[:, 0]))]
    assert hr.hull_by_definition(cube)[0].tolist() != bad.tolist()
    with pytest.raises(AssertionError, match="different fans"):
        hr.certificate(cube, bad)


def test_box_rule_against_a_plain_loop():
    rng = np.random.default_rng(9)
    pts = rng.uniform(-2, 2, (400, 3))
    pts[:6] = [[1, 0.3, 0.2], [-1, 0, 0], [0.5, 2, -0.5], [0, -2, 0], [0.25, 0.5, 0.75], [0, 0, -0.75]]   # on faces
    pts[6] = [0.125, -0.375, 1.5]
    ang = 0.7
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
    boxes = np.array([np.r_[0, 0, 0, np.eye(3).ravel(), 1, 2, 0.75],
                      np.r_[0.1, -0.2, 0.3, Rz.ravel(), 1.5, 0.5, 1.0],
                      np.r_[0.125, -0.375, 1.5, Rz.ravel(), 0, 0, 0]])          # zero extent, centred on a point
    ptr, idx = hr.boxes_rule(pts, boxes)
    want = []
    for b in boxes:
        c, R, h = b[:3], b[3:12].reshape(3, 3), b[12:]
        for i, p in enumerate(pts):
            d = p - c
            t = [(d[0] * R[0][k] + d[1] * R[1][k]) + d[2] * R[2][k] for k in range(3)]
            if all(abs(t[k]) <= h[k] for k in range(3)):
                want.append(i)
    assert idx.tolist() == want
    assert set(range(6)) <= set(idx[ptr[0]:ptr[1]].tolist())
    assert idx[ptr[2]:ptr[3]].tolist() == [6]


def test_oriented_box_host_side():
    """The wrapper's host half: the PCA frame is the one oriented_bounds uses, and the box algebra."""
    from pyqsm_amd.geometry import skeletonize
    from pyqsm_amd.geometry.hull import OrientedBoundingBox, pca_frame
    pts = np.random.default_rng(3).normal(size=(60, 3)) * [3, 1, 0.3]
    from scipy.spatial import ConvexHull
    hv = pts[np.sort(ConvexHull(pts).vertices)]
    box = OrientedBoundingBox.from_hull_points(hv)
    lo, hi = skeletonize.oriented_bounds(pts)
    assert np.array_equal(box.get_min_bound(), lo) and np.array_equal(box.get_max_bound(), hi)
    mean, R, flo, fhi = pca_frame(hv)
    assert np.allclose(R[:, 0], np.cross(R[:, 1], R[:, 2])) and np.allclose(R.T @ R, np.eye(3))
    assert box.volume() == pytest.approx(float(np.prod(fhi - flo)))
    assert np.allclose(np.sort(box.get_box_points(), axis=0),
                       np.sort(OrientedBoundingBox(box.center, box.R, box.extent).get_box_points(), axis=0))
    c0 = box.center.copy()
    moved = OrientedBoundingBox(box.center, box.R, box.extent).translate((0, 0, 1)).scale(1.1, c0)
    assert np.allclose(moved.center, c0 + 1.1 * np.array([0, 0, 1.0])) and np.allclose(moved.extent, 1.1 * box.extent)
    row = box.as_row()
    ptr, idx = hr.boxes_rule(hv, row[None, :])
    assert ptr[1] >= len(hv) - 6          # the vertices span the box: all inside up to rounding on the faces


def test_hull_result_volume_and_area_from_integers():
    from scipy.spatial import ConvexHull as Q
    from pyqsm_amd.geometry.hull import ConvexHull
    ijk = hr.random_cloud(*hr.RANDOM_CASES[0])
    rows, dim = hr.hull_by_definition(ijk)
    pts = ijk * 0.25
    h = ConvexHull(pts, ijk, rows, dim, 0.25, np.zeros(3))
    q = Q(pts)
    assert h.six_volume == hr.RANDOM_SIX_VOLUMES[0] and isinstance(h.six_volume, int)
    assert h.volume == pytest.approx(q.volume, rel=1e-12) and h.area == pytest.approx(q.area, rel=1e-12)
    assert np.array_equal(h.vertices, np.sort(q.vertices))
    m = h.to_mesh()
    assert np.array_equal(np.asarray(m.triangles), rows) and len(np.asarray(m.vertices)) == len(pts)
