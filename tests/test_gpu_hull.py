"""pyqsm_convex_hull on the GPU: its rows byte for byte against the contract stated by definition
(tests/hull_restatement.py, itself pinned to Qhull by tests/test_hull_host.py) on small clouds, and against
the certificate and SciPy's vertex set on clouds too large for the definition."""
import functools

import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry import hull as gh
from pyqsm_amd.geometry import skeletonize
from pyqsm_amd.geometry.cloud import PointCloud
from tests import hull_restatement as hr

pytestmark = pytest.mark.gpu

SHAPES = hr.fixed_shapes()
SMALL = sorted(SHAPES) + [f"random{k}" for k in range(3)]


def cloud(name):
    return hr.random_cloud(*hr.RANDOM_CASES[int(name[6:])]) if name.startswith("random") else SHAPES[name]


@functools.lru_cache(maxsize=None)
def expected(name):
    return hr.hull_by_definition(cloud(name))


@functools.lru_cache(maxsize=None)
def ball():
    from scipy.spatial import ConvexHull
    ijk = hr.ball_cloud()
    return ijk, np.sort(ConvexHull(ijk.astype(np.float64)).vertices)


@pytest.mark.parametrize("name", SMALL)
def test_rows_equal_the_definition(gpu, name):
    ijk = cloud(name)
    rows, dim = expected(name)
    r = hip.convex_hull(ijk)
    assert int(r.dim[0]) == dim
    assert r.tris.dtype == np.int32 and r.tris.tobytes() == rows.tobytes()
    assert r.tri_ptr.tolist() == [0, len(rows)]
    if dim == 3:
        hr.certificate(ijk, r.tris)
        dup = len(ijk) - len(np.unique(ijk, axis=0))
        assert r.stats["merged_duplicates"] <= dup and r.stats["rounds"] >= 1 and r.stats["tests"] > 0
    else:
        assert r.stats["tests"] == 0


def test_flat_facets_are_counted(gpu):
    assert hip.convex_hull(SHAPES["cube444"]).stats["flat_facets"] == 6
    assert hip.convex_hull(SHAPES["prism12"]).stats["flat_facets"] == 14
    assert hip.convex_hull(cloud("random1")).stats["flat_facets"] == 0


def test_batched_call_equals_the_single_calls(gpu):
    names = SMALL + ["empty", "tetrahedron"]
    extra = [np.zeros((0, 3), np.int32), np.array([[0, 0, 0], [4, 1, 0], [2, 7, 1]], np.int32), SHAPES["coplanar"] + 9]
    parts = [cloud(n) + np.int32(17 * k) for k, n in enumerate(names)] + extra
    seg = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    r = hip.convex_hull(np.concatenate(parts), seg)
    want_dim = [expected(n)[1] for n in names] + [-1, 2, 2]
    assert r.dim.tolist() == want_dim
    for s, n in enumerate(names):
        rows = expected(n)[0]
        got = r.tris[r.tri_ptr[s]:r.tri_ptr[s + 1]]
        assert np.array_equal(got, rows + np.int32(seg[s])), n
    assert r.tri_ptr[-1] == sum(len(expected(n)[0]) for n in names)


def test_ball_of_70000_points(gpu):
    ijk, qv = ball()
    r = hip.convex_hull(ijk)
    V, F = hr.certificate(ijk, r.tris)
    assert np.array_equal(np.unique(r.tris), qv)
    assert F == 2 * V - 4 and r.stats["flat_facets"] == 0      # general position
    assert r.stats["candidates"] < len(ijk) // 4                # the prefilter did its work
    pts = ijk.astype(np.float64)
    lo, hi = skeletonize.oriented_bounds(pts)
    box = PointCloud(pts).get_oriented_bounding_box()
    assert np.array_equal(box.get_min_bound(), lo) and np.array_equal(box.get_max_bound(), hi)
    lo2, hi2 = skeletonize.oriented_bounds(pts, device=0, hull="device")
    assert np.array_equal(lo2, lo) and np.array_equal(hi2, hi)
    lo3, hi3 = skeletonize.oriented_bounds(pts, device=0)
    assert np.array_equal(lo3, lo) and np.array_equal(hi3, hi)


def test_shell_runs_many_rounds(gpu):
    from scipy.spatial import ConvexHull
    ijk = hr.shell_cloud()
    r = hip.convex_hull(ijk)
    V, F = hr.certificate(ijk, r.tris)
    assert np.array_equal(np.unique(r.tris), np.sort(ConvexHull(ijk.astype(np.float64)).vertices))
    assert V > 0.95 * len(np.unique(ijk, axis=0)) and r.stats["candidates"] > 0.95 * len(ijk)
    assert r.stats["rounds"] > 10


def test_max_tests_ends_the_call(gpu):
    ijk, _ = ball()
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.convex_hull(ijk, max_tests=1)
    assert e.value.code == -4                                   # PYQSM_ERANGE


def test_extent_above_2_20_is_refused(gpu):
    ijk = np.array([[0, 0, 0], [(1 << 20) + 1, 0, 0], [0, 5, 0], [0, 0, 5]], np.int32)
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.convex_hull(ijk)
    assert e.value.code == -1                                   # PYQSM_EINVAL
    ok = ijk.copy()
    ok[1, 0] = 1 << 20
    assert len(hip.convex_hull(ok).tris) == 4


def test_two_runs_give_the_same_bytes(gpu):
    ijk = hr.shell_cloud(600, seed=8)
    a, b = hip.convex_hull(ijk), hip.convex_hull(ijk)
    assert a.tris.tobytes() == b.tris.tobytes() and a.stats == b.stats
    ijk2, _ = ball()
    c, d = hip.convex_hull(ijk2), hip.convex_hull(ijk2)
    assert c.tris.tobytes() == d.tris.tobytes() and c.stats == d.stats


def test_hull_object_and_pyqsm_names(gpu):
    from scipy.spatial import ConvexHull
    from pyqsm_amd.utils import lib_integration as li
    pts = np.random.default_rng(21).normal(size=(3000, 3)) * [2.0, 1.0, 4.0]
    h = gh.convex_hull(pts)
    q = ConvexHull(pts)
    assert h.dim == 3 and np.array_equal(h.vertices, np.sort(q.vertices))
    assert h.volume == pytest.approx(q.volume, rel=1e-5) and h.area == pytest.approx(q.area, rel=1e-5)
    mesh, idx = PointCloud(pts).compute_convex_hull()
    assert np.array_equal(idx, h.vertices) and len(np.asarray(mesh.vertices)) == len(idx)
    assert np.array_equal(idx[np.asarray(mesh.triangles)], h.simplices)
    full = li.sps_hull_to_mesh(PointCloud(pts))
    assert np.array_equal(np.asarray(full.triangles), h.simplices) and len(np.asarray(full.vertices)) == len(pts)
    seg = np.array([0, 1000, 1000, 3000])
    hs = gh.convex_hulls(pts, seg)
    assert [x.dim for x in hs] == [3, -1, 3]
    assert np.array_equal(hs[2].vertices, np.sort(ConvexHull(pts[1000:]).vertices))
