"""pyqsm_alpha_shape3 on the GPU against the CPU statements of its contract (tests/alpha3_restatement.py;
tests/test_alpha3_host.py pins the brute-force definition to the Delaunay route and to the table the contract was
settled on): rows, kinds, vol6 and the deterministic counters are compared as integers, never within a tolerance."""
import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry import hull
from pyqsm_amd.geometry import mesh_processing as mp
from pyqsm_amd.geometry.cloud import PointCloud, TriangleMesh
from tests import alpha3_restatement as A

pytestmark = pytest.mark.gpu

DETERMINISTIC = ("estimated_tests", "tests", "candidates", "unresolved_ties", "max_stencil", "max_cell_points",
                 "work_items")


def assert_same(res, ref):
    rows, vol6, unresolved = ref
    assert res.rows.dtype == np.int32 and res.rows.shape[1] == 4
    assert np.array_equal(res.rows, rows)                   # (a, b, c, kind): triangles, orientation and kinds
    assert res.vol6 == vol6
    assert res.stats["unresolved_ties"] == unresolved


def assert_work(res, P, rho2, seg_start=None):
    cands, tests = A.work(P, rho2, seg_start)
    assert (res.stats["candidates"], res.stats["tests"]) == (cands, tests)


@pytest.mark.parametrize("key", sorted(A.TABLE))
def test_table_clouds(gpu, key):
    seed, n, ext, rho2 = key
    P = A.table_cloud(seed, n, ext)
    ref = A.table_reference(key)
    both = hip.alpha_shape3(P, rho2, faces="all")
    assert_same(both, ref)
    assert_work(both, P, rho2)
    regular = hip.alpha_shape3(P, rho2)
    assert_same(regular, (ref[0][ref[0][:, 3] == A.REGULAR], ref[1], 0))
    want = A.TABLE[key]
    assert ((both.rows[:, 3] == 1).sum(), (both.rows[:, 3] == 2).sum(), both.vol6[0]) == want
    assert {k: both.stats[k] for k in DETERMINISTIC} == {k: regular.stats[k] for k in DETERMINISTIC}


@pytest.mark.parametrize("pitch", (1, 7))
@pytest.mark.parametrize("which", (0, 1))
def test_tie_lattice(gpu, pitch, which):
    rho2 = A.tie_radii(pitch)[which]
    far = (-(1 << 31), 17, (1 << 31) - 1 - 2 * pitch)
    for perm_seed, shift in ((None, (0, 0, 0)), (5, (0, 0, 0)), (6, (-40, 1 << 20, 3)), (None, far), (7, far)):
        P = A.tie_lattice(pitch, perm_seed, shift)
        for faces in ("all", "regular"):
            res = hip.alpha_shape3(P, rho2, faces=faces)
            assert_same(res, A.brute(P, rho2, faces=faces))
            assert_work(res, P, rho2)
            assert res.vol6 == [6 * (2 * pitch) ** 3] and res.stats["exact_fallbacks"] > 0


def test_cube_corners_count_their_ties(gpu):
    P = A.cube_corners()
    res = hip.alpha_shape3(P, A.cube_rho2(), faces="all")
    assert_same(res, A.brute(P, A.cube_rho2()))
    assert res.stats["unresolved_ties"] == len(res.rows) > 0


def test_sphere_sheets(gpu):
    P = A.sphere_points()
    res = hip.alpha_shape3(P, 500 * 500, faces="all")
    assert_same(res, A.brute(P, 500 * 500))
    assert len(res.rows) == 2 * len(P) - 4 and (res.rows[:, 3] == A.SINGULAR).all()
    assert len(hip.alpha_shape3(P, 500 * 500).rows) == 0


def test_nested_shells_slices_chunks_and_empty_cells(gpu):
    P, rho2 = A.nested_shells()
    rows, vol6 = A.nested_shells_reference()
    res = hip.alpha_shape3(P, rho2)
    assert_same(res, (rows, vol6, 0))
    assert res.stats["max_stencil"] > hip.ALPHA3_CHUNK and res.stats["max_cell_points"] > 4 * hip.ALPHA3_SLICE
    assert res.stats["work_items"] > 64
    both = hip.alpha_shape3(P, rho2, faces="all")
    assert np.array_equal(both.rows[both.rows[:, 3] == A.REGULAR], rows) and both.vol6 == vol6


def test_segments_equal_each_alone(gpu):
    (ka, kb) = [k for k in sorted(A.TABLE) if k[3] == 900][:2]
    Pa, Pb = A.table_cloud(*ka[:3]), A.table_cloud(*kb[:3])           # both fill the same box of 100 units
    P = np.concatenate([Pa, Pb])
    seg = [0, len(Pa), len(P)]
    for faces in ("all", "regular"):
        res = hip.alpha_shape3(P, 900, seg_start=seg, faces=faces)
        assert_same(res, A.brute(P, 900, seg_start=seg, faces=faces))
        ra, rb = hip.alpha_shape3(Pa, 900, faces=faces), hip.alpha_shape3(Pb, 900, faces=faces)
        moved = rb.rows.copy()
        moved[:, :3] += len(Pa)
        assert np.array_equal(res.rows, np.concatenate([ra.rows, moved])) and res.vol6 == ra.vol6 + rb.vol6
    assert_work(res, P, 900, seg)
    one = hip.alpha_shape3(P, 900)
    assert_same(one, A.brute(P, 900, faces="regular"))
    assert one.vol6[0] != res.vol6[0] + res.vol6[1] and len(one.rows) != len(res.rows)
    # an empty segment and one of two points among them
    seg4 = [0, 0, len(Pa), len(Pa) + 2, len(P)]
    res4 = hip.alpha_shape3(P, 900, seg_start=seg4)
    assert_same(res4, A.brute(P, 900, seg_start=seg4, faces="regular"))
    assert res4.vol6[0] == 0 and res4.vol6[2] == 0 and res4.vol6[1] == ra.vol6[0]
    shapes = hull.alpha_shapes(P.astype(np.float64), seg, 30.0, quantum=1.0)
    assert [s.six_volume for s in shapes] == res.vol6
    assert np.array_equal(shapes[1].triangles, rb.rows[:, :3]) and len(shapes[1].points) == len(Pb)


def test_repeats_and_permutations(gpu):
    key = sorted(A.TABLE)[0]
    P, rho2 = A.table_cloud(*key[:3]), key[3]
    first = hip.alpha_shape3(P, rho2, faces="all")
    for _ in range(3):
        again = hip.alpha_shape3(P, rho2, faces="all")
        assert again.rows.tobytes() == first.rows.tobytes() and again.vol6 == first.vol6
        assert {k: again.stats[k] for k in DETERMINISTIC} == {k: first.stats[k] for k in DETERMINISTIC}
    perm = np.random.default_rng(1).permutation(len(P))
    shuffled = hip.alpha_shape3(P[perm], rho2, faces="all")
    assert A.geometric_set(P[perm], shuffled.rows) == A.geometric_set(P, first.rows)
    assert shuffled.vol6 == first.vol6
    Q, q_rho2 = A.nested_shells()
    a, b = hip.alpha_shape3(Q, q_rho2), hip.alpha_shape3(Q[::-1].copy(), q_rho2)
    assert A.geometric_set(Q[::-1], b.rows) == A.geometric_set(Q, a.rows) and a.vol6 == b.vol6


def test_volume_is_below_the_hull(gpu):
    pts, alpha, q = A.solid_cloud()
    ijk, _, rho2 = hull.snap_for_radius(pts, alpha)
    res = hip.alpha_shape3(ijk, rho2)
    h = hip.convex_hull(ijk)
    assert res.stats["unresolved_ties"] == 0
    assert 0 < res.vol6[0] <= hull.six_volume(ijk, h.tris)


def test_refusals(gpu):
    key = sorted(A.TABLE)[0]
    P, rho2 = A.table_cloud(*key[:3]), key[3]
    ref = A.table_reference(key)
    lib = _lib.load()
    import ctypes
    n_rows, out, halves, st = ctypes.c_int64(0), ctypes.c_void_p(), np.zeros(2, np.uint64), np.zeros(8, np.int64)
    code = lib.pyqsm_alpha_shape3(P.ctypes.data, len(P), None, 1, hip.RECON_MAX_RHO2 + 1, 0, 0, ctypes.byref(n_rows),
                                  ctypes.byref(out), halves.ctypes.data, st.ctypes.data, 0)
    assert code == -1 and not out.value and b"would fit" in lib.pyqsm_last_error()          # PYQSM_EINVAL
    with pytest.raises(hip.AlphaShapeRefused, match="max_tests") as e:
        hip.alpha_shape3(P, rho2, max_tests=1)
    assert e.value.code == -4 and e.value.stats["estimated_tests"] > 1 and e.value.stats["max_stencil"] > 0
    assert e.value.stats["candidates"] == 0                                                  # no triangle pass ran
    assert_same(hip.alpha_shape3(P, rho2, faces="all"), ref)
    S = A.cospherical_set()
    with pytest.raises(hip.AlphaShapeRefused, match="more than 16 n") as e:
        hip.alpha_shape3(S, A.R2_SPHERE)
    assert e.value.code == -4 and e.value.stats["candidates"] == 40 * 39 * 38 // 6
    assert_same(hip.alpha_shape3(P, rho2, faces="all"), ref)
    for n in (0, 2):
        assert hip.alpha_shape3(P[:n], rho2).rows.shape == (0, 4)
    T = np.array([[5, 5, 5], [15, 5, 5], [5, 15, 5]], np.int32)         # three points: one sheet, two empty balls
    three = hip.alpha_shape3(T, 100, faces="all")
    assert_same(three, A.brute(T, 100))
    assert three.rows.tolist() == [[0, 1, 2, A.SINGULAR]] and len(hip.alpha_shape3(T, 100).rows) == 0


def test_wrappers(gpu):
    pts, alpha, q = A.solid_cloud()
    mesh = TriangleMesh.create_from_point_cloud_alpha_shape(PointCloud(pts), alpha, None, None)
    assert mesh.n_unresolved_ties == 0 and mesh.quantum == q and len(mesh.vertices) == len(pts)
    props = mp.check_properties(mesh)
    assert props["watertight"] and props["edge_manifold"] and props["orientable"]
    shape = hull.alpha_shape(pts, alpha, faces="all")
    ijk, _, rho2 = hull.snap_for_radius(pts, alpha)
    rows, vol6 = A.delaunay(ijk, rho2)
    regular = shape.triangles[shape.kinds == hip.ALPHA3_REGULAR]
    assert np.array_equal(regular, rows[:, :3]) and np.array_equal(mesh.triangles, regular)
    assert shape.six_volume == vol6[0] == mesh.six_volume
    assert shape.volume == vol6[0] * q ** 3 / 6 == mesh.volume
    assert abs(shape.area - mesh.get_surface_area()) <= 1e-12 * shape.area
    assert np.array_equal(shape.vertices, np.unique(shape.triangles))
    assert shape.volume < hull.convex_hull(pts).volume
