"""The ball-pivoting contract on the CPU (tests/recon_restatement.py): the brute-force definition and the
Delaunay route agree on the clouds in general position the GPU tests use, the degenerate fixtures give
what the issue's trial gave, and the host side of the wrappers (snapping, refusals, vertex normals, the
binding's constants, the sanitizer program of the integer predicate and of the fp64 filter in front of it)
holds without a GPU, and the tie-dense inputs of tests/recon_cases.py have the properties they are for."""
import os
import re
import subprocess

import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry.cloud import PointCloud, TriangleMesh
from tests import recon_cases as C
from tests import recon_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(R.GENERAL_POSITION))
def test_brute_force_equals_delaunay_route(name):
    P, Nr, rho2 = R.GENERAL_POSITION[name]()
    b, d = R.brute(P, Nr, rho2), R.delaunay(P, Nr, rho2)
    assert np.array_equal(b[0], d[0]) and np.array_equal(b[1], d[1]) and b[2] == d[2] == 0
    T, lv = b[:2]
    assert R.open_half_edges(T) == [] and len(T) == 2 * len(P) - 4      # closed, Euler characteristic 2
    if name == "holed_sphere":
        rim = R.open_half_edges(T[lv == 0])
        assert len(rim) > 3 and R.loops(rim) == 1 and 0 < (lv == 1).sum() < len(rim)
    if name == "holed_sphere_late":                                      # the same mesh, two levels later
        ref = R.delaunay(*R.holed_sphere())
        assert np.array_equal(T, ref[0]) and np.array_equal(lv, ref[1] + 2)


def test_nested_surfaces_delaunay_route_is_closed():
    """Two closed surfaces; points the ball cannot reach between higher neighbours stay unused."""
    P, Nr, rho2 = R.nested_surfaces()
    T, lv, _ = R.delaunay(P, Nr, rho2)
    used = len(np.unique(T))
    assert R.open_half_edges(T) == [] and len(T) == 2 * used - 8 and used > 0.9 * len(P)
    outer = np.linalg.norm(P - P.mean(axis=0), axis=1) > 2.6 * np.sqrt(rho2[0])
    assert 0 < outer.sum() < len(P) and (outer[T].all(axis=1) | ~outer[T].any(axis=1)).all()   # none joins the two


def test_plane_grid_takes_one_diagonal_per_square():
    P, Nr, rho2 = R.plane_grid()
    T, lv, unresolved = R.brute(P, Nr, rho2)
    assert len(T) == 72 and R.twice_area(P, T) == 720000 and unresolved == 0
    half = R.half_edges(T)
    assert len(set(half)) == len(half)
    # the fourth corner of a square lies on the ball of the other three at ANY radius (the four are
    # concyclic): the rule, not the radius, is what leaves one diagonal
    assert len(R.brute(P, Nr, (150 * 150 + 1,))[0]) == 72


def test_cospherical_corners_are_counted():
    P, Nr, rho2 = R.cospherical_five()
    T, lv, unresolved = R.brute(P, Nr, rho2)
    assert [0, 1, 2] in T.tolist() and unresolved > 0


def test_classify_matches_the_ball():
    """setup / classify against the ball written out in fp64, on random triples and points."""
    rng = np.random.default_rng(2)
    seen = set()
    for _ in range(400):
        a, b, c, p = (tuple(int(v) for v in rng.integers(-300, 300, 3)) for _ in range(4))
        t = R.setup(a, b, c, 400 * 400)
        if t is None:
            continue
        n = np.array(t["n"], np.float64)
        centre = np.array(a) + np.array(t["w"], np.float64) / (2 * t["n2"]) + np.sqrt(float(t["H"])) * n / (2 * t["n2"])
        for q in (a, b, c):
            assert abs(np.linalg.norm(centre - np.array(q)) - 400) < 1e-6
        gap = np.linalg.norm(centre - np.array(p)) - 400
        if abs(gap) > 1e-6:
            w = R.classify(t, tuple(x - y for x, y in zip(p, a)))
            assert w == (R.INSIDE if gap < 0 else R.OUTSIDE)
            seen.add(w)
    assert seen == {R.INSIDE, R.OUTSIDE}


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "pyqsm_hip.h")).read()

    def macro(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))

    assert hip.RECON_MAX_RHO2 == macro("PYQSM_RECON_MAX_RHO2") >= 1 << 20       # rho of at least 2^10
    assert hip.RECON_CHUNK == macro("PYQSM_RECON_CHUNK")
    assert hip.RECON_SLICE == macro("PYQSM_RECON_SLICE")
    assert hip.RECON_DEFAULT_MAX_TESTS == macro("PYQSM_RECON_DEFAULT_MAX_TESTS")


def test_host_side_refusals_and_snapping():
    P, Nr, rho2 = R.sphere()
    cloud = PointCloud(P.astype(np.float64), normals=Nr.astype(np.float64) / (1 << 14))
    assert np.array_equal(hip.snap_normals(cloud.normals), Nr)
    with pytest.raises(ValueError, match="would fit"):
        hip.ball_pivot(P, Nr, [hip.RECON_MAX_RHO2 + 1])
    with pytest.raises(ValueError, match="a quantum of 4.0 would fit"):
        TriangleMesh.create_from_point_cloud_ball_pivoting(cloud, [100.0, 5000.0], quantum=2.0)
    with pytest.raises(ValueError, match="no normals"):
        TriangleMesh.create_from_point_cloud_ball_pivoting(PointCloud(P.astype(np.float64)), [700.0])
    with pytest.raises(ValueError, match="power of two"):
        TriangleMesh.create_from_point_cloud_ball_pivoting(cloud, [700.0], quantum=3.0)
    with pytest.raises(ValueError, match="below the quantum"):
        TriangleMesh.create_from_point_cloud_ball_pivoting(cloud, [0.5, 700.0], quantum=1.0)
    with pytest.raises(ValueError, match="shape"):
        hip.ball_pivot(P, Nr[:-1], rho2)
    with pytest.raises(ValueError, match="integers"):
        hip.ball_pivot(P.astype(np.float64), Nr, rho2)
    assert issubclass(hip.BallPivotRefused, ValueError) and issubclass(hip.BallPivotRefused, _lib.PyQSMHipError)
    err = hip.BallPivotRefused(-4, "refused")
    assert err.code == -4 and "refused" in str(err)
    # fewer than three points: no triangle and no device
    mesh = TriangleMesh.create_from_point_cloud_ball_pivoting(
        PointCloud(np.zeros((2, 3)) + [[0.0], [1.0]], normals=np.tile([0.0, 0.0, 1.0], (2, 1))), [0.5])
    assert mesh.triangles.shape == (0, 3) and mesh.triangle_levels.shape == (0,) and mesh.n_unresolved_ties == 0


def test_vertex_normals_are_area_weighted():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 1], [9, 9, 9]], np.float64)
    m = TriangleMesh(v, [[0, 1, 2], [0, 3, 1]]).compute_vertex_normals()
    # areas 2 (normal +z) and 1 (normal +y... of (0,3,1): (0,0,1) x (2,0,0) = (0, 2, 0))
    assert np.allclose(m.triangle_normals, [[0, 0, 1], [0, 1, 0]])
    assert np.allclose(m.vertex_normals[0], np.array([0, 2, 4]) / np.sqrt(20))
    assert np.allclose(m.vertex_normals[2], [0, 0, 1]) and np.allclose(m.vertex_normals[3], [0, 1, 0])
    assert np.allclose(m.vertex_normals[4], [0, 0, 1])                   # no triangle: Open3D's default


def test_integer_predicate_under_the_sanitizers():
    """recon_exact.hpp as a stand-alone host program under ASan and UBSan (csrc/Makefile: recon_check):
    host code only, built and run on the CPU."""
    if _lib.device_count() > 0:
        pytest.skip("sanitizer runs belong on machines without a GPU")
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "pyqsm_amd", "csrc"), "recon_check"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "recon_check: ok" in out.stdout
    # the fp64 filter against the integers: both signs taken, a hand-over that was used, no disagreement
    counts = re.search(r"filter: (\d+) inside, (\d+) outside, (\d+) undecided, (\d+) exact ties among them, "
                       r"0 disagreements", out.stdout)
    assert counts, out.stdout
    inside, outside, undecided, ties = map(int, counts.groups())
    assert inside + outside + undecided >= 1_000_000 and min(inside, outside) > 0 and undecided >= ties > 100_000


# ---- the tie-dense inputs of tests/test_gpu_recon.py (tests/recon_cases.py): each has, on the CPU, the
# property its GPU test depends on, and a reference within the library's triangle cap

def test_cases_snap_normals_as_the_binding_does():
    assert C.NORMAL_SCALE == hip.RECON_NORMAL_SCALE
    v = np.random.default_rng(0).normal(size=(50, 3))
    assert np.array_equal(C.snap(v), hip.snap_normals(v / np.linalg.norm(v, axis=1, keepdims=True)))
    assert max(r for _, radii in C.TIE_TABLE for r in radii) == C.R2_CUBE <= hip.RECON_MAX_RHO2
    assert C.R2_CUBE < C.R2_TOP <= hip.RECON_MAX_RHO2


@pytest.mark.parametrize("pitch,radii", C.TIE_TABLE)
def test_tie_lattices_tie_and_fit_the_cap(pitch, radii):
    off_plane = second_level = 0
    for key in C.tie_lattice_keys():
        if key[2] != pitch:
            continue
        P, Nr, rho2 = C.tie_lattice(*key)
        seed, m, _, _, flat = key
        assert rho2 == radii and P.shape == (C.N_TIE_LATTICE, 3) and P.dtype == np.int32 and Nr.dtype == np.int16
        sites = (P.astype(np.int64) - P.min(axis=0)) // pitch
        assert np.array_equal(sites * pitch, P.astype(np.int64) - P.min(axis=0)) and sites.max() <= m - 1
        assert np.abs(P).max() <= (1 << 20) + (m - 1) * pitch
        assert len(np.unique(P, axis=0)) < len(P)                        # coincident points
        if flat:
            assert max(np.bincount(sites[:, 2])) >= len(P) // 2 - 3      # half the cloud in one plane, but for copies
        axis = (np.abs(Nr.astype(np.int64)).max(axis=1) == C.NORMAL_SCALE) & ((Nr != 0).sum(axis=1) == 1)
        assert axis.sum() >= 5
        assert C.perpendicular_normals(P, Nr, max(rho2)) > 0             # da == 0 in recon_pair
        T, lv, unresolved = C.reference("tie_lattice", *key)
        coplanar, off = C.census("tie_lattice", *key)
        assert 0 < len(T) <= C.triangle_cap(len(P)) and coplanar > 0
        assert (unresolved > 0) == (off > 0)
        off_plane += off
        second_level += int((lv > 0).sum())
    assert off_plane > 0 and second_level > 0


@pytest.mark.parametrize("r2", sorted(C.SPHERE_POINTS))
def test_lattice_spheres_are_cospherical(r2):
    assert len(C.sphere_points(r2)) == C.SPHERE_POINTS[r2]               # the counts csrc/recon_check.cpp finds
    centre = C.lattice_sphere_centre(r2)
    for inward in (True, False):
        P, Nr, rho2 = C.lattice_sphere(r2, 18, inward)
        Q = P.astype(np.int64) - centre
        assert rho2 == (r2,) and len(np.unique(P, axis=0)) == 18 and ((Q * Q).sum(axis=1) == r2).all()
        assert (((Q * Nr).sum(axis=1) < 0) == inward).all()
        T, lv, unresolved = C.reference("lattice_sphere", r2, 18, inward)
        assert 0 < len(T) <= 816 <= C.triangle_cap(18)
        if inward:      # every triple rests on the sphere itself, and every other point ties
            assert unresolved == len(T) >= 800 and sum(C.census("lattice_sphere", r2, 18, inward)) >= 15 * len(T)
    big = C.lattice_sphere(C.R2_CUBE, 30, True)[0]
    assert len(np.unique(big, axis=0)) == 30 and 30 * 29 * 28 // 6 > 3 * C.triangle_cap(30)


def test_rectangle_has_its_ball_centre_in_the_plane():
    for height, sign in ((50, 1), (50, -1), (49, 1), (49, -1)):
        P, Nr, rho2 = C.rectangle_h0(height)
        Pl = R.as_ints(P)
        for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3), (0, 2, 1)):
            assert R.setup(Pl[i], Pl[j], Pl[k], rho2[0])["H"] == 0
        t = R.setup(Pl[0], Pl[1], Pl[2], rho2[0])
        assert R.classify(t, Pl[3]) == R.TIE_COPLANAR
        assert R.classify(t, Pl[4]) == (R.TIE_OFF_PLANE if height == 50 else R.INSIDE)
        T, lv, unresolved = R.brute(P, sign * Nr, rho2)
        in_plane = [row for row in T.tolist() if 4 not in row]
        # with the tie off the plane both diagonals stay and are counted; with the point inside no
        # triangle of the rectangle alone is left
        assert (len(in_plane), unresolved > 0) == ((4, True) if height == 50 else (0, False))


def test_dense_box_fills_chunks_and_slices():
    P, Nr, rho2 = C.dense_box()
    assert len(P) == 1100 > hip.RECON_CHUNK and len(np.unique(P, axis=0)) == 1090
    assert P.min() == 0 and P.max() == 11 and rho2 == (1, 2)
    edge = int(np.ceil(2 * np.sqrt(max(rho2)))) + 1                      # 4: three cells per axis
    cells = np.unique(P // edge, axis=0, return_counts=True)[1]
    assert edge == 4 and len(cells) == 27 and cells.min() > hip.RECON_SLICE
    T, lv, unresolved = C.reference("dense_box")
    assert 1000 < len(T) <= C.triangle_cap(len(P)) and unresolved > 100 and (lv == 1).sum() > 0


@pytest.mark.parametrize("low", C.FAR_LOWS)
def test_far_apart_spans_the_int32_range(low):
    P, Nr, rho2 = C.far_apart(low)
    assert P.dtype == np.int32 and int(P[:, 0].min()) == low and int(P[:, 0].max()) == low + (1 << 31) - 1
    assert low >= -(1 << 31) and np.abs(P[:, 1:].astype(np.int64)).max() < 1 << 21
    halves = [C.tie_lattice(*k)[0] for k in C.FAR_HALVES]
    assert np.array_equal(P[:36, 1:], halves[0][:, 1:]) and np.array_equal(P[36:, 1:], halves[1][:, 1:])   # x only
    assert np.array_equal(np.diff(P[:36, 0].astype(np.int64)), np.diff(halves[0][:, 0].astype(np.int64)))
    ref, want = C.reference("far_apart", low), C.far_apart_from_halves()
    assert np.array_equal(ref[0], want[0]) and np.array_equal(ref[1], want[1]) and ref[2] == want[2] > 0
    assert (ref[0] < 36).all(axis=1).any() and (ref[0] >= 36).all(axis=1).any()
    # one unit more on that axis is refused. The span is measured per axis, as the library does: a y or z
    # above zero lies more than 2^31 above the lowest x of the cloud from INT32_MIN, and that is no span.
    wide = P.copy()
    wide[np.argmax(P[:, 0]), 0] += 1
    with pytest.raises(ValueError, match="spans more than 2\\^31"):
        hip.ball_pivot(wide, Nr, rho2)
