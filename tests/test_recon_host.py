"""The ball-pivoting contract on the CPU (tests/recon_restatement.py): the brute-force definition and the
Delaunay route agree on the clouds in general position the GPU tests use, the degenerate fixtures give
what the issue's trial gave, and the host side of the wrappers (snapping, refusals, vertex normals, the
binding's constants, the sanitizer program of the integer predicate) holds without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry.cloud import PointCloud, TriangleMesh
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
