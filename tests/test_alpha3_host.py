"""The 3-D alpha-shape contract on the CPU (tests/alpha3_restatement.py): the brute-force definition and the
Delaunay route agree and reproduce the table the contract was settled on, the fixtures of the GPU tests have
the properties they are for, and the host side of the wrappers (snapping, refusals, the binding's constants,
the sanitizer program of the two-sided predicate) holds without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry import hull
from pyqsm_amd.geometry.cloud import PointCloud, TriangleMesh
from tests import alpha3_restatement as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("key", sorted(A.TABLE))
def test_brute_force_equals_delaunay_route_and_the_table(key):
    seed, n, ext, rho2 = key
    P = A.table_cloud(seed, n, ext)
    assert len(P) == n                                                   # no coincident draws in these clouds
    rows, vol6, unresolved = A.table_reference(key)
    d_rows, d_vol6 = A.delaunay(P, rho2)
    regular = rows[rows[:, 3] == A.REGULAR]
    assert np.array_equal(regular, d_rows) and unresolved == 0
    assert vol6 == d_vol6                                                # the oriented rows enclose the tetrahedra
    assert (len(regular), int((rows[:, 3] == A.SINGULAR).sum()), vol6[0]) == A.TABLE[key]
    assert (rows[:, 0] < rows[:, 1]).all() and (rows[:, 0] < rows[:, 2]).all()
    sing = rows[rows[:, 3] == A.SINGULAR]
    assert (sing[:, 1] < sing[:, 2]).all()
    # every edge of the regular set has as many triangles one way as the other: it closes
    half = [(int(t[k]), int(t[(k + 1) % 3])) for t in regular for k in range(3)]
    assert sorted(half) == sorted((v, u) for u, v in half)
    only_regular = A.brute(P, rho2, faces="regular")
    assert np.array_equal(only_regular[0], regular) and only_regular[1] == vol6


def test_sphere_has_sheets_only():
    """300 points on a sphere of radius 1000 units, alpha = 500: no tetrahedron is kept, so nothing is regular,
    and a ball rests on every facet of the sphere from either side: 2 V - 4 singular triangles, the cocircular
    polygons of the lattice sphere cut into fans."""
    P = A.sphere_points()
    assert len(np.unique(P, axis=0)) == len(P) == 300
    assert (((P.astype(np.int64) - 1000) ** 2).sum(axis=1) == A.R2_SPHERE).all()
    rows, vol6, unresolved = A.brute(P, 500 * 500)
    assert (rows[:, 3] == A.REGULAR).sum() == 0 and vol6 == [0] and unresolved == 0
    assert len(rows) == 2 * len(P) - 4
    assert len(A.brute(P, 500 * 500, faces="regular")[0]) == 0
    edges = {}
    for t in rows[:, :3].tolist():
        for k in range(3):
            e = tuple(sorted((t[k], t[(k + 1) % 3])))
            edges[e] = edges.get(e, 0) + 1
    assert set(edges.values()) == {2} and len(edges) == 3 * len(P) - 6   # a closed triangulation of the sphere


@pytest.mark.parametrize("pitch", (1, 7))
def test_tie_lattices_have_coplanar_and_off_plane_ties(pitch):
    small, large = A.tie_radii(pitch)
    assert 4 * small >= 3 * pitch * pitch > 4 * (small - 1) and large == 3 * pitch * pitch
    P = A.tie_lattice(pitch)
    assert P.shape == (27, 3) and P.min() == 0 and P.max() == 2 * pitch
    coplanar, off = A.tie_census(P, large)          # the box's own circumsphere passes through its corners
    assert coplanar > 0 and off > 0
    assert A.tie_census(P, small)[0] > 0
    for r2 in (small, large):
        rows, vol6, _ = A.brute(P, r2)
        # the box is one solid: eight triangles on each face of 2 x 2 squares, and its volume
        assert (rows[:, 3] == A.REGULAR).sum() == 48 and vol6 == [6 * (2 * pitch) ** 3]
    moved = A.tie_lattice(pitch, perm_seed=5, shift=(-(1 << 31), 17, (1 << 31) - 1 - 2 * pitch))
    assert moved.dtype == np.int32 and moved[:, 0].min() == -(1 << 31) and moved[:, 2].max() == (1 << 31) - 1
    # the fan rule follows the numbering, so a permuted lattice cuts its squares elsewhere: the same solid
    rows, vol6, _ = A.brute(moved, large)
    assert (rows[:, 3] == A.REGULAR).sum() == 48 and vol6 == [6 * (2 * pitch) ** 3]
    shifted = A.tie_lattice(pitch, shift=(-(1 << 31), 17, (1 << 31) - 1 - 2 * pitch))
    assert np.array_equal(A.brute(shifted, large)[0], A.brute(P, large)[0])


def test_cube_corners_are_kept_and_counted():
    """The eight corners of a cube at its circumradius: every ball that is empty has the other corners exactly
    on it, off the plane of the triple."""
    P = A.cube_corners()
    rows, vol6, unresolved = A.brute(P, A.cube_rho2())
    assert unresolved > 0 and unresolved == len(rows)


def test_cospherical_set_exceeds_the_row_cap():
    P = A.cospherical_set()
    assert len(P) == 40 and len(np.unique(P, axis=0)) == 40
    rows, _, unresolved = A.brute(P, A.R2_SPHERE)
    assert (rows[:, 3] == A.REGULAR).sum() > 16 * len(P) + 1024 and unresolved == len(rows)


def test_nested_shells_reach_every_kernel_class():
    P, rho2 = A.nested_shells()
    edge = int(np.ceil(2 * np.sqrt(rho2))) + 1
    assert 2900 < len(P) <= 3000 and len(np.unique(P, axis=0)) == len(P)
    cells, counts = np.unique(P // edge, axis=0, return_counts=True)
    assert (cells.max(axis=0) == 3).all() and cells.min() == 0          # four cells per axis
    assert len(cells) < 64                                               # empty cells
    assert counts.max() > 4 * hip.ALPHA3_SLICE                           # more than one work item per cell
    d2 = ((P[:, None, :].astype(np.int64) - P[None, :, :]) ** 2).sum(axis=2)
    assert ((d2 <= 4 * rho2).sum(axis=1) - 1).max() > hip.ALPHA3_CHUNK   # a neighbour list of several chunks
    rows, vol6 = A.nested_shells_reference()
    assert 1000 < len(rows) <= 16 * len(P) + 1024 and vol6[0] > 0


def test_solid_fixture_closes():
    """The 400-point solid of the wrapper test: its regular set, by the Delaunay route, is a closed surface."""
    pts, alpha, q = A.solid_cloud()
    ijk, q2, rho2 = hull.snap_for_radius(pts, alpha)
    assert q2 == q and np.array_equal(ijk * q + pts.min(axis=0), pts)        # the points are lattice points
    rows, vol6 = A.delaunay(ijk, rho2)
    edges = {}
    for t in rows[:, :3].tolist():
        for k in range(3):
            edges[(t[k], t[(k + 1) % 3])] = edges.get((t[k], t[(k + 1) % 3]), 0) + 1
    assert set(edges.values()) == {1} and all((v, u) in edges for u, v in edges)


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "pyqsm_hip.h")).read()

    def macro(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))

    assert hip.ALPHA3_CHUNK == macro("PYQSM_ALPHA3_CHUNK")
    assert hip.ALPHA3_SLICE == macro("PYQSM_ALPHA3_SLICE")
    assert hip.ALPHA3_DEFAULT_MAX_TESTS == macro("PYQSM_ALPHA3_DEFAULT_MAX_TESTS")
    assert (macro("PYQSM_ALPHA3_REGULAR"), macro("PYQSM_ALPHA3_ALL")) == (0, 1)
    assert (hip.ALPHA3_REGULAR, hip.ALPHA3_SINGULAR) == (A.REGULAR, A.SINGULAR) == (1, 2)


def test_host_side_refusals_and_snapping():
    P = A.table_cloud(0, 70, 100)
    with pytest.raises(ValueError, match="would fit"):
        hip.alpha_shape3(P, hip.RECON_MAX_RHO2 + 1)
    with pytest.raises(ValueError, match="positive"):
        hip.alpha_shape3(P, 0)
    with pytest.raises(ValueError, match="faces"):
        hip.alpha_shape3(P, 900, faces="singular")
    with pytest.raises(ValueError, match="integers"):
        hip.alpha_shape3(P.astype(np.float64), 900)
    with pytest.raises(ValueError, match="shape"):
        hip.alpha_shape3(P[:, :2], 900)
    with pytest.raises(ValueError, match="seg_start"):
        hip.alpha_shape3(P, 900, seg_start=[0, 80, 70])
    wide = P.copy()
    wide[0, 0], wide[1, 0] = -(1 << 31), (1 << 31) - 1
    with pytest.raises(ValueError, match="spans more than 2\\^31"):
        hip.alpha_shape3(wide, 900)
    assert issubclass(hip.AlphaShapeRefused, ValueError) and issubclass(hip.AlphaShapeRefused, _lib.PyQSMHipError)
    err = hip.AlphaShapeRefused(-4, "refused")
    assert err.code == -4 and "refused" in str(err)

    pts = P.astype(np.float64)
    # the default quantum: the larger of extent / 2^20 and the smallest at which alpha <= 2^11 units
    ijk, q, rho2 = hull.snap_for_radius(pts, 30.0)
    assert q == 2.0 ** -6 and rho2 == (30 * 64) ** 2 and np.array_equal(ijk, (P - P.min(axis=0)) * 64)
    ijk, q, rho2 = hull.snap_for_radius(pts, 5000.0)
    assert q == 4.0 and rho2 == 1250 ** 2
    ijk, q, rho2 = hull.snap_for_radius(pts, 30.5, quantum=1.0)
    assert q == 1.0 and rho2 == 930 and np.array_equal(ijk, P - P.min(axis=0))      # floor(30.5^2)
    with pytest.raises(ValueError, match="a quantum of 4.0 would fit"):
        hull.snap_for_radius(pts, 5000.0, quantum=2.0)
    with pytest.raises(ValueError, match="power of two"):
        hull.snap_for_radius(pts, 30.0, quantum=3.0)
    with pytest.raises(ValueError, match="below the quantum"):
        hull.snap_for_radius(pts, 0.5, quantum=1.0)
    with pytest.raises(ValueError, match="positive"):
        hull.alpha_shape(pts, -1.0)
    with pytest.raises(ValueError, match="finite"):
        hull.alpha_shape(np.array([[0.0, 0.0, np.nan]] * 4), 1.0)

    # fewer than three points: nothing, and no device
    for n in (0, 2):
        res = hip.alpha_shape3(P[:n], 900, faces="all")
        assert res.rows.shape == (0, 4) and res.rows.dtype == np.int32 and res.vol6 == [0]
        assert all(v == 0 for v in res.stats.values())
    shape = hull.alpha_shape(pts[:2], 30.0, quantum=1.0)
    assert shape.triangles.shape == (0, 3) and shape.kinds.shape == (0,) and len(shape.vertices) == 0
    assert (shape.volume, shape.area, shape.n_unresolved_ties, shape.quantum) == (0.0, 0.0, 0, 1.0)
    mesh = TriangleMesh.create_from_point_cloud_alpha_shape(PointCloud(pts[:2]), 30.0, None, None, 1.0)
    assert mesh.triangles.shape == (0, 3) and len(mesh.vertices) == 2 and mesh.volume == 0.0
    both = hull.alpha_shapes(pts[:4], [0, 2, 2, 4], 30.0, quantum=1.0)
    assert [len(s.triangles) for s in both] == [0, 0, 0] and [len(s.points) for s in both] == [2, 0, 2]


def test_two_sided_predicate_under_the_sanitizers():
    """alpha3_exact.hpp as a stand-alone host program under ASan and UBSan (csrc/Makefile: alpha3_check): host
    code only, built and run on the CPU."""
    if _lib.device_count() > 0:
        pytest.skip("sanitizer runs belong on machines without a GPU")
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "pyqsm_amd", "csrc"), "alpha3_check"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "alpha3_check: ok" in out.stdout
    counts = re.search(r"filter: (\d+) inside, (\d+) outside, (\d+) undecided, (\d+) exact ties among them, "
                       r"0 disagreements", out.stdout)
    assert counts, out.stdout
    inside, outside, undecided, ties = map(int, counts.groups())
    # two sides per test: a million random configurations and the tie families
    assert inside + outside + undecided >= 2_000_000 and min(inside, outside) > 0 and undecided >= ties > 50_000
