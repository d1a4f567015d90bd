"""Point-to-mesh distance (a10: `mri`, ray_casting.py:237-260 -> compute_signed_distance):
HIP kernel against the CPU mirror oracle (bit-exact: same fp32 operation sequence), against the
INDEPENDENT fp64 references of oracle/meshdist_f64.c (distance, closest triangle, inside/outside
sign by winding number; families and bounds in tests/meshdist_cases.py) and analytic cases.
Open3D is not installable, so parity with its implementation is unpinned."""
import numpy as np
import pytest

import oracle
from pyqsm_amd import hip, synth
from pyqsm_amd.viz.ray_casting import RaycastingScene, get_points_inside_mesh, mri
from tests import meshdist_cases as mc

pytestmark = pytest.mark.gpu

CUBE_V, CUBE_T = mc.CUBE_V, mc.CUBE_T


@pytest.mark.parametrize("n_tris,n_q", [(1, 1), (7, 63), (2000, 5000), (20_000, 40_000)])
def test_matches_oracle_bit_for_bit(gpu, n_tris, n_q):
    verts, tris = synth.canopy_mesh(max(n_tris, 2), seed=n_tris, side=0.4)
    tris = tris[:n_tris]
    rng = np.random.default_rng(n_q)
    q = rng.uniform(verts.min(0) - 1, verts.max(0) + 1, (n_q, 3)).astype(np.float32)
    q[: min(n_q, len(verts))] = verts[: min(n_q, len(verts))]          # some queries ON vertices
    d, p = hip.point_mesh_distance(verts, tris, q, device=gpu)
    d0, p0 = oracle.point_mesh_distance(verts, tris, q)
    assert np.array_equal(d, d0) and np.array_equal(p, p0)
    assert d[: min(n_q, 3 * n_tris)].min() == 0.0


@pytest.mark.parametrize("name", list(mc.DISTANCE_FAMILIES))
def test_families_match_oracle_bit_for_bit_and_fp64(gpu, name):
    """Every family: bit-equal to the mirror (distance and lowest-index closest triangle), and
    within the bounds of the independent fp64 evaluation — the check the mirror cannot give."""
    v, t, q, _, _ = mc.distance_case(name)
    d, p = hip.point_mesh_distance(v, t, q, device=gpu)
    d0, p0 = oracle.point_mesh_distance(v, t, q)
    assert np.array_equal(d, d0) and np.array_equal(p, p0)
    mc.check_distance(name, d, p)


@pytest.mark.parametrize("n_q", [255, 256, 257, 513])
def test_query_counts_around_the_block(gpu, n_q):
    """Q on both sides of the 256-thread block, on a mesh with every kind of triangle."""
    v, t = mc.mixed_mesh()
    q = np.random.default_rng(n_q).uniform(-2, 2, (n_q, 3)).astype(np.float32)
    q[-1] = v[t[-1, 0]]                                    # the last lane of the last block, ON a vertex
    d, p = hip.point_mesh_distance(v, t, q, device=gpu)
    d0, p0 = oracle.point_mesh_distance(v, t, q)
    assert np.array_equal(d, d0) and np.array_equal(p, p0)
    d64, _ = oracle.point_mesh_distance_f64(v, t, q)
    assert d[-1] == 0.0
    assert (np.abs(d - d64) <= mc.T_RTOL * np.maximum(d64, mc.NEAR * mc.diagonal(v))).all()


@pytest.mark.parametrize("name", list(mc.SIGN_FAMILIES))
def test_signed_distance_against_winding_number(gpu, name):
    """compute_signed_distance < 0 exactly where the fp64 winding number says inside, on every
    query further than 1e-4 * diag from the surface; |signed| == compute_distance bit for bit;
    get_points_inside_mesh shares the occupancy."""
    v, t, q, _, _ = mc.sign_case(name)
    scene = RaycastingScene(gpu)
    scene.add_triangles((v, t))
    sd, d = scene.compute_signed_distance(q), scene.compute_distance(q)
    mc.check_sign(name, sd, d)
    inside = get_points_inside_mesh((v, t), q, device=gpu) > 0.5
    assert np.array_equal(inside[d > 0], sd[d > 0] < 0)       # (a query ON the surface: -0.0 or 0.0)


def test_cube_known_answers_and_sign(gpu):
    scene = RaycastingScene(gpu)
    scene.add_triangles((CUBE_V, CUBE_T))
    q = np.array([[0.5, 0.375, 0.5], [0.5, 0.375, 2.0], [2, 2, 2], [0.5, 0.375, 0.875], [-1, 0.375, 0.5],
                  [0.25, 0.375, 0.5]], np.float32)
    d = scene.compute_distance(q)
    assert np.allclose(d, [0.375, 1.0, np.sqrt(3), 0.125, 1.0, 0.25], rtol=1e-6)
    sd = scene.compute_signed_distance(q)
    assert np.allclose(sd, [-0.375, 1.0, np.sqrt(3), -0.125, 1.0, -0.25], rtol=1e-6)
    # y == z: an axis-aligned parity ray from these runs through the diagonal shared by the two
    # triangles of a face (counted twice by an edge-inclusive test); the occupancy ray is generic
    q = np.array([[0.5, 0.5, 0.5], [0.25, 0.375, 0.375], [0.5, 0.75, 0.75], [-1, 0.5, 0.5], [0.5, 2, 2],
                  [0.125, 0.125, 0.125], [1.5, 0.25, 0.25]], np.float32)
    sd = scene.compute_signed_distance(q)
    assert np.allclose(sd, [-0.5, -0.25, -0.25, 1.0, np.sqrt(2), -0.125, 0.5], rtol=1e-6)
    assert np.array_equal(np.abs(sd), scene.compute_distance(q))
    # shapes follow the input (Open3D convention)
    lattice = np.zeros((4, 5, 6, 3), np.float32) + 0.5
    assert scene.compute_signed_distance(lattice).shape == (4, 5, 6)


def test_mri_returns_the_fields_the_reference_plots(gpu):
    pts, sd, lattice, sd_grid = mri((CUBE_V, CUBE_T), grid=16, device=gpu)
    assert pts.shape == (256, 3) and sd.shape == (256,)
    assert (sd <= 0).mean() > 0.95            # bounding box of the cube = the cube
    assert lattice.shape == (16, 16, 16, 3) and sd_grid.shape == (16, 16, 16)
    assert abs(sd_grid).max() <= 0.5 + 1e-6
    # every strictly interior lattice point is negative, nothing is positive beyond 1e-6 (the
    # lattice points ON the faces are at distance 0 with either sign)
    interior = ((lattice > 0) & (lattice < 1)).all(-1)
    assert interior.sum() == 14 ** 3 and (sd_grid[interior] < 0).all()
    assert sd_grid.max() <= 1e-6 and sd.max() <= 1e-6
    assert np.array_equal(lattice.reshape(-1, 3), mc.box_lattice(CUBE_V, 16))


def test_empty_mesh_and_bad_indices(gpu):
    from pyqsm_amd._lib import PyQSMHipError
    d, p = hip.point_mesh_distance(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32),
                                   np.zeros((3, 3), np.float32), device=gpu)
    assert np.isinf(d).all() and (p == 0xFFFFFFFF).all()
    with pytest.raises(PyQSMHipError):
        hip.point_mesh_distance(CUBE_V, np.array([[0, 1, 99]], np.int32), np.zeros((1, 3), np.float32),
                                device=gpu)
