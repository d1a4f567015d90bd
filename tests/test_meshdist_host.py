"""The MIRROR oracle of point-to-mesh distance (oracle.point_mesh_distance: the fp32 operation
sequence of meshdist.hip) and the crossing parity along the wrapper's occupancy direction
(oracle.list_intersections, the mirror of the all-hits kernel) against the independent fp64
references of oracle/meshdist_f64.c, on the families of tests/meshdist_cases.py. No GPU: the GPU
tests hold the kernels bit-equal to these mirrors, so what is wrong here is wrong there.

Measured on the CPU (max |d - d64| / max(d64, 0.05 * diag) per family, bound 1e-5): the figures
are printed by every case; DESIGN.md "parity status" keeps the table."""
import numpy as np
import pytest

import oracle
from pyqsm_amd.viz import ray_casting as rc

from tests import meshdist_cases as mc


def test_fp64_references_on_known_answers():
    """The references themselves, against answers known in closed form."""
    q = np.array([[0.5, 0.375, 0.5], [0.5, 0.375, 2.0], [2, 2, 2], [0.5, 0.5, 0.5], [-1, 0.5, 0.5],
                  [0.25, 0.25, 0.25], [1.5, 1.5, 0.5]], np.float32)
    d, p = oracle.point_mesh_distance_f64(mc.CUBE_V, mc.CUBE_T, q)
    assert np.allclose(d, [0.375, 1.0, np.sqrt(3), 0.5, 1.0, 0.25, np.sqrt(0.5)], rtol=0, atol=1e-15)
    assert p.dtype == np.int64 and ((p >= 0) & (p < 12)).all()
    assert np.array_equal(oracle.point_tri_pairs_f64(mc.CUBE_V, mc.CUBE_T, q, p), d)
    wn = oracle.inside_closed_mesh_f64(mc.CUBE_V, mc.CUBE_T, q)
    assert np.allclose(np.abs(wn), [1, 0, 0, 1, 0, 1, 0], atol=1e-12)
    # a single triangle: above the interior, beyond an edge, beyond a vertex; zero-area triangles
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [1, 0, 0]], np.float32)
    q = np.array([[0.5, 0.5, 3], [1, -2, 0], [-3, -4, 0], [2, 2, 0]], np.float32)
    for tri in ([0, 1, 2], [1, 2, 0], [2, 1, 0]):
        d, _ = oracle.point_mesh_distance_f64(v, np.array([tri], np.int32), q)
        assert np.allclose(d, [3, 2, 5, np.sqrt(2)], rtol=0, atol=1e-15)
    for tri in ([0, 3, 1], [0, 1, 1], [0, 0, 1], [1, 0, 1]):                # the segment (0,0,0)-(2,0,0)
        d, _ = oracle.point_mesh_distance_f64(v, np.array([tri], np.int32), q)
        assert np.allclose(d, [np.sqrt(0.25 + 9), 2, 5, 2], rtol=0, atol=1e-15)
    d, _ = oracle.point_mesh_distance_f64(v, np.array([[3, 3, 3]], np.int32), q)
    assert np.allclose(d, np.linalg.norm(q.astype(np.float64) - [1, 0, 0], axis=1), rtol=0, atol=1e-15)
    d, p = oracle.point_mesh_distance_f64(v, np.zeros((0, 3), np.int32), q)
    assert np.isinf(d).all() and (p == -1).all()
    # the winding number does not depend on a ray: a non-convex solid, both arms and the notch
    lv, lt = mc.l_prism()
    q = np.array([[1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [1.5, 1.5, 0.5], [0.5, 0.5, 0.5], [3, 3, 3]], np.float32)
    assert np.allclose(oracle.inside_closed_mesh_f64(lv, lt, q), [1, 1, 0, 1, 0], atol=1e-12)
    sv, st = mc.uv_sphere(12, 16, 0.7, (3, -2, 5), mc.fixed_rotation())
    q = np.array([[3, -2, 5], [3.3, -2.2, 5.1], [3, -2, 5.9]], np.float32)
    assert np.allclose(oracle.inside_closed_mesh_f64(sv, st, q), [1, 1, 0], atol=1e-12)


@pytest.mark.parametrize("name", list(mc.DISTANCE_FAMILIES))
def test_mirror_distance_against_fp64(name):
    v, t, q, _, _ = mc.distance_case(name)
    d, p = oracle.point_mesh_distance(v, t, q)
    mc.check_distance(name, d, p)


@pytest.mark.parametrize("name", list(mc.SIGN_FAMILIES))
def test_mirror_parity_sign_against_winding_number(name):
    v, t, q, _, _ = mc.sign_case(name)
    d, _ = oracle.point_mesh_distance(v, t, q)
    counts = oracle.list_intersections(v, t, rc.occupancy_rays(q))["counts"]
    signed = np.where(counts % 2 == 1, -d, d).astype(np.float32)
    mc.check_sign(name, signed, d)
