"""The alpha-area contract on the CPU (tests/alpha_restatement.py): the directed-edge rule over all
points, the same rule over the candidates within 2 alpha, and scipy's Delaunay triangulation with
an exact circumradius filter give the same twice-area and the same boundary edges; the host side of
pyqsm_amd.viz.projection (quantize_plane) is exact on lattice input."""
import numpy as np
import pytest

from pyqsm_amd.viz import projection as pj
from tests import alpha_restatement as R

CASES = [(name, k) for name in R.SMALL_GROUPS for k in range(3)]


@pytest.mark.parametrize("name,k", CASES)
def test_three_statements_agree(name, k):
    make, a2s = R.SMALL_GROUPS[name]
    P, A2 = make(), a2s[k]
    b, l, d = R.brute(P, A2), R.local(P, A2), R.delaunay_filtered(P, A2)
    assert b == l == d
    assert R.degrees_balanced(b[1])
    if k == 0:
        assert b == (0, [])                  # an alpha that keeps nothing
    if k == 1:
        full = R.brute(P, a2s[2])[0]
        assert 0 < b[0] < full               # a part
    if k == 2:
        from scipy.spatial import ConvexHull
        assert b[0] == round(2 * ConvexHull(P.astype(np.float64)).volume)   # everything: the hull


def test_cocircular_cell_is_one_cell():
    """At A2 = R^2 exactly the twelve-gon is kept whole (inclusive bound), at R^2 - 1 it is not: the
    two results differ by its area and by nothing else."""
    P = R.cocircular()
    gon = sum(int(P[i, 0]) * int(P[(i + 1) % 12, 1]) - int(P[i, 1]) * int(P[(i + 1) % 12, 0]) for i in range(12))
    at, below = R.brute(P, 65000 ** 2), R.brute(P, 65000 ** 2 - 1)
    assert at[0] - below[0] == gon


def test_big_cloud_local_equals_delaunay():
    P, A2 = R.big_cloud(), R.big_cloud_a2()
    l, d = R.local(P, A2), R.delaunay_filtered(P, A2)
    assert l == d and l[0] > 0
    assert R.degrees_balanced(l[1])


def test_dense_cloud_triangulation_is_pinned():
    """The GPU test of the dense cloud compares against the Delaunay filter at an alpha at which the
    rule itself is too slow in Python; the triangulation does not depend on alpha, so the rule pins it here
    at a small one."""
    P = R.dense_cloud()
    l, d = R.local(P, 40), R.delaunay_filtered(P, 40)
    assert l == d and l[0] > 0
    big = R.delaunay_filtered(P, 150 ** 2)
    assert big[0] > l[0] and R.degrees_balanced(big[1])


def test_inclusive_bound_on_even_pitch_lattice():
    m, s = 6, 4
    P = R.square_lattice(m, s)
    assert R.brute(P, s * s // 2)[0] == 2 * ((m - 1) * s) ** 2   # every cell: R^2 = s^2 / 2 exactly
    assert R.brute(P, s * s // 2 - 1) == (0, [])
    assert R.local(P, s * s // 2) == R.brute(P, s * s // 2)


def test_annulus_has_two_loops():
    P = R.annulus()
    A2 = 2 * 3 * 3           # keeps the unit squares of pitch 3 (R^2 = 4.5) and nothing across the hole
    tw, boundary = R.local(P, A2)
    assert (tw, boundary) == R.delaunay_filtered(P, A2)
    assert len(R.loops(boundary)) == 2


def test_quantize_plane_is_exact_on_lattice_input():
    rng = np.random.default_rng(0)
    ij0 = rng.integers(0, 1000, size=(200, 2))
    q = 2.0 ** -7
    pts = np.concatenate([(ij0 + 12345) * q, rng.normal(size=(200, 1))], axis=1)
    ij, q1 = pj.quantize_plane(pts, quantum=q)
    assert q1 == q and ij.dtype == np.int32
    assert np.array_equal(ij, ij0 - ij0.min(axis=0))
    again, _ = pj.quantize_plane(np.concatenate([ij * q, np.zeros((200, 1))], axis=1), quantum=q)
    assert np.array_equal(again, ij)                                   # idempotent


def test_quantize_plane_default_quantum():
    pts = np.array([[0.0, 0.0, 1.0], [30.0, 12.0, 5.0], [7.3, 29.9, 2.0]])
    ij, q = pj.quantize_plane(pts)
    assert q == 2.0 ** -15                                             # a 30 m crown: 0.03 mm
    assert ij.max() <= 1 << 20 and ij.min() == 0
    assert np.array_equal(ij, np.rint(pts[:, :2] / q).astype(np.int64))
    one, q1 = pj.quantize_plane(np.array([[1.0, 2.0, 3.0]]))
    assert q1 == 1.0 and np.array_equal(one, [[0, 0]])
    exact, q2 = pj.quantize_plane(np.array([[0.0, 0.0, 0.0], [32.0, 1.0, 0.0]]))
    assert q2 == 2.0 ** -15 and exact.max() == 1 << 20                  # extent / q == 2^20 is allowed


def test_quantize_plane_alone_and_in_a_batch():
    rng = np.random.default_rng(1)
    a, b = rng.normal(size=(50, 3)) * 3 + 100, rng.normal(size=(70, 3)) - 40
    q = 2.0 ** -12
    both, _ = pj.quantize_plane(np.concatenate([a, b]), quantum=q, seg_start=[0, 50, 120])
    assert np.array_equal(both[:50], pj.quantize_plane(a, quantum=q)[0])
    assert np.array_equal(both[50:], pj.quantize_plane(b, quantum=q)[0])
    tilted, _ = pj.quantize_plane(np.concatenate([a, b]), normal=(1, 2, 3), quantum=q, seg_start=[0, 50, 120])
    assert np.array_equal(tilted[50:], pj.quantize_plane(b, normal=(1, 2, 3), quantum=q)[0])


def test_quantize_plane_refuses_bad_input():
    bad = np.zeros((4, 3))
    bad[2, 1] = np.nan
    with pytest.raises(ValueError):
        pj.quantize_plane(bad)
    bad[2, 1] = np.inf
    with pytest.raises(ValueError):
        pj.quantize_plane(bad)
    with pytest.raises(ValueError):
        pj.quantize_plane(np.zeros((4, 3)), quantum=0.3)
    with pytest.raises(ValueError):
        pj.quantize_plane(np.array([[0.0, 0, 0], [100.0, 0, 0]]), quantum=2.0 ** -20)   # 1e8 lattice units


def test_alpha_must_be_positive():
    pts = np.random.default_rng(2).normal(size=(10, 3))
    for alpha in (0, -1.0, None, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            pj.projected_area(pts, alpha)
