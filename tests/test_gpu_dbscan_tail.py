"""The tail of the DBSCAN step (dbscan.hip): sub-cell representatives, roots, cluster numbering and
labels. Up to kRankCap (4096) clusters one workgroup numbers them; beyond it a bitmap of the
components' smallest indices does, whatever their count. Labels, core flags and the cluster count
of the device entry point are checked on both sides of that capacity, on long sub-cell runs, on a
plan miss followed by a hit and on the doubled-cell path."""
import numpy as np
import pytest

import oracle
from pyqsm_amd import hip

pytestmark = pytest.mark.gpu

RANK_CAP = 4096


def _count(P, eps, min_pts, gpu):
    """The device entry point's cluster count, its labels and core flags."""
    n = P.shape[0]
    d_xyz = hip.DeviceBuffer.from_array(np.ascontiguousarray(P, dtype=np.float64), device=gpu)
    d_lab = hip.DeviceBuffer(n * 8, device=gpu)
    d_core = hip.DeviceBuffer(n, device=gpu)
    cnt = hip.dbscan_dev(d_xyz.ptr, n, eps, min_pts, d_lab.ptr, d_core.ptr, gpu, want_count=True)
    return cnt, d_lab.download((n,), np.int64), d_core.download((n,), np.uint8).astype(bool)


def _check(P, eps, min_pts, gpu, want=None):
    lab0, core0 = oracle.dbscan(P, eps, min_pts)
    lab, core = hip.dbscan(P, eps, min_pts, device=gpu)
    assert np.array_equal(core, core0)
    assert np.array_equal(lab, lab0)
    cnt, lab_d, core_d = _count(P, eps, min_pts, gpu)
    assert np.array_equal(lab_d, lab0) and np.array_equal(core_d, core0)
    assert cnt == lab0.max() + 1 if lab0.size else cnt == 0
    if want is not None:
        assert cnt == want
    return cnt


def _pairs(k, seed):
    """k clusters of two points each (min_pts = 2), far apart on a shuffled lattice, plus noise."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(k ** (1 / 3))) + 1
    cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = cells[rng.permutation(len(cells))[:k]] * 0.5
    a = centres + rng.uniform(0, 0.03, (k, 3))
    b = a + rng.uniform(-0.04, 0.04, (k, 3))
    noise = cells[rng.permutation(len(cells))[:200]] * 0.5 + 0.25  # between the pairs, 0.5 apart
    P = np.concatenate([a, b, noise]).astype(np.float32).astype(np.float64)
    return P[rng.permutation(len(P))]


@pytest.mark.parametrize("k", [0, 1, 2, RANK_CAP - 1, RANK_CAP, RANK_CAP + 1])
def test_cluster_counts_around_the_workgroup_capacity(gpu, k):
    P = _pairs(k, 100 + k)
    _check(P, 0.1, 2, gpu, want=k)


def test_min_pts_1_sparse_cloud(gpu):
    """About one cluster per point: the bitmap numbering."""
    rng = np.random.default_rng(31)
    P = rng.uniform(0, 10, (30_000, 3))
    cnt = _check(P, 0.05, 1, gpu)
    assert cnt > 25_000


def test_one_cluster_per_point_beyond_a_prefix_round(gpu):
    """600 k isolated points (a shuffled lattice, eps below its spacing) with min_pts = 1: every point
    is its own cluster, numbered by its index — more bitmap words than one round of the prefix covers."""
    rng = np.random.default_rng(32)
    side = 85
    g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3)
    P = g[rng.permutation(len(g))[:600_000]]
    n = P.shape[0]
    cnt, lab, core = _count(P, 0.5, 1, gpu)
    assert cnt == n
    assert core.all()
    assert np.array_equal(lab, np.arange(n))


def test_long_runs_with_late_core_points(gpu):
    """Dense clumps of 70-300 points (sub-cell runs longer than a wave, starting anywhere in one) in
    sparse halos, with min_pts near the clump sizes: the first core point of a run lies anywhere in it."""
    rng = np.random.default_rng(33)
    parts = []
    for _ in range(40):
        c = rng.uniform(0, 4, 3)
        parts.append(c + rng.uniform(0, 0.04, (rng.integers(70, 300), 3)))
        parts.append(c + rng.uniform(-0.1, 0.14, (rng.integers(5, 60), 3)))
    parts.append(rng.uniform(0, 4, (3000, 3)))
    P = np.concatenate(parts)
    P = P[rng.permutation(len(P))]
    for min_pts in (1, 20, 90, 160, 260, 330):
        _check(P, 0.1, min_pts, gpu)


def test_plan_miss_then_hit(gpu, monkeypatch):
    """The first call on a new shape plans on the host, the next one runs on the device's plan."""
    P = _pairs(RANK_CAP + 300, 34)

    def run():
        hip.prof_enable(True, gpu)
        hip.prof_reset(gpu)
        cnt, lab, core = _count(P, 0.1, 2, gpu)
        hit = hip.prof_get("dbscan_plan_hit", gpu)[1]
        hip.prof_enable(False, gpu)
        return cnt, lab, core, hit

    lab0, core0 = oracle.dbscan(P, 0.1, 2)
    monkeypatch.setenv("PYQSM_DBSCAN_PLAN", "host")  # a small hint first: three points planned on the host
    _count(np.array([[0.0, 0.0, 0.0], [0.0625, 0.0, 0.0], [0.0, 0.0625, 0.0]]), 0.1, 2, gpu)
    monkeypatch.delenv("PYQSM_DBSCAN_PLAN")
    paths = []
    for _ in range(2):
        cnt, lab, core, hit = run()
        assert np.array_equal(lab, lab0) and np.array_equal(core, core0)
        assert cnt == RANK_CAP + 300
        paths.append(hit)
    assert paths == [0, 1]


@pytest.mark.parametrize("groups,min_pts", [(800, 2), (5000, 2), (5000, 4)])
def test_doubled_cell_path(gpu, monkeypatch, groups, min_pts):
    """Groups along the space diagonal occupy so many slabs per axis that the grid doubles its
    cells: the per-point union-find, the same numbering. (Planned on the host: a speculative step
    that leaves without work would still count its k_hook_sub launch.)"""
    monkeypatch.setenv("PYQSM_DBSCAN_PLAN", "host")
    rng = np.random.default_rng(36 + groups + min_pts)
    eps = 0.1
    centres = np.cumsum(rng.uniform(0.6, 2.0, groups) * eps)[:, None] * [1.0, 1.0, 1.0]
    sizes = rng.integers(1, 6, groups)
    P = np.concatenate([c + rng.uniform(0, 0.3 * eps, (s, 3)) for c, s in zip(centres, sizes)])
    P = P[rng.permutation(len(P))]
    hip.prof_enable(True, gpu)
    hip.prof_reset(gpu)
    _check(P, eps, min_pts, gpu)
    hooks = hip.prof_get("k_hook_sub", gpu)[1]
    hip.prof_enable(False, gpu)
    assert hooks == 0  # not the sub-cell path
