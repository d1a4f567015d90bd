"""DBSCAN's grid planned on the device (dbscan.hip, grid.hip: plan_grid_device): the step is
enqueued behind the bounding box with the shapes of the last host-planned call and runs when the
device's plan fits them (a hit); otherwise it is planned on the host (a miss). Either way labels
and core flags are those of the oracle and of PYQSM_DBSCAN_PLAN=host, and the counters
dbscan_plan_hit / dbscan_plan_miss say which path ran."""
import os

import numpy as np
import pytest

import oracle
from pyqsm_amd import hip, synth
from pyqsm_amd._lib import PyQSMHipError

pytestmark = pytest.mark.gpu


def _run(P, eps, min_pts, gpu, host=False, radius_inclusive=True):
    """(labels, core, 'hit' | 'miss') of one call on the calling thread's context."""
    old = os.environ.pop("PYQSM_DBSCAN_PLAN", None)
    if host:
        os.environ["PYQSM_DBSCAN_PLAN"] = "host"
    try:
        hip.prof_enable(True, gpu)
        hip.prof_reset(gpu)
        lab, core = hip.dbscan(P, eps, min_pts, device=gpu, radius_inclusive=radius_inclusive)
        hit = hip.prof_get("dbscan_plan_hit", gpu)[1]
        miss = hip.prof_get("dbscan_plan_miss", gpu)[1]
        hip.prof_enable(False, gpu)
    finally:
        os.environ.pop("PYQSM_DBSCAN_PLAN", None)
        if old is not None:
            os.environ["PYQSM_DBSCAN_PLAN"] = old
    assert hit + miss == 1
    return lab, core, "hit" if hit else "miss"


def _prime_small_hint(gpu):
    """A host-planned call on a tiny cloud (fp32-representable, so that it makes a hint): the
    context's hint is then a small directory."""
    P = np.array([[0.0, 0.0, 0.0], [0.0625, 0.0, 0.0], [0.0, 0.0625, 0.0]])
    assert _run(P, 0.1, 2, gpu, host=True)[2] == "miss"


def _expect(P, eps, min_pts, gpu, paths, radius_inclusive=True):
    """Calls in a row on one cloud, each checked against the oracle and the host-planned path."""
    lab0, core0 = oracle.dbscan(P, eps, min_pts, radius_inclusive=radius_inclusive)
    lab_h, core_h, _ = _run(P, eps, min_pts, gpu, host=True, radius_inclusive=radius_inclusive)
    assert np.array_equal(lab_h, lab0) and np.array_equal(core_h, core0)
    got = []
    for _ in paths:
        lab, core, path = _run(P, eps, min_pts, gpu, radius_inclusive=radius_inclusive)
        assert np.array_equal(core, core0)
        assert np.array_equal(lab, lab0)
        got.append(path)
    assert got == list(paths)
    return lab0, core0


def test_repeated_calls_miss_once_then_hit(gpu):
    _prime_small_hint(gpu)
    P = synth.forest(50_000)
    lab0, core0 = oracle.dbscan(P, 0.1, 10)
    paths = []
    for _ in range(4):
        lab, core, path = _run(P, 0.1, 10, gpu)
        assert np.array_equal(lab, lab0) and np.array_equal(core, core0)
        paths.append(path)
    assert paths == ["miss", "hit", "hit", "hit"]


def test_larger_extent_misses_once(gpu):
    _prime_small_hint(gpu)
    small = synth.forest(20_000) * 0.5
    large = synth.forest(20_000) * 2.0
    _expect(small, 0.1, 10, gpu, ["hit", "hit"])   # the host-planned call in _expect made the hint
    _prime_small_hint(gpu)
    lab0, core0 = oracle.dbscan(small, 0.1, 10)
    lab, core, path = _run(small, 0.1, 10, gpu)
    assert path == "miss" and np.array_equal(lab, lab0) and np.array_equal(core, core0)
    lab0, core0 = oracle.dbscan(large, 0.1, 10)
    for want in ("miss", "hit"):
        lab, core, path = _run(large, 0.1, 10, gpu)
        assert path == want and np.array_equal(lab, lab0) and np.array_equal(core, core0)
    # the larger hint covers the smaller cloud
    lab, core, path = _run(small, 0.1, 10, gpu)
    assert path == "hit"


def test_fp32_cloud_then_non_representable(gpu):
    P = synth.forest(30_000)
    _expect(P, 0.1, 10, gpu, ["hit", "hit"])
    Q = P + 1e-9                                          # not exactly representable in fp32
    assert not np.array_equal(Q.astype(np.float32).astype(np.float64), Q)
    _expect(Q, 0.1, 10, gpu, ["miss", "miss"])            # fp64 records: always planned on the host
    _expect(P, 0.1, 10, gpu, ["hit"])


def test_axis_mapped_cloud_after_the_forest(gpu):
    P = synth.forest(30_000)
    _expect(P, 0.1, 10, gpu, ["hit", "hit"])
    rng = np.random.default_rng(11)
    blob = rng.uniform(0, 0.6, (6000, 3))
    far = rng.uniform(-50, 50, (40, 3))
    Q = np.concatenate([blob, far]).astype(np.float32).astype(np.float64)
    _expect(Q, 0.03, 4, gpu, ["miss", "miss"])            # compressed axes: planned on the host
    _expect(P, 0.1, 10, gpu, ["hit"])                     # the forest's hint is still there


def test_cells_of_more_than_255_points(gpu):
    rng = np.random.default_rng(3)
    P = rng.uniform(0, 0.15, (8000, 3)).astype(np.float32).astype(np.float64)
    P = np.concatenate([P, rng.uniform(0.5, 1.0, (2000, 3)).astype(np.float32).astype(np.float64)])
    _expect(P, 0.1, 10, gpu, ["hit", "hit"])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_sizes_around_a_wave_and_a_tile(gpu, n):
    rng = np.random.default_rng(n)
    P = rng.uniform(0, 0.4, (n, 3)).astype(np.float32).astype(np.float64)
    _expect(P, 0.05, 3, gpu, ["hit", "hit"])


def test_non_finite_after_a_hit(gpu):
    P = synth.forest(20_000)
    lab0, core0 = _expect(P, 0.1, 10, gpu, ["hit", "hit"])
    Q = P.copy()
    Q[123, 2] = np.nan
    with pytest.raises(PyQSMHipError) as e:
        hip.dbscan(Q, 0.1, 10, device=gpu)
    assert e.value.code == -1                             # PYQSM_EINVAL
    Q[123, 2] = np.inf
    with pytest.raises(PyQSMHipError):
        hip.dbscan(Q, 0.1, 10, device=gpu)
    lab, core, path = _run(P, 0.1, 10, gpu)               # the library is still usable
    assert path == "hit" and np.array_equal(lab, lab0) and np.array_equal(core, core0)


@pytest.mark.parametrize("radius_inclusive", [True, False])
def test_radius_inclusive_both_ways(gpu, radius_inclusive):
    # a lattice of spacing eps: neighbours lie exactly at eps, where the two forms differ
    g = np.arange(12) * 0.125
    P = np.stack(np.meshgrid(g, g, g[:6], indexing="ij"), -1).reshape(-1, 3)
    P = np.concatenate([P, P[::7] + 0.0625])
    lab0, core0 = _expect(P, 0.125, 7, gpu, ["hit", "hit"], radius_inclusive=radius_inclusive)
    other = oracle.dbscan(P, 0.125, 7, radius_inclusive=not radius_inclusive)
    assert not np.array_equal(core0, other[1])            # the case at hand is sensitive to it


def test_want_count(gpu):
    P = synth.forest(50_000)
    lab0, core0 = oracle.dbscan(P, 0.1, 10)
    n = P.shape[0]
    d_xyz = hip.DeviceBuffer.from_array(P, gpu)
    d_lab = hip.DeviceBuffer(n * 8, gpu)
    d_core = hip.DeviceBuffer(n, gpu)
    _prime_small_hint(gpu)
    for want in ("miss", "hit", "hit"):
        hip.prof_enable(True, gpu)
        hip.prof_reset(gpu)
        cnt = hip.dbscan_dev(d_xyz.ptr, n, 0.1, 10, d_lab.ptr, d_core.ptr, gpu, want_count=True)
        hit = hip.prof_get("dbscan_plan_hit", gpu)[1]
        hip.prof_enable(False, gpu)
        assert ("hit" if hit else "miss") == want
        assert cnt == lab0.max() + 1
        assert np.array_equal(d_lab.download((n,), np.int64), lab0)
        assert np.array_equal(d_core.download((n,), np.uint8).astype(bool), core0)
