"""DBSCAN's profiling timers on device-clock stamps (common.hpp: stamped, StampScope): the step's
phases and its three timed kernels are measured from per-block stamps, not from events between the
kernels. Profiling changes nothing in the results, every timer counts one launch per step, the
phases are positive, disjoint and inside dbscan_total. Also: cells of more than 255 points, which
the bucket sort now orders itself (grid.hip: k_bk_sort), with profiling on and off."""
import os

import numpy as np
import pytest

import oracle
from pyqsm_amd import hip, synth

pytestmark = pytest.mark.gpu

PHASES = ("dbscan_bin", "dbscan_core", "dbscan_union", "dbscan_label")
KERNELS = ("k_core_tiled", "k_hook_sub", "k_union_sub")


def _steps(P, eps, min_pts, gpu, steps, prof):
    """Labels, core flags and the timers of `steps` calls of the device entry point."""
    n = P.shape[0]
    d_xyz = hip.DeviceBuffer.from_array(np.ascontiguousarray(P, dtype=np.float64), device=gpu)
    d_lab = hip.DeviceBuffer(n * 8, gpu)
    d_core = hip.DeviceBuffer(n, gpu)
    hip.prof_enable(prof, gpu)
    hip.prof_reset(gpu)
    for _ in range(steps):
        hip.dbscan_dev(d_xyz.ptr, n, eps, min_pts, d_lab.ptr, d_core.ptr, gpu)
    timers = {k: hip.prof_get(k, gpu) for k in PHASES + KERNELS + ("dbscan_total", "dbscan_plan_hit",
                                                                   "dbscan_plan_miss")}
    hip.prof_enable(False, gpu)
    return d_lab.download((n,), np.int64), d_core.download((n,), np.uint8), timers


def test_timers_on_the_forest(gpu):
    P = synth.forest(200_000, seed=5)
    _steps(P, 0.1, 10, gpu, 2, False)  # a hint for this shape: the timed calls below are hits
    lab0, core0, _ = _steps(P, 0.1, 10, gpu, 1, False)
    steps = 4
    lab, core, t = _steps(P, 0.1, 10, gpu, steps, True)
    assert np.array_equal(lab, lab0) and np.array_equal(core, core0)
    assert t["dbscan_plan_hit"][1] == steps
    for k in PHASES + KERNELS + ("dbscan_total",):
        assert t[k][1] == steps, k
        assert t[k][0] > 0, k
    phases = sum(t[k][0] for k in PHASES)
    assert phases <= t["dbscan_total"][0] * (1 + 1e-9)
    assert t["k_core_tiled"][0] <= t["dbscan_core"][0]
    assert t["k_hook_sub"][0] + t["k_union_sub"][0] <= t["dbscan_union"][0]


def test_miss_then_hit_with_profiling(gpu, monkeypatch):
    """A missed speculation records its (empty) scopes as well: two of each per miss."""
    rng = np.random.default_rng(41)
    P = np.concatenate([rng.uniform(0, 1, (20_000, 3)), rng.uniform(5, 6, (5_000, 3))])
    P = P.astype(np.float32).astype(np.float64)
    lab0, core0 = oracle.dbscan(P, 0.05, 5)
    monkeypatch.setenv("PYQSM_DBSCAN_PLAN", "host")  # a small hint first
    _steps(np.array([[0.0, 0.0, 0.0], [0.0625, 0.0, 0.0], [0.0, 0.0625, 0.0]]), 0.1, 2, gpu, 1, False)
    monkeypatch.delenv("PYQSM_DBSCAN_PLAN")
    lab, core, t = _steps(P, 0.05, 5, gpu, 1, True)  # the hint is too small: a miss
    assert np.array_equal(lab, lab0) and np.array_equal(core.astype(bool), core0)
    assert t["dbscan_plan_miss"][1] == 1
    for k in PHASES:
        assert t[k][1] == 2 and t[k][0] > 0, k
    assert t["dbscan_total"][1] == 1
    assert sum(t[k][0] for k in PHASES) <= t["dbscan_total"][0] * (1 + 1e-9)
    lab, core, t = _steps(P, 0.05, 5, gpu, 1, True)  # the same shape again: a hit
    assert np.array_equal(lab, lab0) and np.array_equal(core.astype(bool), core0)
    assert t["dbscan_plan_hit"][1] == 1
    for k in PHASES + KERNELS:
        assert t[k][1] == 1 and t[k][0] > 0, k


@pytest.mark.parametrize("prof", [False, True])
def test_cells_above_255_points(gpu, prof):
    """Dense blobs put thousands of points into single cells: the bucket sort orders them by octant
    itself (no k_order_big launch). Planned on the host, then on the device."""
    rng = np.random.default_rng(77 + prof)
    blobs = [c + rng.uniform(0, 0.08, (m, 3)) for c, m in (((0, 0, 0), 3000), ((1, 0, 0), 700), ((0, 1, 0), 256))]
    P = np.concatenate(blobs + [rng.uniform(-1, 2, (4000, 3))])
    P = P[rng.permutation(len(P))].astype(np.float32).astype(np.float64)
    lab0, core0 = oracle.dbscan(P, 0.1, 10)
    for _ in range(2):  # miss (host plan), then hit (device plan)
        lab, core, _ = _steps(P, 0.1, 10, gpu, 1, prof)
        assert np.array_equal(lab, lab0) and np.array_equal(core.astype(bool), core0)
