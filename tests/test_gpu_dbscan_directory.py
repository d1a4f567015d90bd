"""DBSCAN's ranked cell directory on the GPU (grid.hpp: CellDir; grid.hip: k_bk_sort, k_dir_from_dense).

Label equality alone cannot see a directory that is too generous (a begin that is too small for an
empty cell only lengthens a run), so every cloud is checked twice in every mode: the directory the
device evaluates, ``hip.octant_directory``, against ``np.searchsorted`` over the cell ids that
tests/grid_restatement.py::dbscan_plan computes, entry by entry, and ``hip.dbscan`` against
``oracle.dbscan``. Integers throughout: ``array_equal``, no tolerance. The modes: planned on the host,
planned on the device (a hit where the grid is of the plannable kind), fp64 records
(PYQSM_COORD_F32=0), and the binning that still counts into a dense array and converts it
(PYQSM_DBSCAN_BIN=atomic). The clouds and what each one claims (word and bucket edges, the
directory's end, every path of the producer, buckets of 8192 cells, compressed axes, doubled cells,
tiny clouds) are tests/directory_restatement.py's; the claims are recomputed here."""
import functools
import os

import numpy as np
import pytest

import oracle
from pyqsm_amd import hip
from pyqsm_amd._lib import PyQSMHipError
from tests import directory_restatement as D

pytestmark = pytest.mark.gpu

ENV = ("PYQSM_DBSCAN_PLAN", "PYQSM_COORD_F32", "PYQSM_DBSCAN_BIN")
# name -> (PYQSM_DBSCAN_PLAN, PYQSM_COORD_F32, PYQSM_DBSCAN_BIN)
MODES = {"host": ("host", None, None), "device": (None, None, None), "fp64": (None, "0", None),
         "atomic": (None, None, "atomic")}


def _call(fn, gpu, mode):
    """fn() under the mode's switches; (result, 'hit' | 'miss')."""
    keep = {k: os.environ.pop(k, None) for k in ENV}
    for k, v in zip(ENV, MODES[mode]):
        if v is not None:
            os.environ[k] = v
    try:
        hip.prof_enable(True, gpu)
        hip.prof_reset(gpu)
        out = fn()
        hit = hip.prof_get("dbscan_plan_hit", gpu)[1]
        miss = hip.prof_get("dbscan_plan_miss", gpu)[1]
        hip.prof_enable(False, gpu)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert hit + miss == 1
    return out, "hit" if hit else "miss"


@functools.lru_cache(maxsize=None)
def _expected(name):
    """(oracle labels, oracle core flags, dense directory or None), computed once per cloud."""
    P, _ = D.cloud(name)
    eps, min_pts, read, _ = D.CLOUDS[name]
    lab, core = oracle.dbscan(P, eps, min_pts)
    pl = D.plan(name)
    start = D.dense(pl.cells, pl.ncell).astype(np.int32) if read else None
    for a in (lab, core, start):
        if a is not None:
            a.setflags(write=False)
    return lab, core, start


@pytest.mark.parametrize("name", list(D.CLOUDS))
def test_directory_and_labels_in_every_mode(gpu, name):
    pl = D.claim(name)
    P, _ = D.cloud(name)
    eps, min_pts, read, plannable = D.CLOUDS[name]
    lab0, core0, start0 = _expected(name)
    n = len(P)
    for mode in MODES:
        # (the device mode follows the host mode on the same cloud: the hint is this cloud's)
        want = "hit" if mode == "device" and plannable else "miss"
        if read:
            (dims, begin), path = _call(lambda: hip.octant_directory(P, eps, device=gpu), gpu, mode)
            assert path == want, (mode, "directory")
            assert tuple(dims.tolist()) == pl.dims, mode
            assert begin[-1] == n and begin[0] == 0, mode
            bad = np.flatnonzero(begin != start0)
            assert bad.size == 0, (mode, bad[:8], begin[bad[:8]], start0[bad[:8]])
        (lab, core), path = _call(lambda: hip.dbscan(P, eps, min_pts, device=gpu), gpu, mode)
        assert path == want, (mode, "labels")
        assert np.array_equal(core, core0), mode
        assert np.array_equal(lab, lab0), mode


def test_directory_larger_than_the_caller_allows_is_refused(gpu):
    P, _ = D.cloud("end_0")
    with pytest.raises(PyQSMHipError) as e:
        hip.octant_directory(P, D.EPS, device=gpu, cap=4096)     # 4097 entries
    assert e.value.code == -4                                    # PYQSM_ERANGE
    dims, begin = hip.octant_directory(P, D.EPS, device=gpu, cap=4097)
    assert tuple(dims.tolist()) == (16, 16, 16) and len(begin) == 4097 and begin[-1] == len(P)
