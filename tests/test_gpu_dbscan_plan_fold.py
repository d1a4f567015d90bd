"""DBSCAN's speculated step has no fold launch: k_bbox clears the binning's counters, every block of k_bk_hist
folds k_bbox's records and plans the grid for itself, and one more block stores the plan for the later kernels
and the host (grid.hip: fold_box_records, PlanFold). A step without a shape hint, or planned on the host, still
runs the one-block fold. Every path here, at sizes around the blocks of both kernels: labels and core flags
against the CPU oracle, the plan counters against what the case must take, and the directory after a
speculated call against the one NumPy builds (tests/grid_restatement.py, as tests/test_gpu_dbscan_directory.py)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from pyqsm_amd import hip
from pyqsm_amd._lib import PyQSMHipError
from tests import directory_restatement as D
from tests import grid_restatement as G
from tests import plan_fold_cases as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, MIN_PTS = F.EPS, F.MIN_PTS


@functools.lru_cache(maxsize=None)
def _cloud(n):
    P = F.cloud(n)
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def _expected(n, variant="fp32"):
    """Oracle labels and core flags of the size's cloud, or of it with one coordinate that is no fp32 value."""
    P = _cloud(n) if variant == "fp32" else _not_fp32(n)
    lab, core = oracle.dbscan(P, EPS, MIN_PTS)
    lab.setflags(write=False)
    core.setflags(write=False)
    return lab, core


def _not_fp32(n):
    Q = _cloud(n).copy()
    Q[n // 2, 1] = np.nextafter(Q[n // 2, 1], np.inf)     # (the next double after a float is no float)
    assert np.float64(np.float32(Q[n // 2, 1])) != Q[n // 2, 1]
    return Q


def _dbscan(P, gpu, want, expected, what):
    (lab, core), hit, miss = F.counted(lambda: hip.dbscan(P, EPS, MIN_PTS, device=gpu), gpu)
    assert (hit, miss) == ((1, 0) if want == "hit" else (0, 1)), what
    assert np.array_equal(core, expected[1]), what
    assert np.array_equal(lab, expected[0]), what


@pytest.mark.parametrize("n", F.SIZES)
def test_every_plan_path(gpu, monkeypatch, n):
    P = _cloud(n)
    exp = _expected(n)
    pl, tiny = G.dbscan_plan(P, EPS), G.dbscan_plan(F.TINY, EPS)
    assert not pl.mapped and not pl.doubled and pl.bits == 12
    monkeypatch.setenv("PYQSM_DBSCAN_PLAN", "host")
    _dbscan(P, gpu, "miss", exp, "planned on the host")
    hip.dbscan(F.TINY, EPS, 2, device=gpu)                       # ... which leaves the smallest hint there is
    monkeypatch.delenv("PYQSM_DBSCAN_PLAN")
    # the box outgrows the hint (a sixteenth of headroom); a single point never does
    outgrows = pl.ncell > tiny.ncell + tiny.ncell // 16
    assert outgrows == (n > 1)
    _dbscan(P, gpu, "miss" if outgrows else "hit", exp, "a box that outgrows the hint")
    _dbscan(P, gpu, "hit", exp, "speculated")
    (dims, begin), hit, miss = F.counted(lambda: hip.octant_directory(P, EPS, device=gpu), gpu)
    assert (hit, miss) == (1, 0)
    assert tuple(dims.tolist()) == pl.dims
    assert np.array_equal(begin, D.dense(pl.cells, pl.ncell))
    _dbscan(_not_fp32(n), gpu, "miss", _expected(n, "not fp32"), "a coordinate that is no fp32 value")
    _dbscan(P, gpu, "hit", exp, "speculated again")
    bad = P.copy()
    bad[n // 3, 2] = np.nan
    with pytest.raises(PyQSMHipError) as e:
        hip.dbscan(bad, EPS, MIN_PTS, device=gpu)
    assert e.value.code == -1 and "finite" in str(e.value)      # PYQSM_EINVAL
    _dbscan(P, gpu, "hit", exp, "after the refused call")


def test_first_calls_of_new_contexts(gpu):
    """No hint: k_bbox and the fold kernel, planned on the host; the second call is speculated. (A process of
    its own: tests/plan_fold_cases.py says why.)"""
    flags = ["-s"] if sys.flags.no_user_site else []        # (as this interpreter was started)
    r = subprocess.run([sys.executable, *flags, "-m", "tests.plan_fold_cases"], cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [row["n"] for row in rows] == list(F.SIZES)
    for row in rows:
        first, second = row["calls"]
        assert first == {"hit": 0, "miss": 1, "equal": True}, row
        assert second == {"hit": 1, "miss": 0, "equal": True}, row
