"""The kNN engine (knn.hip: knn_device) on coordinates that are NOT fp32-representable: the fp64-array
storage form that the contraction loop always runs, through every kernel class, the tie passes, the
retry levels and both ways of making a retry grid. Every comparison is np.array_equal on both d2 and
idx against oracle.knn (ties broken by index on both sides).

The inputs are those of tests/knn_cases.py, whose properties tests/test_knn_cases_host.py proves on
the CPU. PYQSM_KNN_TRACE says, per level, the grid, how it was made, the storage form and the kernel:
each test asserts the path it believes it ran."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle
from pyqsm_amd import hip, synth
from pyqsm_amd.geometry import skeletonize as sk

from tests import knn_cases as kc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = "fp32 records", "fp64 arrays"
LEVEL = re.compile(r"knn level (\d+): grid (\d+) x (\d+) x (\d+) of cell (\S+?)( binned again| coarsened)?, "
                   r"(fp32 records|fp64 arrays), (\S+), (\d+) queries(, last level)?\n")
TIES = re.compile(r"knn level 0: (\d+) queries searched again for a tie at the k-th place")


def kernel_of(k, level=0, variant="4,true"):
    """The kernel knn_device picks (knn.hip: pick_kernel, buffer slots and the strict first pass of the
    register kernel included; kernel_name prints it)."""
    if level == 0 and k <= 32:
        return f"k_knn_reg<{(k + 3) // 4 * 4},{variant}>"
    if level > 0 and k <= 64:
        return "k_knn_wave"
    return f"k_knn<{256 if k <= 48 else 128 if k <= 96 else 64}>"


@pytest.fixture
def traced(gpu, monkeypatch, capfd):
    """search(P, k, excl) -> (idx, d2, levels, stderr); levels: one dict per level that ran."""
    monkeypatch.setenv("PYQSM_KNN_TRACE", "1")

    def search(P, k, excl=True):
        capfd.readouterr()
        idx, d2 = hip.knn(P, k, excl, device=gpu)
        err = capfd.readouterr().err
        levels = [dict(level=int(m[1]), cells=int(m[2]) * int(m[3]) * int(m[4]), cell=float(m[5]),
                       made=(m[6] or "").strip(), storage=m[7], kernel=m[8], queries=int(m[9]), last=bool(m[10]))
                  for m in LEVEL.finditer(err)]
        # levels count up from 0; level 0 may run twice (knn.hip: most queries open after the first pass)
        assert levels and [lv["level"] for lv in levels] in (list(range(len(levels))),
                                                            [0] + list(range(len(levels) - 1))), err
        print(err, end="")
        return idx, d2, levels, err
    return search


def records_fit(cells):
    """grid.hip: bucketed_fits. The two-level sort, and with it the fp32 records, take directories of
    up to 16 384 buckets of 2^12 cells (2^13 beyond 2^26 cells); a larger grid keeps fp64 arrays."""
    bits = 12 if cells + 1 <= 16384 << 12 else 13
    return (cells + (1 << bits)) >> bits <= 16384


def storage_by_level(levels, representable):
    """What every level must hold: fp64 arrays for coordinates no float holds; else fp32 records where
    build_grid's sort has them, and whatever the fine grid held where the grid was derived from it."""
    out = []
    for lv in levels:
        if lv["made"] == "coarsened":
            out.append(out[-1])
        else:
            out.append(F32 if representable and records_fit(lv["cells"]) else F64)
    return out


def assert_equal(got, want, what):
    assert np.array_equal(got[1], want[1]), what       # d2, bit for bit
    assert np.array_equal(got[0], want[0]), what       # idx, ties by index


# ---- a. level 0, every kernel class, fp64 storage ------------------------------------------------

@pytest.mark.parametrize("excl", [True, False])
@pytest.mark.parametrize("k", kc.LEVEL0_KS)
def test_level0_kernels_on_fp64_arrays(traced, k, excl):
    idx, d2, levels, _ = traced(kc.offgrid(5000), k, excl)
    assert levels[0]["storage"] == F64 and levels[0]["kernel"] == kernel_of(k)
    assert levels[0]["queries"] == 5000
    assert_equal((idx, d2), kc.expected("offgrid", 5000, k=k, exclude_self=excl), (k, excl))


# ---- b. the storage form changes no bit ----------------------------------------------------------

@pytest.mark.parametrize("k", [8, 20, 33, 64, 150])
@pytest.mark.parametrize("name,args", [("forest", (5000,)), ("lattice", ())])
def test_storage_form_changes_no_bit(traced, monkeypatch, name, args, k):
    P = kc.cloud(name, *args)
    idx, d2, levels, _ = traced(P, k)
    assert all(lv["storage"] == F32 for lv in levels)
    monkeypatch.setenv("PYQSM_COORD_F32", "0")          # read per call (grid.hip: build_grid)
    idx1, d21, levels1, _ = traced(P, k)
    assert all(lv["storage"] == F64 for lv in levels1)
    assert [lv["kernel"] for lv in levels] == [lv["kernel"] for lv in levels1]
    assert_equal((idx1, d21), (idx, d2), (name, k))
    assert_equal((idx, d2), kc.expected(name, *args, k=k), (name, k))


# ---- c. ties at the k-th place in fp64 -----------------------------------------------------------

def tie_count(err):
    """The tie list's length after the pass of level 0 that answered (the last one, if it ran twice)."""
    found = TIES.findall(err)
    assert found, err
    return int(found[-1])


@pytest.mark.parametrize("k", kc.FEW_TIES_KS)
def test_few_ties_take_the_wave_tie_pass(traced, k):
    P = kc.few_ties()
    idx, d2, levels, err = traced(P, k)
    assert levels[0]["storage"] == F64 and levels[0]["kernel"] == kernel_of(k)
    assert 0 < tie_count(err) <= len(P) // 16
    assert_equal((idx, d2), kc.expected("few_ties", k=k), k)


@pytest.mark.parametrize("k", kc.MANY_TIES_KS)
def test_many_ties_take_the_per_lane_pass_over_the_list(traced, k):
    """Five or six points on each node of a 9 x 9 x 9 lattice of 0.1 steps; the oracle ties at the k-th
    place for 3 382 (k = 8) and 3 670 (k = 20) of the 4 000 queries.

    This is the input that showed level 0 answering nobody: knn_device aims at k / 3 points per occupied
    cell, a node already holds 5.5, so at k = 20 the cell edge stays at ext / 64 = 0.0125, an eighth of
    the lattice step, three rings reach no other node, 4 000 of 4 000 queries stayed open and a wave per
    query answered the whole cloud at level 1 (bit-equal, 0 queries on the tie list). knn_device now
    runs level 0 once more on the 4x coarser grid when more than half of all queries stay open; the
    count asserted here is that pass's. At k = 8 (cell edge 0.003) the 864 queries on nodes with more
    than eight points end at level 0 and 423 of them tie."""
    P = kc.many_ties()
    idx, d2, levels, err = traced(P, k)
    assert levels[0]["storage"] == F64 and levels[0]["kernel"] == kernel_of(k)
    assert_equal((idx, d2), kc.expected("many_ties", k=k), k)
    print(f"many_ties k={k}: {tie_count(err)} queries on the tie list, n // 16 = {len(P) // 16}")
    assert tie_count(err) > len(P) // 16
    if k == 20:
        assert [lv["level"] for lv in levels[:2]] == [0, 0] and levels[1]["kernel"] == kernel_of(k)
        assert levels[1]["queries"] == len(P) and levels[1]["made"] == "coarsened"


@pytest.mark.parametrize("k", kc.SPREAD_TIES_KS)
def test_spread_ties_take_the_per_lane_pass_over_the_list(traced, k):
    """One point per lattice node: the first grid answers every query, so the tie list of its strict
    pass is as long as the oracle's tie count says."""
    P = kc.spread_ties()
    idx, d2, levels, err = traced(P, k)
    assert levels[0]["storage"] == F64 and levels[0]["kernel"] == kernel_of(k)
    assert tie_count(err) > len(P) // 16
    assert_equal((idx, d2), kc.expected("spread_ties", k=k), k)


# ---- d. retry levels in fp64, k <= 64 ------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 20, 64])
def test_few_strays_are_searched_one_by_one_on_fp64_arrays(traced, k):
    """test_few_far_outliers_are_searched_one_by_one off the fp32 lattice, at its 60 000 points: the
    grids are built over the box without the strays, which clamp into the outermost cells of an fp64
    grid, and their own queries go to the whole-cloud search. (On 6 000 points the coarsened grid of
    level 1 is at most 18 cells wide at k = 20 and 64, so it is the last level and answers them.)"""
    X, stray = kc.few_strays(False, 60_000)
    want = kc.expected("few_strays", False, 60_000, k=k)
    idx, d2, levels, err = traced(X, k)
    assert "without its tails" in err and "searched over the whole cloud" in err
    assert all(lv["storage"] == F64 for lv in levels)
    assert [lv["kernel"] for lv in levels] == [kernel_of(k, lv["level"]) for lv in levels]
    assert_equal((idx, d2), want, k)
    assert_equal((idx[stray], d2[stray]), (want[0][stray], want[1][stray]), (k, "the strays' own"))


@pytest.mark.parametrize("k", [8, 20, 64])
@pytest.mark.parametrize("name", ["few_strays", "many_strays"])
def test_retry_levels_on_fp64_arrays(traced, monkeypatch, name, k):
    X, stray = kc.STRAYS[name](False)
    want = kc.expected(name, False, k=k)
    idx, d2, levels, err = traced(X, k)
    assert all(lv["storage"] == F64 for lv in levels)
    if name == "few_strays":    # the grids of the box without the strays, which clamp into its outermost cells
        assert "without its tails" in err
    assert_equal((idx, d2), want, (name, k))
    assert_equal((idx[stray], d2[stray]), (want[0][stray], want[1][stray]), (name, k, "the strays' own"))
    monkeypatch.setenv("PYQSM_KNN_ROBUST_BOX", "0")     # grids over the full box: retry levels
    idx, d2, levels, err = traced(X, k)
    assert "without its tails" not in err
    assert len(levels) >= 2 and "knn level 1:" in err
    assert all(lv["storage"] == F64 for lv in levels)
    assert [lv["kernel"] for lv in levels] == [kernel_of(k, lv["level"]) for lv in levels]
    assert all(lv["queries"] < len(X) for lv in levels[1:])
    assert_equal((idx, d2), want, (name, k, "full box"))
    assert_equal((idx[stray], d2[stray]), (want[0][stray], want[1][stray]), (name, k, "full box, the strays' own"))


# ---- e. retry levels with k > 64 (the LDS kernel over a query list), both storage forms ----------

@pytest.mark.parametrize("k", [80, 150])
@pytest.mark.parametrize("representable", [True, False])
@pytest.mark.parametrize("name", ["few_strays", "many_strays"])
def test_retry_levels_beyond_k64(traced, name, representable, k):
    X, stray = kc.STRAYS[name](representable)
    want = kc.expected(name, representable, k=k)
    idx, d2, levels, err = traced(X, k)
    assert "without its tails" not in err               # no robust box for k > 64
    assert len(levels) >= 2 and "knn level 1:" in err
    assert [lv["storage"] for lv in levels] == storage_by_level(levels, representable)
    assert levels[-1]["storage"] == (F32 if representable else F64)
    assert all(lv["kernel"] == kernel_of(k, lv["level"]) == kernel_of(k) for lv in levels)
    assert all(lv["queries"] < len(X) for lv in levels[1:])
    assert_equal((idx, d2), want, (name, representable, k))
    assert_equal((idx[stray], d2[stray]), (want[0][stray], want[1][stray]), (name, representable, k, "strays"))


# ---- f. both ways of making the retry grid -------------------------------------------------------

@pytest.mark.parametrize("representable", [True, False])
@pytest.mark.parametrize("name,k,made", [("many_strays", 20, "binned again"), ("few_strays", 80, "binned again"),
                                         ("axis_strays", 20, "coarsened"), ("axis_strays", 80, "coarsened")])
def test_both_ways_of_making_the_retry_grid(traced, monkeypatch, name, k, made, representable):
    """knn_device bins the points again when the fine grid has more than 2^22 cells and derives the
    coarse grid from the fine one (grid.hip: coarsen_grid) otherwise; each way feeds the wave kernel
    (k = 20) and the LDS kernel over a query list (k = 80). (At k = 80 the cells of many_strays' full
    box are wide enough for its first grid to stay below 2^22; few_strays' is above it.)"""
    monkeypatch.setenv("PYQSM_KNN_ROBUST_BOX", "0")
    X, stray = kc.STRAYS[name](representable)
    idx, d2, levels, err = traced(X, k)
    assert len(levels) >= 2
    assert (levels[0]["cells"] > 1 << 22) == (made == "binned again")
    assert levels[1]["made"] == made
    for prev, lv in zip(levels, levels[1:]):            # every level says how its grid was made
        assert lv["made"] == ("binned again" if prev["cells"] > 1 << 22 else "coarsened")
    assert [lv["storage"] for lv in levels] == storage_by_level(levels, representable)
    assert levels[1]["storage"] == (F32 if representable else F64)
    want = kc.expected(name, representable, k=k)
    assert_equal((idx, d2), want, (name, representable, k))
    assert_equal((idx[stray], d2[stray]), (want[0][stray], want[1][stray]), (name, representable, k, "strays"))


# ---- g. the contracted cloud ---------------------------------------------------------------------

@pytest.mark.parametrize("k", [20, 30])
def test_contracted_cloud(traced, k):
    P = kc.contracted()[0]
    idx, d2, levels, _ = traced(P, k, True)
    assert all(lv["storage"] == F64 for lv in levels)
    assert_equal((idx, d2), kc.expected("contracted", k=k), k)


def test_what_the_contraction_loop_hands_over(traced):
    got = sk.extract_skeleton(synth.forest(2500, seed=9), max_iter=8, contraction_factor=7, attraction_factor=3,
                              termination_ratio=0.0, device=0)[0]
    P = np.ascontiguousarray(got.points, dtype=np.float64)
    assert P.shape == (2500, 3) and np.isfinite(P).all()
    assert not kc.f32_representable(P).all()
    idx, d2, levels, _ = traced(P, 20, True)
    assert all(lv["storage"] == F64 for lv in levels)
    assert_equal((idx, d2), oracle.knn(P, 20, True), "contracted by the loop")


# ---- h. degenerates in fp64 ----------------------------------------------------------------------

def test_degenerates_on_fp64_arrays(traced):
    idx, d2, levels, _ = traced(kc.THREE, 5, True)      # fewer points than k: padded
    assert levels[0]["storage"] == F64
    assert list(idx[0]) == [1, 2, 3, 3, 3] and np.all(np.isinf(d2[:, 2:]))
    assert_equal((idx, d2), oracle.knn(kc.THREE, 5, True), "three points")
    idx, d2, levels, _ = traced(kc.IDENTICAL, 3, True)  # extent 0
    assert levels[0]["storage"] == F64
    assert np.all(d2 == 0) and list(idx[0]) == [1, 2, 3] and list(idx[39]) == [0, 1, 2]
    assert_equal((idx, d2), oracle.knn(kc.IDENTICAL, 3, True), "identical points")
    for excl in (True, False):
        idx, d2, levels, _ = traced(kc.ONE, 2, excl)
        assert levels[0]["storage"] == F64
        assert_equal((idx, d2), oracle.knn(kc.ONE, 2, excl), ("one point", excl))
    assert idx.tolist() == [[0, 1]] and d2[0, 0] == 0 and np.isinf(d2[0, 1])


# ---- i. the device-resident entry ----------------------------------------------------------------

@pytest.mark.parametrize("name,storage", [("forest", F32), ("offgrid", F64)])
def test_knn_dev_equals_knn(gpu, monkeypatch, capfd, name, storage):
    P = kc.cloud(name, 5000)
    n, k = len(P), 20
    d_xyz = hip.DeviceBuffer.from_array(P, device=gpu)
    d_idx = hip.DeviceBuffer(n * k * 4, device=gpu)
    d_d2 = hip.DeviceBuffer(n * k * 8, device=gpu)
    try:
        monkeypatch.setenv("PYQSM_KNN_TRACE", "1")
        capfd.readouterr()
        hip.knn_dev(d_xyz.ptr, n, k, True, d_idx.ptr, d_d2.ptr, device=gpu)
        err = capfd.readouterr().err
        idx, d2 = d_idx.download((n, k), np.int32), d_d2.download((n, k), np.float64)
        again = d_xyz.download((n, 3), np.float64)
    finally:
        for b in (d_xyz, d_idx, d_d2):
            b.free()
    m = LEVEL.search(err)
    assert m and m[7] == storage and m[8] == kernel_of(k), err
    assert np.array_equal(again, P)                     # the caller's points are left as they were
    assert_equal((idx, d2), hip.knn(P, k, True, device=gpu), name)
    assert_equal((idx, d2), kc.expected(name, 5000, k=k), name)


# ---- j. the compiled-in alternates of k_knn_reg --------------------------------------------------

@pytest.mark.parametrize("knob,variant", [("PYQSM_KNN_BUF", "0,false"), ("PYQSM_KNN_STRICT", "4,false")])
def test_alternate_instantiations_in_a_child_process(gpu, knob, variant):
    """PYQSM_KNN_BUF=0 (k_knn_reg<K, 0, false>) and PYQSM_KNN_STRICT=0 (k_knn_reg<K, 4, false>) are read
    once per process: a fresh child each, one after the other. Neither has a tie pass, so the trace
    counts no query searched again on the cloud where the default counts most of them."""
    env = dict(os.environ, PYQSM_KNN_TRACE="1")
    env.pop("PYQSM_KNN_BUF", None)
    env.pop("PYQSM_KNN_STRICT", None)
    env[knob] = "0"
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from tests import knn_cases as kc; "
            "sys.exit(kc.check_alternates())")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=120)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("equal to the oracle") == len(kc.ALTERNATE_CLOUDS)
    first = [(m[7], m[8]) for m in LEVEL.finditer(r.stderr) if m[1] == "0"]     # (many_ties runs level 0 twice)
    assert len(first) >= len(kc.ALTERNATE_CLOUDS) and set(first) == {(F64, kernel_of(20, 0, variant))}
    ties = [int(c) for c in TIES.findall(r.stderr)]
    assert len(ties) >= len(kc.ALTERNATE_CLOUDS) and not any(ties)


# ---- 3. what is computed from (idx, d2) does not depend on the storage form ----------------------

def test_consumers_do_not_depend_on_the_storage_form(gpu, monkeypatch):
    P = kc.forest(3000)
    values = np.random.default_rng(3).normal(size=(len(P), 2))

    def consumers():
        keep, avg, stats = hip.stat_outlier(P, 20, 2.0, return_stats=True, device=gpu)
        smooth, nbr = hip.smooth_values(P, values, 12, "mean", return_indices=True, device=gpu)
        edges, ed2 = hip.skeletal_forest(P, 8, device=gpu)
        (indptr, indices, data), mass = hip.pc_laplacian(P, 20, device=gpu)
        normals = hip.estimate_normals(P, None, 30, device=gpu)          # KNN search
        return dict(keep=keep, avg=avg, stats=np.array(stats), smooth=smooth, nbr=nbr, edges=edges, ed2=ed2,
                    indptr=indptr, indices=indices, data=data, mass=mass, normals=normals)

    monkeypatch.delenv("PYQSM_COORD_F32", raising=False)
    records = consumers()
    monkeypatch.setenv("PYQSM_COORD_F32", "0")
    arrays = consumers()
    for name in records:
        assert records[name].shape == arrays[name].shape and records[name].size, name
        assert np.array_equal(records[name], arrays[name]), name
