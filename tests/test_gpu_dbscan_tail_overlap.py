"""The latency-bound tail passes of the DBSCAN step ride other launches (dbscan.hip): the stragglers of the
core pass walk their stencil centre row first (stencil_runs in kRunOrder), the list of non-core points is
built by extra blocks of the k_rep_root launch (flags_role; a launch of its own on the doubled-cell path), and
the border points are labelled inside the k_labels launch, by the waves that have stored their core points'
labels. Every case compares labels, core flags and the cluster count of the device entry point with the
oracle, twice on the same context: a counter the first call left behind would show in the second. The second
call runs under PYQSM_DBSCAN_TRACE, whose lines give the lengths of the two lists."""
import functools
import re

import numpy as np
import pytest

import oracle
from pyqsm_amd import hip

pytestmark = pytest.mark.gpu

EPS = 0.1


def _f32(P):
    return np.ascontiguousarray(P, dtype=np.float64).astype(np.float32).astype(np.float64)


def _call(P, eps, min_pts, gpu, with_core=True):
    n = P.shape[0]
    d_xyz = hip.DeviceBuffer.from_array(np.ascontiguousarray(P, dtype=np.float64), device=gpu)
    d_lab = hip.DeviceBuffer(n * 8, device=gpu)
    d_core = hip.DeviceBuffer(n, device=gpu) if with_core else None
    cnt = hip.dbscan_dev(d_xyz.ptr, n, eps, min_pts, d_lab.ptr, d_core.ptr if with_core else None, gpu,
                         want_count=True)
    core = d_core.download((n,), np.uint8).astype(bool) if with_core else None
    return d_lab.download((n,), np.int64), core, cnt


def _twice(P, eps, min_pts, gpu, monkeypatch, capfd, ref, with_core=True):
    """Two calls against the oracle's (labels, core flags), the second one traced. Returns (stragglers of
    the core pass, listed non-core points) of the step that produced the second call's results."""
    lab0, core0 = ref
    want = int(lab0.max()) + 1 if lab0.size else 0
    trace = None
    for traced in (False, True):
        if traced:
            monkeypatch.setenv("PYQSM_DBSCAN_TRACE", "1")
            capfd.readouterr()
        lab, core, cnt = _call(P, eps, min_pts, gpu, with_core)
        if traced:
            trace = capfd.readouterr().err
            monkeypatch.delenv("PYQSM_DBSCAN_TRACE")
        if with_core:
            assert np.array_equal(core, core0)
        assert np.array_equal(lab, lab0)
        assert cnt == want
    stragglers = [int(x) for x in re.findall(r"core pass: (\d+) stragglers", trace)]
    listed = [int(x) for x in re.findall(r"label pass: (\d+) non-core points listed", trace)]
    assert stragglers and listed, trace
    print(f"n {P.shape[0]}: {stragglers[-1]} stragglers, {listed[-1]} non-core points listed, {cnt} clusters")
    return stragglers[-1], listed[-1]


# ---- 1. border points between two clusters --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _bridged_pairs(seed):
    """300 pairs of 12-point groups 0.19 apart with one point between them that has core neighbours in both
    (and fewer than min_pts = 12 neighbours itself), on a lattice of spacing 0.5; 500 noise points in a slab
    one unit above. Returns the cloud and the oracle's result for eps 0.1, min_pts 12."""
    rng = np.random.default_rng(seed)
    sites = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    sites = sites * 0.5 + rng.uniform(0.0, 0.2, 3)
    xs = np.linspace(-0.02, 0.0, 12)
    a = np.stack([xs, np.zeros(12), np.zeros(12)], 1)
    b = np.stack([0.19 - xs, np.zeros(12), np.zeros(12)], 1)
    parts = []
    for s in sites:
        parts.append(s + a + rng.uniform(-0.002, 0.002, (12, 3)))
        parts.append(s + b + rng.uniform(-0.002, 0.002, (12, 3)))
        parts.append(s + np.array([[0.095, 0.0, 0.0]]))
    top = sites[:, 2].max() + 1.0
    noise = np.stack([rng.uniform(0, 5, 500), rng.uniform(0, 5, 500), rng.uniform(top, top + 0.5, 500)], 1)
    P = np.concatenate(parts + [noise])
    P = _f32(P[rng.permutation(len(P))])
    lab0, core0 = oracle.dbscan(P, EPS, 12)
    # the recipe's counts, from the oracle, before the GPU is trusted with it
    assert len(P) == 8000 and lab0.max() + 1 == 600 and (lab0 < 0).sum() == 500
    border = np.flatnonzero(~core0 & (lab0 >= 0))
    assert len(border) == 300
    for i in border:  # core neighbours in exactly two clusters, labelled with the smaller number
        near = core0 & (((P - P[i]) ** 2).sum(1) <= EPS * EPS)
        both = np.unique(lab0[near])
        assert len(both) == 2 and lab0[i] == both.min()
    return P, (lab0, core0)


@pytest.mark.parametrize("seed", [61, 62])
def test_border_points_between_two_clusters(gpu, monkeypatch, capfd, seed):
    P, ref = _bridged_pairs(seed)
    _, listed = _twice(P, EPS, 12, gpu, monkeypatch, capfd, ref)
    assert listed == 800  # 300 border points and 500 noise points


# ---- 2. neighbours confined to one row of the stencil, at the threshold ------------------------------------

MIN_PTS_ROWS = 10
COPIES = 6


@functools.lru_cache(maxsize=None)
def _row_cloud(row, m):
    """COPIES planted points at cell centres (the grid's origin is the cloud's minimum corner, pinned by a point
    at 0; cells of edge eps), each with m neighbours within +-0.005 of the spot 0.085 away in row (dy, dz) of
    its stencil — for the centre row in the two x-neighbour cells —, in a sparse uniform background (about one
    neighbour within eps) that is cleared around them. Nobody of the background gets near min_pts."""
    dy, dz = row % 3 - 1, row // 3 - 1
    rng = np.random.default_rng(1000 + 10 * row + m)
    n_bg = 3000
    side = (n_bg * 4.19e-3) ** (1.0 / 3.0)  # one expected neighbour in a ball of radius eps
    bg = rng.uniform(0.0, side, (n_bg, 3))
    sites = np.stack(np.meshgrid(*[np.array([4, 10, 16])] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = (sites[rng.permutation(len(sites))[:COPIES]] + 0.5) * EPS  # at least six cells apart
    parts = [np.zeros((1, 3))]
    for ctr in centres:
        bg = bg[((bg - ctr) ** 2).sum(1) > 0.3 ** 2]
        if dy == 0 and dz == 0:  # both x-neighbour cells, 0.17 apart: only the planted point sees them all
            offs = np.array([[0.085, 0.0, 0.0]]) * np.where(np.arange(m) % 2 == 0, 1.0, -1.0)[:, None]
        else:
            offs = np.tile(np.array([0.0, dy, dz]) * (0.085 / np.hypot(dy, dz)), (m, 1))
        parts.append(ctr[None, :])
        parts.append(ctr + offs + rng.uniform(-0.005, 0.005, (m, 3)))
    P = np.concatenate(parts + [bg])
    P = _f32(P[rng.permutation(len(P))])
    return P, oracle.dbscan(P, EPS, MIN_PTS_ROWS)


@pytest.mark.parametrize("m", [MIN_PTS_ROWS - 2, MIN_PTS_ROWS - 1])
@pytest.mark.parametrize("row", range(9))
def test_row_confined_neighbours_at_the_threshold(gpu, monkeypatch, capfd, row, m):
    """The planted point counts itself and m neighbours: min_pts - 1 (not core) or exactly min_pts (core),
    whichever row of the stencil holds them, that is wherever in the centre-first sequence they come.

    The straggler count is n wherever the tiled pass decides nobody. A wave of k_core_tiled stages the centre
    interval of its tile first (its own points' cells and what lies between them in the grid's linear order, with
    the x-neighbour cells), then the intervals one y-row down and up, and hands everybody still short on after
    kMaxChunks = 3 chunks of 64. The three intervals of its own z-layer hold candidates each, in this background,
    so it never stages a candidate of the layers below and above.
    - m = min_pts - 2: nobody reaches min_pts anywhere: n stragglers, every row.
    - m = min_pts - 1, neighbours in a layer below or above (dz != 0): a planted point and its neighbours each
      count min_pts - 1 inside their own layer and need the other layer for the last one: n stragglers, and
      k_core_rest decides the threshold case through stencil_runs.
    - m = min_pts - 1, centre row: the neighbours lie in the x-neighbour cells, inside the centre interval, which
      holds the wave's 64 points and a few more, two chunks: the tiled pass itself finds the planted points core.
      Their neighbours (five and four a side) stay short: n less the COPIES planted points.
    - m = min_pts - 1, rows dy = -1, +1 of the own layer: the 64 points of a wave lie some 270 cells apart in
      this background, some ten y-rows, so the centre interval usually holds the neighbouring y-rows too and the
      tiled pass decides the planted groups; a group cut by the end of a wave's interval is handed on. Only
      bounded: n less at most the core points."""
    P, ref = _row_cloud(row, m)
    lab0, core0 = ref
    n = len(P)
    if m == MIN_PTS_ROWS - 2:
        assert not core0.any() and (lab0 == -1).all()
    else:
        centre = row == 4
        # centre row: the neighbours sit in two groups 0.17 apart, so only the planted points are core
        assert core0.sum() == (COPIES if centre else COPIES * (m + 1)) and lab0.max() + 1 == COPIES
    stragglers, listed = _twice(P, EPS, MIN_PTS_ROWS, gpu, monkeypatch, capfd, ref)
    assert listed == n - core0.sum()
    if m == MIN_PTS_ROWS - 2 or row // 3 != 1:
        assert stragglers == n
    elif row == 4:
        assert stragglers == n - COPIES
    else:
        assert n - core0.sum() <= stragglers <= n


# ---- 3. edges of the two roles ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _clump_and_strays(n):
    """Most points in one clump of diameter < eps, every eighth (at most 40) a stray on a line, 3 eps apart."""
    rng = np.random.default_rng(n)
    strays = min(n // 8, 40)
    clump = rng.uniform(0.0, 0.05, (n - strays, 3))
    line = np.zeros((strays, 3))
    line[:, 0] = 1.0 + 3.0 * EPS * np.arange(strays)
    P = np.concatenate([clump, line])
    P = _f32(P[rng.permutation(n)])
    return P, oracle.dbscan(P, EPS, 5)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_sizes_around_the_roles_blocks(gpu, monkeypatch, capfd, n):
    P, ref = _clump_and_strays(n)
    _, listed = _twice(P, EPS, 5, gpu, monkeypatch, capfd, ref)
    assert listed == (~ref[1]).sum()


@pytest.mark.parametrize("kind", ["all core", "one non-core", "no core"])
def test_list_lengths_0_and_1_and_no_root(gpu, monkeypatch, capfd, kind):
    rng = np.random.default_rng(71)
    P = rng.uniform(0.0, 0.05, (700, 3))  # one clump: every point a core point
    if kind == "one non-core":
        P = np.concatenate([P, [[2.0, 2.0, 2.0]]])
    if kind == "no core":
        P = np.stack([np.arange(700) * 3.0 * EPS, np.zeros(700), np.zeros(700)], 1)
    P = _f32(P[rng.permutation(len(P))])
    ref = oracle.dbscan(P, EPS, 5)
    want = {"all core": 0, "one non-core": 1, "no core": 700}[kind]
    assert (~ref[1]).sum() == want and ref[0].max() + 1 == (0 if kind == "no core" else 1)
    _, listed = _twice(P, EPS, 5, gpu, monkeypatch, capfd, ref)
    assert listed == want


def test_without_core_flags(gpu, monkeypatch, capfd):
    P, ref = _bridged_pairs(61)
    _, listed = _twice(P, EPS, 12, gpu, monkeypatch, capfd, ref, with_core=False)
    assert listed == 800


# ---- 4. paths -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [("PYQSM_DBSCAN_PLAN", "host"), ("PYQSM_COORD_F32", "0")])
def test_host_plan_and_fp64_records(gpu, monkeypatch, capfd, env):
    monkeypatch.setenv(*env)
    P, ref = _bridged_pairs(62)
    _, listed = _twice(P, EPS, 12, gpu, monkeypatch, capfd, ref)
    assert listed == 800


def test_doubled_cells_with_noise(gpu, monkeypatch, capfd):
    """Groups along the space diagonal: the grid doubles its cells, the per-point union-find runs, the flags
    list is built by a launch of its own. min_pts = 4 leaves the smaller groups as noise."""
    monkeypatch.setenv("PYQSM_DBSCAN_PLAN", "host")  # (a speculative step would count its k_hook_sub launch)
    rng = np.random.default_rng(81)
    groups = 5000
    centres = np.cumsum(rng.uniform(0.6, 2.0, groups) * EPS)[:, None] * [1.0, 1.0, 1.0]
    sizes = rng.integers(1, 6, groups)
    P = np.concatenate([c + rng.uniform(0, 0.3 * EPS, (s, 3)) for c, s in zip(centres, sizes)])
    P = P[rng.permutation(len(P))]
    ref = oracle.dbscan(P, EPS, 4)
    assert (ref[0] < 0).any() and ref[1].any()
    hip.prof_enable(True, gpu)
    hip.prof_reset(gpu)
    try:
        _, listed = _twice(P, EPS, 4, gpu, monkeypatch, capfd, ref)
        hooks = hip.prof_get("k_hook_sub", gpu)[1]
    finally:
        hip.prof_enable(False, gpu)
    assert hooks == 0  # not the sub-cell path
    assert listed == (~ref[1]).sum()


def test_bitmap_numbering_with_noise(gpu, monkeypatch, capfd):
    """4400 clusters of two points (min_pts = 2) and 200 noise points: more roots than one workgroup ranks,
    the border role reads the bitmap numbering as the label role does."""
    k = 4400
    rng = np.random.default_rng(91)
    side = int(np.ceil(k ** (1 / 3))) + 1
    cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = cells[rng.permutation(len(cells))[:k]] * 0.5
    a = centres + rng.uniform(0, 0.03, (k, 3))
    b = a + rng.uniform(-0.04, 0.04, (k, 3))
    noise = cells[rng.permutation(len(cells))[:200]] * 0.5 + 0.25
    P = _f32(np.concatenate([a, b, noise]))
    P = P[rng.permutation(len(P))]
    ref = oracle.dbscan(P, EPS, 2)
    assert ref[0].max() + 1 == k and (ref[0] < 0).sum() == 200
    _, listed = _twice(P, EPS, 2, gpu, monkeypatch, capfd, ref)
    assert listed == 200


def test_profiling_on_equals_off(gpu):
    """The stamped launches carry two roles each: the results are those of an unprofiled step, and the label
    and union phases are counted once per step."""
    P, (lab0, core0) = _bridged_pairs(61)
    for _ in range(2):  # (a hint for this shape: the profiled calls are hits)
        lab, core, _ = _call(P, EPS, 12, gpu)
        assert np.array_equal(lab, lab0) and np.array_equal(core, core0)
    steps = 3
    hip.prof_enable(True, gpu)
    hip.prof_reset(gpu)
    try:
        for _ in range(steps):
            lab, core, cnt = _call(P, EPS, 12, gpu)
            assert np.array_equal(lab, lab0) and np.array_equal(core, core0) and cnt == 600
        timers = {k: hip.prof_get(k, gpu) for k in ("dbscan_label", "dbscan_union", "dbscan_plan_hit")}
    finally:
        hip.prof_enable(False, gpu)
    assert timers["dbscan_plan_hit"][1] == steps
    for k in ("dbscan_label", "dbscan_union"):
        assert timers[k][1] == steps and timers[k][0] > 0, k
