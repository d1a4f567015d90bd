"""DBSCAN's union phase with second links (dbscan.hip): k_hook_sub hooks every sub-cell under its first
connected neighbour among the 13 near negative offsets and records the next connected one as the
sub-cell's second link; the compression that reaches the roots unites across those links; a third, short
compression writes the cells' summary words; k_union_sub remains what makes the phase complete.
The clouds are built so that each part has to carry the result: trees that only second links join,
sub-cells without a second link, candidates that have to be passed over, trees that must stay apart,
thousands of unions racing with the compression's stores, and the list's edges. Every case is compared
with the CPU oracle for labels, core flags and the cluster count, on a host-planned call and on the call
after it. The figures asserted from PYQSM_DBSCAN_TRACE follow from the shapes (see each fixture)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle
from pyqsm_amd import hip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 0.1
U = 0.5 * EPS * (1.0 + 1.0 / 1048576.0)      # a sub-cell's edge: half a cell of the device's grid


def _f32(P):
    return np.ascontiguousarray(P, dtype=np.float64).astype(np.float32).astype(np.float64)


def _call(P, eps, min_pts, gpu, host=False, radius_inclusive=True, prof=True):
    """(labels, core, cluster count, 'hit' | 'miss' | None) of one call of the device entry point."""
    n = P.shape[0]
    d_xyz = hip.DeviceBuffer.from_array(np.ascontiguousarray(P, dtype=np.float64), gpu)
    d_lab = hip.DeviceBuffer(n * 8, gpu)
    d_core = hip.DeviceBuffer(n, gpu)
    old = os.environ.pop("PYQSM_DBSCAN_PLAN", None)
    if host:
        os.environ["PYQSM_DBSCAN_PLAN"] = "host"
    path = None
    try:
        if prof:
            hip.prof_enable(True, gpu)
            hip.prof_reset(gpu)
        cnt = hip.dbscan_dev(d_xyz.ptr, n, eps, min_pts, d_lab.ptr, d_core.ptr, gpu, want_count=True,
                             radius_inclusive=radius_inclusive)
        if prof:
            hit = hip.prof_get("dbscan_plan_hit", gpu)[1]
            miss = hip.prof_get("dbscan_plan_miss", gpu)[1]
            hip.prof_enable(False, gpu)
            assert hit + miss == 1
            path = "hit" if hit else "miss"
    finally:
        os.environ.pop("PYQSM_DBSCAN_PLAN", None)
        if old is not None:
            os.environ["PYQSM_DBSCAN_PLAN"] = old
    return d_lab.download((n,), np.int64), d_core.download((n,), np.uint8).astype(bool), cnt, path


def _check(P, eps, min_pts, gpu, runs=2, radius_inclusive=True, paths=("miss", "hit"), prof=True):
    """A host-planned call (a miss that leaves this cloud's hint), then runs - 1 more; each against the
    oracle. `paths`: what the calls must report (None: the cloud decides)."""
    lab0, core0 = oracle.dbscan(P, eps, min_pts, radius_inclusive=radius_inclusive)
    got = []
    for i in range(runs):
        lab, core, cnt, path = _call(P, eps, min_pts, gpu, host=i == 0, radius_inclusive=radius_inclusive, prof=prof)
        assert np.array_equal(core, core0)
        assert np.array_equal(lab, lab0)
        assert cnt == lab0.max() + 1
        got.append(path)
    if paths is not None and prof:
        assert got == [paths[0]] + [paths[1]] * (runs - 1)
    return lab0, core0


def _trace(P, eps, min_pts, gpu, capfd, radius_inclusive=True):
    """One more call with PYQSM_DBSCAN_TRACE: (labels, {'listed', 'hook_roots', 'links', 'crossing',
    'roots_left', 'seams'}); the link pass's figures are absent where the second links are switched off."""
    os.environ["PYQSM_DBSCAN_TRACE"] = "1"
    try:
        capfd.readouterr()
        lab, _, _, _ = _call(P, eps, min_pts, gpu, radius_inclusive=radius_inclusive)
        err = capfd.readouterr().err
    finally:
        del os.environ["PYQSM_DBSCAN_TRACE"]
    out = {}
    m = re.findall(r"hook pass: (\d+) sub-cells, (\d+) roots", err)
    if m:
        out["listed"], out["hook_roots"] = int(m[-1][0]), int(m[-1][1])
    m = re.findall(r"link pass: (\d+) recorded, (\d+) crossed trees, (\d+) roots left", err)
    if m:
        out["links"], out["crossing"], out["roots_left"] = (int(x) for x in m[-1])
    m = re.findall(r"seam union: (\d+) sub-cells", err)
    if m:
        out["seams"] = int(m[-1])
    return lab, out


def _link2_on():
    return os.environ.get("PYQSM_DBSCAN_LINK2", "1") != "0"


def _clumps(centres, k=4, seed=0):
    """k near-coincident points (within 1e-3 eps) around every centre, shuffled."""
    rng = np.random.default_rng(seed)
    centres = np.asarray(centres, dtype=np.float64)
    P = centres[:, None, :] + rng.uniform(-1e-3, 1e-3, (centres.shape[0], k, 3)) * EPS
    P = P.reshape(-1, 3)
    return _f32(P[rng.permutation(P.shape[0])])


# ---- two basins that second links join ---------------------------------------------------------

def _arch(up, levels=40, gap=8):
    """An upside-down U: two arms of clumps 0.45 eps apart along axis `up`, `gap` steps apart along the next
    axis, joined by a bar of clumps at the top. Pointers of the hook pass lead to lexicographically smaller
    sub-cells, so each arm drains to its own bottom: two basins. Where the bar meets the far arm a sub-cell
    has a connected neighbour in either basin, one as its first link and the other as its second."""
    side = (up + 1) % 3
    step = 0.45 * EPS
    c = []
    for i in range(levels):
        for b in (0, gap):
            p = np.zeros(3)
            p[up], p[side] = i * step, b * step
            c.append(p)
    for b in range(1, gap):
        p = np.zeros(3)
        p[up], p[side] = (levels - 1) * step, b * step
        c.append(p)
    return _clumps(c, seed=up)


@pytest.mark.parametrize("up", [0, 1, 2])
def test_two_basins_joined_by_second_links(gpu, capfd, up):
    P = _arch(up)
    lab0, core0 = _check(P, EPS, 4, gpu)
    assert core0.all() and lab0.max() == 0          # the fixture: one arch, one cluster
    lab, tr = _trace(P, EPS, 4, gpu, capfd)
    assert np.array_equal(lab, lab0)
    assert tr["hook_roots"] >= 2                    # the arms' bottoms
    if _link2_on():
        assert tr["crossing"] >= 1
        assert tr["roots_left"] < tr["hook_roots"]


# ---- no second link ----------------------------------------------------------------------------

def _row(direction, clumps, pitch, k=4, seed=0):
    d = np.asarray(direction, dtype=np.float64)
    d /= np.linalg.norm(d)
    return _clumps(np.arange(clumps)[:, None] * (pitch * EPS) * d[None, :], k=k, seed=seed)


def test_single_row_has_one_near_neighbour_each(gpu, capfd):
    # clumps 0.45 eps apart along x: a sub-cell's only near negative neighbour is the one before it
    P = _row((1, 0, 0), 300, 0.45)
    lab0, core0 = _check(P, EPS, 4, gpu)
    assert core0.all() and lab0.max() == 0
    lab, tr = _trace(P, EPS, 4, gpu, capfd)
    assert np.array_equal(lab, lab0) and tr["hook_roots"] == 1
    if _link2_on():
        assert tr["links"] == 0 and tr["crossing"] == 0 and tr["roots_left"] == 1


def test_isolated_clumps_have_no_link(gpu, capfd):
    P = _row((1, 0, 0), 200, 3.3)
    lab0, core0 = _check(P, EPS, 4, gpu)
    assert core0.all() and lab0.max() + 1 == 200
    lab, tr = _trace(P, EPS, 4, gpu, capfd)
    # (a clump that straddles a sub-cell boundary is listed as two sub-cells, one hooked under the other)
    assert np.array_equal(lab, lab0) and tr["listed"] >= 200 and tr["hook_roots"] == 200
    if _link2_on():
        assert tr["links"] == 0 and tr["roots_left"] == 200


@pytest.mark.parametrize("direction", [(1, 0, 0), (0, 0, 1), (1, 1, 1), (1, -1, 0)])
def test_far_rows_are_left_to_the_seam_pass(gpu, capfd, direction):
    # clumps 0.9 eps apart: a sub-cell has one connected neighbour below it at most (the one after the next
    # is 1.8 eps away), most of them two sub-cells away, so there is never a second link and the hook pass
    # leaves many trees for k_union_sub
    P = _row(direction, 300, 0.9, seed=1)
    lab0, core0 = _check(P, EPS, 4, gpu)
    assert core0.all() and lab0.max() == 0
    lab, tr = _trace(P, EPS, 4, gpu, capfd)
    assert np.array_equal(lab, lab0) and tr["hook_roots"] > 1 and tr["seams"] > 0
    if _link2_on():
        assert tr["links"] == 0 and tr["roots_left"] == tr["hook_roots"]


# ---- candidates that have to be passed over ----------------------------------------------------

def _passed_over(same_tree):
    """Clumps in sub-cell units around S = sub-cell (4, 4, 4); the single point at the origin pins the grid.
    S's candidates in the hook pass's order: A at offset (1, 0, 0), connected, the hook; B at (-1, 1, 0),
    occupied but in the opposite corner, more than eps (= 2 sub-cells) from S; C at (0, 1, 0), connected:
    the second link, found only by passing over B. With `same_tree` A and C are connected to each other (A
    hangs under C, the second link is a no-op); without, they are 2.5 sub-cells apart, two trees that S's
    second link joins."""
    if same_tree:
        S, A, C, B = (4.1, 4.9, 4.1), (3.9, 4.9, 4.1), (4.1, 3.9, 4.1), (5.95, 3.05, 4.95)
    else:
        S, A, C, B = (4.5, 4.5, 4.5), (3.1, 4.9, 4.5), (4.9, 3.1, 4.5), (5.95, 3.05, 4.9)
    P = _clumps(np.array([S, A, C, B]) * U, seed=3)
    return np.concatenate([np.zeros((1, 3)), P])


@pytest.mark.parametrize("same_tree", [False, True])
def test_unconnected_candidate_is_passed_over(gpu, capfd, same_tree):
    P = _passed_over(same_tree)
    lab0, core0 = _check(P, EPS, 4, gpu)
    # the fixture: S, A, C (and B through C) are one cluster when A and C are apart; B is 2.2 sub-cells
    # from C in the other layout and stays alone
    assert lab0.max() + 1 == (2 if same_tree else 1) and core0[1:].all() and not core0[0]
    lab, tr = _trace(P, EPS, 4, gpu, capfd)
    assert np.array_equal(lab, lab0) and tr["listed"] == 4
    if _link2_on():
        assert tr["links"] == 1                     # S's, across B
        assert tr["crossing"] == (0 if same_tree else 1)
        assert tr["roots_left"] == (2 if same_tree else 1)


# ---- trees that must stay apart ----------------------------------------------------------------

def test_two_sheets_in_shared_cells_stay_apart(gpu, capfd):
    # two sheets normal to (1, 1, 0), 1.05 eps apart: a cell is 1.41 eps wide that way, so most cells hold
    # sub-cells of both (mixed words), and no pair of points of different sheets is within eps
    a = np.arange(30) * (0.3 * EPS)
    s, z = np.meshgrid(a, a, indexing="ij")
    along, normal = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0), np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    sheet = s.reshape(-1, 1) * along + z.reshape(-1, 1) * np.array([0.0, 0.0, 1.0])
    P = np.concatenate([sheet, sheet + 1.05 * EPS * normal])
    which = np.repeat([0, 1], sheet.shape[0])
    perm = np.random.default_rng(5).permutation(P.shape[0])
    P, which = _f32(P[perm]), which[perm]
    lab0, core0 = _check(P, EPS, 3, gpu)
    assert core0.all() and lab0.max() + 1 == 2
    assert np.unique(lab0[which == 0]).size == 1 and np.unique(lab0[which == 1]).size == 1
    lab, tr = _trace(P, EPS, 3, gpu, capfd)
    assert np.array_equal(lab, lab0) and tr["seams"] > 0
    if _link2_on():
        assert tr["roots_left"] >= 2


# ---- many trees --------------------------------------------------------------------------------

def _sticks(nx=50, ny=40):
    """nx * ny pairs of sticks, five points each 0.45 eps apart in height, leaning towards each other: 0.45
    eps apart at the top, 1.45 eps one level down (and 1.05 eps from a top to the other stick's next level).
    Every stick drains to its own bottom, and the two of a pair touch at their tops only."""
    pts = []
    for i in range(5):
        half = (0.225 + 0.5 * (4 - i)) * EPS
        for sgn in (-1.0, 1.0):
            pts.append((sgn * half, 0.0, i * 0.45 * EPS))
    pair = np.array(pts)
    gx, gy = np.meshgrid(np.arange(nx) * 6.3 * EPS, np.arange(ny) * 2.6 * EPS, indexing="ij")
    off = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], -1)
    P = (off[:, None, :] + pair[None, :, :]).reshape(-1, 3)
    return _f32(P[np.random.default_rng(7).permutation(P.shape[0])])


def test_thousands_of_trees_touching_in_pairs(gpu, capfd):
    P = _sticks()
    lab0, core0 = _check(P, EPS, 2, gpu, runs=3)
    assert core0.all() and lab0.max() + 1 == 2000
    lab, tr = _trace(P, EPS, 2, gpu, capfd)
    assert np.array_equal(lab, lab0) and tr["hook_roots"] >= 4000


# ---- the list's edges --------------------------------------------------------------------------

def _block(m):
    """m listed sub-cells, a point in the middle of each, two rows along x (half a cell between neighbours:
    all one cluster, most sub-cells with two or more connected near neighbours); the first point is at the
    origin and pins the grid."""
    ij = [(i, j) for i in range(m) for j in (0, 1)][1:m]
    P = np.array([(0.0, 0.0, 0.0)] + [((i + 0.5) * U, (j + 0.5) * U, 0.5 * U) for i, j in ij])
    return _f32(P)


@pytest.mark.parametrize("m", [8, 9, 10, 11, 255, 256, 257])
def test_list_lengths(gpu, capfd, m):
    P = _block(m)
    lab0, core0 = _check(P, EPS, 2, gpu)
    assert core0.all() and lab0.max() == 0
    lab, tr = _trace(P, EPS, 2, gpu, capfd)
    assert np.array_equal(lab, lab0) and tr["listed"] == m
    if _link2_on():
        assert tr["links"] >= m // 2 - 1 and tr["roots_left"] >= 1


def test_one_sub_cell(gpu, capfd):
    P = _f32(np.array([[0.0, 0.0, 0.0], [1e-3, 0.0, 0.0], [0.0, 1e-3, 0.0]]))
    lab0, core0 = _check(P, EPS, 3, gpu)
    assert core0.all() and lab0.max() == 0
    _, tr = _trace(P, EPS, 3, gpu, capfd)
    assert tr["listed"] == 1
    if _link2_on():
        assert (tr["links"], tr["crossing"], tr["roots_left"]) == (0, 0, 1)


def test_no_core_point(gpu, capfd):
    P = _f32(np.random.default_rng(9).uniform(0, 1, (50, 3)))
    lab0, core0 = _check(P, EPS, 10, gpu)
    assert not core0.any() and lab0.max() == -1
    _, tr = _trace(P, EPS, 10, gpu, capfd)
    assert tr["listed"] == 0
    if _link2_on():
        assert (tr["links"], tr["crossing"], tr["roots_left"]) == (0, 0, 0)


# ---- variants ----------------------------------------------------------------------------------

def _not_f32(P):
    Q = P.copy()
    Q[0, 0] += 1e-9
    assert not np.array_equal(_f32(Q), Q)
    return Q


def _clump_cloud(seed, n=6000):
    """Clumps of 5-40 points on random walks with steps of U(0.3, 1.2) eps: near and far neighbours, dense
    and sparse places, a few walks."""
    rng = np.random.default_rng(seed)
    P, centre, total = [], np.zeros(3), 0
    while total < n:
        if rng.random() < 0.04:
            centre = rng.uniform(-1, 1, 3) * 10 * EPS
        else:
            d = rng.normal(size=3)
            centre = centre + d / np.linalg.norm(d) * rng.uniform(0.3, 1.2) * EPS
        k = int(rng.integers(5, 41))
        P.append(centre + rng.normal(size=(k, 3)) * 0.1 * EPS)
        total += k
    P = np.concatenate(P)[:n]
    return _f32(P[rng.permutation(n)])


def test_fp64_records(gpu):
    _check(_not_f32(_arch(2)), EPS, 4, gpu, paths=("miss", "miss"))
    _check(_not_f32(_sticks(10, 10)), EPS, 2, gpu, paths=("miss", "miss"))


def test_strict_radius(gpu):
    _check(_arch(0), EPS, 4, gpu, radius_inclusive=False)
    _check(_clump_cloud(11), EPS, 5, gpu, radius_inclusive=False)


@pytest.mark.parametrize("min_pts", [1, 10])
def test_min_pts(gpu, min_pts):
    _check(_clump_cloud(20 + min_pts), EPS, min_pts, gpu)


def test_profiling_on_and_off(gpu):
    P = _clump_cloud(31)
    _check(P, EPS, 5, gpu, prof=True)
    _check(P, EPS, 5, gpu, prof=False)


_SWITCH_SCRIPT = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from pyqsm_amd import hip, _lib
_lib.require_gpu(0)
clouds = np.load(sys.argv[2])
out = {}
for name in clouds.files:
    P = clouds[name]
    for rep in range(2):
        lab, core = hip.dbscan(P, 0.1, int(name.split("_")[-1]))
        out[f"{name}_lab{rep}"], out[f"{name}_core{rep}"] = lab, core
np.savez(sys.argv[3], **out)
"""


def test_switch_gives_identical_labels(gpu, tmp_path):
    # PYQSM_DBSCAN_LINK2 is read once per process: a fresh process for each value
    clouds = {"arch_4": _arch(1), "sticks_2": _sticks(20, 20), "walks_5": _clump_cloud(41), "walks_1": _clump_cloud(42)}
    np.savez(tmp_path / "clouds.npz", **clouds)
    (tmp_path / "run.py").write_text(_SWITCH_SCRIPT)
    res = {}
    for value in ("0", "1"):
        env = dict(os.environ, PYQSM_DBSCAN_LINK2=value)
        env.pop("PYQSM_DBSCAN_TRACE", None)
        r = subprocess.run([sys.executable, str(tmp_path / "run.py"), ROOT, str(tmp_path / "clouds.npz"),
                            str(tmp_path / f"out{value}.npz")], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr
        res[value] = np.load(tmp_path / f"out{value}.npz")
    assert sorted(res["0"].files) == sorted(res["1"].files) and len(res["0"].files) == 16
    for key in res["0"].files:
        assert np.array_equal(res["0"][key], res["1"][key]), key
    for name, P in clouds.items():
        lab0, core0 = oracle.dbscan(P, EPS, int(name.split("_")[-1]))
        assert np.array_equal(res["1"][f"{name}_lab1"], lab0) and np.array_equal(res["1"][f"{name}_core1"], core0)
