"""DBSCAN's union phase with the seams decided per CELL (dbscan.hip): the words launch folds every listed
sub-cell's root into its cell's seam word (a table indexed by the cell's directory slot), folds the runs'
smallest indices into the roots and lists the pre-roots; k_union_sub filters one leader per run of a
cell's list entries, 64 entries per wave; k_fold_roots settles the pre-roots after the seams, and the label
pass reaches a component's number in three hops.
The clouds are built so that each of these has to carry the result: runs and leaders across the wave and
block boundaries of the list, cells that must not be taken for one tree, unions that only the seam pass
finds, numbers that have to travel from a final root to a pre-root, counts around the numbering's
capacity, and the empty edges. Every case is compared with the CPU oracle for exact equality of labels,
core flags and the cluster count, on a host-planned call and on the call after it. What a fixture claims
for itself (cluster count, all core, one cell) is asserted on the oracle's result, on the CPU."""
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
C = EPS * (1.0 + 1.0 / 1048576.0)            # a cell's edge on the device; the grid's origin is the cloud's minimum
RANK_CAP = 4096


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


def _check(P, eps, min_pts, gpu, runs=2, radius_inclusive=True, paths=("miss", "hit"), prof=True, always_host=False):
    """A host-planned call (a miss that leaves this cloud's hint), then runs - 1 more; each against the
    oracle. `paths`: what the calls must report (None: the cloud decides)."""
    lab0, core0 = oracle.dbscan(P, eps, min_pts, radius_inclusive=radius_inclusive)
    got = []
    for i in range(runs):
        lab, core, cnt, path = _call(P, eps, min_pts, gpu, host=always_host or i == 0,
                                     radius_inclusive=radius_inclusive, prof=prof)
        assert np.array_equal(core, core0)
        assert np.array_equal(lab, lab0)
        assert cnt == lab0.max() + 1
        got.append(path)
    if paths is not None and prof:
        assert got == [paths[0]] + [paths[1]] * (runs - 1)
    return lab0, core0


def _listed(P, eps, min_pts, gpu, capfd):
    """Listed sub-cells of one more call, from PYQSM_DBSCAN_TRACE."""
    os.environ["PYQSM_DBSCAN_TRACE"] = "1"
    try:
        capfd.readouterr()
        _call(P, eps, min_pts, gpu)
        err = capfd.readouterr().err
    finally:
        del os.environ["PYQSM_DBSCAN_TRACE"]
    m = re.findall(r"hook pass: (\d+) sub-cells", err)
    assert m
    return int(m[-1])


def _clumps(centres, k=4, seed=0):
    """k near-coincident points (within 1e-3 eps, at or above the centre) at every centre, in centre order."""
    rng = np.random.default_rng(seed)
    centres = np.asarray(centres, dtype=np.float64)
    return (centres[:, None, :] + rng.uniform(0, 1e-3, (centres.shape[0], k, 3)) * EPS).reshape(-1, 3)


# ---- runs and leaders ------------------------------------------------------------------------

def _line(k, y=0.0):
    """k points 0.3 eps apart along x from 0."""
    P = np.zeros((k, 3))
    P[:, 0] = np.arange(k) * (0.3 * EPS)
    P[:, 1] = y
    return P


def _half_cells(P):
    """Occupied sub-cells of a cloud whose minimum is the origin: what the list holds when every point is core."""
    return np.unique(np.floor(P / (0.5 * C)).astype(np.int64), axis=0).shape[0]


def _line_with_sub_cells(m):
    """The shortest line along x that occupies m sub-cells (a point more adds one sub-cell at most)."""
    for k in range(m // 2, 4 * m + 8):
        P = _f32(_line(k))
        if _half_cells(P) == m:
            return P
    raise AssertionError(m)


@pytest.mark.parametrize("m", [63, 64, 65, 255, 256, 257])
def test_list_lengths_around_the_stretch(gpu, m, capfd):
    # one dense line: two listed sub-cells per cell, the list on either side of a wave's stretch of 64
    # entries and of a block's 256
    P = _line_with_sub_cells(m)
    lab0, core0 = _check(P, EPS, 3, gpu)
    assert core0.all() and lab0.max() == 0
    assert _listed(P, EPS, 3, gpu, capfd) == m


@pytest.mark.parametrize("lead", [0, 1, 2, 3, 4, 5])
def test_runs_across_wave_and_block_ends(gpu, lead):
    # A dense line of 1100 points behind `lead` points of an earlier grid row: the sorted positions 63 / 64 /
    # 65, 255 / 256 / 257 and 1023 / 1024 / 1025 (ends of a wave's and of a 1024-point block's share of the
    # sorted order, where the list is cut) slide over the line's cells and their two sub-cells, point by point.
    main = _line(1100, y=5.0 * EPS)
    P = _f32(np.concatenate([_line(lead), main]))
    lab0, core0 = _check(P, EPS, 3, gpu)
    assert core0[lead:].all()
    assert np.unique(lab0[lead:]).size == 1 and lab0[lead] >= 0        # the line is one cluster
    assert lab0.max() == (1 if lead >= 3 else 0)                         # ... and three points in front are one


# ---- cells that must not be taken for one tree -------------------------------------------------

_DIRS = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1), "xy": (1, 1, 0), "xyz": (1, 1, 1), "x-y": (1, -1, 0)}


def _two_blocks(direction):
    """Two 6 x 6 x 6 lattices of pitch 0.3 eps whose nearest points are 1.05 eps apart along `direction`."""
    d = np.asarray(_DIRS[direction], dtype=np.float64)
    g = np.stack(np.meshgrid(*[np.arange(6) * 0.3 * EPS] * 3, indexing="ij"), -1).reshape(-1, 3)
    shift = d * (1.5 * EPS + 1.05 * EPS / np.linalg.norm(d))
    P = np.concatenate([g, g + shift])
    rng = np.random.default_rng(3)
    perm = rng.permutation(P.shape[0])
    return _f32(P[perm]), (np.arange(P.shape[0]) >= g.shape[0])[perm]


@pytest.mark.parametrize("direction", list(_DIRS))
def test_two_clusters_just_beyond_eps(gpu, direction):
    P, second = _two_blocks(direction)
    lab0, core0 = _check(P, EPS, 5, gpu)
    assert core0.all() and lab0.max() == 1                               # the fixture: two clusters,
    assert np.unique(lab0[second]).size == 1 and np.unique(lab0[~second]).size == 1   # a block each


def _mixed_cell():
    """Two chains of clumps whose first clumps lie in ONE cell, in opposite octants 1.56 eps apart; a point
    at (-12, -12, -12) cells, below every chain, pins the grid, so that the cell is [0, C)^3. One chain leaves
    towards -x from the lower corner, the other towards +x from the upper one."""
    a = np.array([[0.05 * C - 0.8 * C * i, 0.05 * C, 0.05 * C] for i in range(12)])
    b = np.array([[0.95 * C + 0.8 * C * i, 0.95 * C, 0.95 * C] for i in range(12)])
    pin = np.full((1, 3), -12.0 * C)
    P = np.concatenate([pin, _clumps(a, seed=1), _clumps(b, seed=2) - 1e-3 * EPS])
    return _f32(P), pin[0]


def test_mixed_cell_stays_apart(gpu):
    P, pin = _mixed_cell()
    cells = np.floor((P - _f32(pin[None])[0]) / C).astype(np.int64)
    assert np.array_equal(cells[1], cells[1 + 48]) and np.array_equal(cells[1], [12, 12, 12])   # one cell
    assert np.linalg.norm(P[1] - P[1 + 48]) > 1.5 * EPS
    lab0, core0 = _check(P, EPS, 4, gpu)
    assert lab0.max() == 1 and lab0[0] == -1 and core0[1:].all()
    assert np.unique(lab0[1:49]).size == 1 and np.unique(lab0[49:]).size == 1 and lab0[1] != lab0[49]


# ---- unions only the seam pass finds -----------------------------------------------------------

def _far_row(direction, clumps=300, min_pts=4, seed=0):
    """Clumps of min_pts near-coincident points, 0.9 eps from one to the next along `direction`."""
    rng = np.random.default_rng(seed)
    d = np.asarray(_DIRS[direction], dtype=np.float64)
    d /= np.linalg.norm(d)
    centres = np.arange(clumps)[:, None] * (0.9 * EPS) * d[None, :]
    P = centres[:, None, :] + rng.uniform(-1e-3, 1e-3, (clumps, min_pts, 3)) * EPS
    return _f32(P.reshape(-1, 3)[rng.permutation(clumps * min_pts)])


@pytest.mark.parametrize("direction", list(_DIRS))
def test_far_offsets_only(gpu, direction):
    P = _far_row(direction)
    lab0, core0 = _check(P, EPS, 4, gpu)
    assert core0.all() and lab0.max() == 0      # the fixture: one row, one cluster


def _two_trees(first):
    """Two dense lines of 1500 points along x, 2.7 eps apart in y, joined at one place by two clumps 0.9 eps
    from one to the next: every step of the bridge is two sub-cells wide (0.45 + 1.8 k cells of half-cells),
    so only the 62-offset treatment finds it, and each line is a tree of its own before. `first`: the line
    that holds original index 0. A point at (-2, -2, -2) cells pins the grid."""
    y0 = 0.45 * C
    a = _line(1500, y0)
    b = _line(1500, y0 + 2.7 * EPS)
    a[:, 2] = b[:, 2] = 0.45 * C
    x = 700 * 0.3 * EPS
    bridge = _clumps([[x, y0 + 0.9 * EPS, 0.45 * C], [x, y0 + 1.8 * EPS, 0.45 * C]], seed=5)
    pin = np.full((1, 3), -2.0 * C)
    lines = [a, b] if first == 0 else [b, a]
    return _f32(np.concatenate(lines + [bridge, pin]))


@pytest.mark.parametrize("first", [0, 1])
def test_two_trees_one_far_link(gpu, first):
    # whichever of the two trees' roots ends under the other: label 0 covers both lines (the number reaches
    # the pre-root that is not final)
    P = _two_trees(first)
    lab0, core0 = _check(P, EPS, 4, gpu)
    assert core0[:-1].all() and not core0[-1]
    assert lab0[0] == 0 and (lab0[:-1] == 0).all() and lab0[-1] == -1


# ---- around the numbering's capacity -----------------------------------------------------------

def _lattice_clumps(k, pairs, seed):
    """k clumps of four points on a shuffled lattice of pitch 3.3 eps; `pairs` of them have a second clump
    0.9 eps further along x, two sub-cells away (their x index keeps the step out of the neighbouring
    sub-cell), so that only the seam pass joins it: k clusters from up to k + pairs pre-roots."""
    rng = np.random.default_rng(seed)
    side = 17
    idx = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    idx = idx[rng.permutation(len(idx))[:k]]
    centres = idx * (3.3 * EPS)
    frac = (2.0 * idx[:, 0] * 3.3) % 1.0
    ok = np.flatnonzero((frac > 0.25) & (frac < 0.9))
    extra = centres[ok[:pairs]] + [0.9 * EPS, 0.0, 0.0]
    assert extra.shape[0] == pairs
    P = _clumps(np.concatenate([centres, extra]), seed=seed)
    return _f32(P[rng.permutation(P.shape[0])])


@pytest.mark.parametrize("k,pairs", [(RANK_CAP - 1, 0), (RANK_CAP, 0), (RANK_CAP + 1, 0), (RANK_CAP - 6, 8),
                                     (RANK_CAP, 3), (RANK_CAP + 1, 3)])
def test_counts_around_the_rank_capacity(gpu, k, pairs):
    P = _lattice_clumps(k, pairs, 50 + k + pairs)
    lab0, core0 = _check(P, EPS, 4, gpu)
    assert core0.all() and lab0.max() + 1 == k


# ---- the empty edges ---------------------------------------------------------------------------

def test_no_core_point(gpu):
    P = _f32(np.random.default_rng(9).uniform(0, 1, (50, 3)))
    lab0, core0 = _check(P, EPS, 10, gpu)
    assert not core0.any() and lab0.max() == -1


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("min_pts", [1, 2, 4])
def test_tiny_clouds(gpu, n, min_pts):
    P = _f32(np.arange(3 * n, dtype=np.float64).reshape(n, 3) * 0.1 * EPS)   # 0.52 eps from one to the next
    _check(P, EPS, min_pts, gpu)


def test_empty_and_single_entry_non_core_list(gpu):
    P = _f32(_line(400))
    lab0, core0 = _check(P, EPS, 3, gpu)
    assert core0.all()                                                       # nothing for the label pass's list
    Q = _f32(np.concatenate([_line(400), [[399 * 0.3 * EPS + 0.9 * EPS, 0.0, 0.0]]]))
    lab0, core0 = _check(Q, EPS, 3, gpu)
    assert (~core0).sum() == 1 and lab0[-1] == 0                             # one border point


# ---- paths -------------------------------------------------------------------------------------

def _not_f32(P):
    Q = P.copy()
    Q[0, 0] += 1e-9
    assert not np.array_equal(_f32(Q), Q)
    return Q


def _clump_cloud(seed, lo=2000, hi=5001):
    """2-5 k points: clumps of 5-40 on random walks with steps of U(0.3, 1.3) eps (blobs), dense lines along
    random directions, and strays."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(lo, hi))
    P, centre, total = [], np.zeros(3), 0
    while total < n:
        u = rng.random()
        if u < 0.05:
            centre = rng.uniform(-1, 1, 3) * 10 * EPS              # a new walk somewhere else
        elif u < 0.10:
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            k = int(rng.integers(10, 80))
            P.append(centre + np.arange(k)[:, None] * 0.3 * EPS * d)   # a line
            centre = centre + k * 0.3 * EPS * d
            total += k
            continue
        elif u < 0.15:
            P.append(rng.uniform(-1, 1, (3, 3)) * 12 * EPS)         # strays
            total += 3
            continue
        else:
            d = rng.normal(size=3)
            centre = centre + d / np.linalg.norm(d) * rng.uniform(0.3, 1.3) * EPS
        k = int(rng.integers(5, 41))
        P.append(centre + rng.normal(size=(k, 3)) * 0.08 * EPS)
        total += k
    P = np.concatenate(P)[:n]
    return _f32(P[rng.permutation(n)])


def test_fp64_records(gpu):
    _check(_not_f32(_two_trees(1)), EPS, 4, gpu, paths=("miss", "miss"))
    _check(_not_f32(_far_row("xy", seed=1)), EPS, 4, gpu, paths=("miss", "miss"))
    _check(_not_f32(_mixed_cell()[0]), EPS, 4, gpu, paths=("miss", "miss"))


def test_strict_radius(gpu):
    _check(_two_trees(0), EPS, 4, gpu, radius_inclusive=False)
    _check(_clump_cloud(11), EPS, 5, gpu, radius_inclusive=False)


def test_doubled_cell_path(gpu, monkeypatch):
    # groups along the space diagonal occupy so many slabs per axis that the grid doubles its cells: the
    # per-point union-find, whose points name their root at once (the label pass's three hops end there)
    monkeypatch.setenv("PYQSM_DBSCAN_PLAN", "host")
    rng = np.random.default_rng(36)
    centres = np.cumsum(rng.uniform(0.6, 2.0, 800) * EPS)[:, None] * [1.0, 1.0, 1.0]
    sizes = rng.integers(1, 6, 800)
    P = np.concatenate([c + rng.uniform(0, 0.3 * EPS, (s, 3)) for c, s in zip(centres, sizes)])
    P = P[rng.permutation(len(P))]
    hip.prof_enable(True, gpu)
    hip.prof_reset(gpu)
    lab0, core0 = oracle.dbscan(P, EPS, 2)
    lab, core = hip.dbscan(P, EPS, 2, device=gpu)
    hooks = hip.prof_get("k_hook_sub", gpu)[1]
    hip.prof_enable(False, gpu)
    assert np.array_equal(lab, lab0) and np.array_equal(core, core0)
    assert hooks == 0  # not the sub-cell path


def test_compressed_axes(gpu):
    P = _two_trees(0)
    Q = P.copy()
    Q[:, 0] += 1000.0
    lab0, _ = _check(_f32(np.concatenate([P, Q])), EPS, 4, gpu, paths=None)   # the host plans it
    assert lab0.max() == 1


def test_profiling_on_and_off(gpu):
    P = _clump_cloud(31)
    _check(P, EPS, 5, gpu, prof=True)
    _check(P, EPS, 5, gpu, prof=False)


# ---- randomised differential -------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(30))
def test_randomised_differential(gpu, seed):
    P = _clump_cloud(100 + seed)
    _check(P, EPS, (1, 3, 5, 10)[seed % 4], gpu, radius_inclusive=seed % 3 != 0)


# ---- without second links ----------------------------------------------------------------------

_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from pyqsm_amd import hip, _lib
_lib.require_gpu(0)
clouds = np.load(sys.argv[2])
out = {}
for name in clouds.files:
    for rep in range(2):
        lab, core = hip.dbscan(clouds[name], 0.1, 4)
        out[f"{name}_lab{rep}"], out[f"{name}_core{rep}"] = lab, core
np.savez(sys.argv[3], **out)
"""


def test_without_second_links(gpu, tmp_path):
    # PYQSM_DBSCAN_LINK2 is read once per process: a fresh process, whose words launch is the one that
    # reaches the roots (and carries the list of non-core points)
    clouds = {"trees": _two_trees(1), "mixed": _mixed_cell()[0], "far": _far_row("x-y"), "walks": _clump_cloud(7)}
    np.savez(tmp_path / "clouds.npz", **clouds)
    (tmp_path / "run.py").write_text(_CHILD)
    env = dict(os.environ, PYQSM_DBSCAN_LINK2="0")
    env.pop("PYQSM_DBSCAN_TRACE", None)
    r = subprocess.run([sys.executable, str(tmp_path / "run.py"), ROOT, str(tmp_path / "clouds.npz"),
                        str(tmp_path / "out.npz")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    res = np.load(tmp_path / "out.npz")
    for name, P in clouds.items():
        lab0, core0 = oracle.dbscan(P, EPS, 4)
        for rep in range(2):
            assert np.array_equal(res[f"{name}_lab{rep}"], lab0), name
            assert np.array_equal(res[f"{name}_core{rep}"], core0), name
