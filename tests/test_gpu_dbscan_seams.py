"""DBSCAN's union phase over sub-cells (dbscan.hip): the hook pass looks at the 13 nearest negative
offsets only and may leave any number of trees; the compression writes one summary word per cell;
k_union_sub gives the full 62-offset treatment to the sub-cells whose 18 surrounding cells show another tree.
The clouds here are built so that each of these has to carry the result alone: neighbours that
only the far offsets reach, cells that hold several trees which must stay apart, chains as long
as the list, seams through dense material at gaps around eps. Every case is compared with the CPU
oracle for labels, core flags and the device entry point's cluster count, on a host-planned call
(a plan miss) and on the call after it (a hit where the cloud allows one)."""
import os
import re

import numpy as np
import pytest

import oracle
from pyqsm_amd import hip

pytestmark = pytest.mark.gpu

EPS = 0.1


def _f32(P):
    return np.ascontiguousarray(P, dtype=np.float64).astype(np.float32).astype(np.float64)


def _call(P, eps, min_pts, gpu, host=False, radius_inclusive=True):
    """(labels, core, cluster count, 'hit' | 'miss') of one call of the device entry point."""
    n = P.shape[0]
    d_xyz = hip.DeviceBuffer.from_array(np.ascontiguousarray(P, dtype=np.float64), gpu)
    d_lab = hip.DeviceBuffer(n * 8, gpu)
    d_core = hip.DeviceBuffer(n, gpu)
    old = os.environ.pop("PYQSM_DBSCAN_PLAN", None)
    if host:
        os.environ["PYQSM_DBSCAN_PLAN"] = "host"
    try:
        hip.prof_enable(True, gpu)
        hip.prof_reset(gpu)
        cnt = hip.dbscan_dev(d_xyz.ptr, n, eps, min_pts, d_lab.ptr, d_core.ptr, gpu, want_count=True,
                             radius_inclusive=radius_inclusive)
        hit = hip.prof_get("dbscan_plan_hit", gpu)[1]
        miss = hip.prof_get("dbscan_plan_miss", gpu)[1]
        hip.prof_enable(False, gpu)
    finally:
        os.environ.pop("PYQSM_DBSCAN_PLAN", None)
        if old is not None:
            os.environ["PYQSM_DBSCAN_PLAN"] = old
    assert hit + miss == 1
    return d_lab.download((n,), np.int64), d_core.download((n,), np.uint8).astype(bool), cnt, "hit" if hit else "miss"


def _check(P, eps, min_pts, gpu, runs=2, radius_inclusive=True, paths=("miss", "hit"), always_host=False):
    """A host-planned call (a miss that leaves this cloud's hint), then runs - 1 more; each against the
    oracle. `paths`: what the calls must report, or None where the cloud decides (fp64 records and
    compressed axes are always planned on the host)."""
    lab0, core0 = oracle.dbscan(P, eps, min_pts, radius_inclusive=radius_inclusive)
    got = []
    for i in range(runs):
        lab, core, cnt, path = _call(P, eps, min_pts, gpu, host=always_host or i == 0,
                                     radius_inclusive=radius_inclusive)
        assert np.array_equal(core, core0)
        assert np.array_equal(lab, lab0)
        assert cnt == lab0.max() + 1
        got.append(path)
    if paths is not None:
        assert got == [paths[0]] + [paths[1]] * (runs - 1)
    return lab0, core0


# ---- far offsets only ------------------------------------------------------------------------

_DIRS = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1), "xy": (1, 1, 0), "xyz": (1, 1, 1), "x-y": (1, -1, 0)}


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
    lab0, core0 = _check(P, EPS, 4, gpu, runs=3 if direction == "x" else 2)
    assert core0.all() and lab0.max() == 0      # the fixture: one row, one cluster


# ---- mixed cells -----------------------------------------------------------------------------

def _lines(rows=4, cols=4, per_line=200, seed=0):
    """rows x cols dense lines along x on a (y, z) lattice of pitch 1.5 eps, points 0.3 eps apart.
    Returns the points in line order and the line of each."""
    x = np.arange(per_line) * (0.3 * EPS)
    P, line = [], []
    for a in range(rows):
        for b in range(cols):
            P.append(np.stack([x, np.full_like(x, a * 1.5 * EPS), np.full_like(x, b * 1.5 * EPS)], -1))
            line.append(np.full(per_line, a * cols + b))
    return np.concatenate(P), np.concatenate(line)


def _bridged_lines(seed, rows=4, cols=4, per_line=200):
    """The lines plus bridge points midway between a seeded choice of lattice-adjacent line pairs (they
    see five points of either line: core, the two lines become one cluster) and points beyond a seeded
    choice of line ends that see one point only (not core: border points that join nothing)."""
    rng = np.random.default_rng(seed)
    P, _ = _lines(rows, cols, per_line)
    extra = []
    for _ in range(6):
        a, b = int(rng.integers(rows)), int(rng.integers(cols))
        along_y = bool(rng.integers(2))
        if (along_y and a == rows - 1) or (not along_y and b == cols - 1):
            continue
        x = float(rng.integers(per_line)) * 0.3 * EPS
        extra.append([x, (a + 0.5 * along_y) * 1.5 * EPS, (b + 0.5 * (not along_y)) * 1.5 * EPS])
    for _ in range(6):
        a, b = int(rng.integers(rows)), int(rng.integers(cols))
        extra.append([(per_line - 1) * 0.3 * EPS + 0.9 * EPS, a * 1.5 * EPS, b * 1.5 * EPS])
    P = np.concatenate([P, np.asarray(extra)])
    return _f32(P[rng.permutation(P.shape[0])]), len(extra)


def test_mixed_cells_stay_apart(gpu):
    P, line = _lines()
    P = _f32(P)
    lab0, core0 = _check(P, EPS, 3, gpu)
    assert core0.all() and lab0.max() + 1 == 16
    for k in range(16):                          # the fixture: one cluster per line
        assert np.unique(lab0[line == k]).size == 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_mixed_cells_with_bridges(gpu, seed):
    P, n_extra = _bridged_lines(seed)
    lab0, core0 = _check(P, EPS, 3, gpu)
    assert 1 <= lab0.max() + 1 < 16             # the fixture: some lines joined, not all
    assert 0 < (~core0).sum() < n_extra         # ... and bridge points of both kinds


# ---- one long chain --------------------------------------------------------------------------

@pytest.mark.parametrize("direction", ["+z", "-x", "+x"])
def test_one_long_chain(gpu, direction):
    # a point per sub-cell (half a cell apart), 2000 of them: every sub-cell hooks under the one before
    t = np.arange(2000) * (0.5 * EPS)
    P = np.zeros((2000, 3))
    if direction == "+z":
        P[:, 2] = t
    elif direction == "+x":
        P[:, 0] = t
    else:
        P[:, 0] = -t                              # the chain runs against the order of the indices
    lab0, core0 = _check(_f32(P), EPS, 2, gpu)
    assert core0.all() and lab0.max() == 0


# ---- seams through dense material ------------------------------------------------------------

def _slabs(axis, gap, bridged, seed):
    """Two slabs of 10 k uniform points each, `gap` eps apart along `axis`, with aligned points on the two
    faces (so that the gap itself is a distance between points), a handful of single pairs that reach
    into the gap towards each other, and noise."""
    rng = np.random.default_rng(seed)
    ext = np.array([1.0, 1.0, 1.0])
    ext[axis] = 0.3
    A = rng.uniform(0, 1, (10000, 3)) * ext
    B = rng.uniform(0, 1, (10000, 3)) * ext
    face_a = np.float64(np.float32(0.3))
    face_b = np.float64(np.float32(face_a + gap * EPS))
    B[:, axis] += face_b
    uv = rng.uniform(0, 1, (40, 3))
    fa, fb = uv.copy(), uv.copy()
    fa[:, axis] = face_a
    fb[:, axis] = face_b
    parts = [A, B, fa, fb]
    if bridged:
        uv = rng.uniform(0.1, 0.9, (5, 3))
        pa, pb = uv.copy(), uv.copy()
        pa[:, axis] = face_a + 0.04 * EPS
        pb[:, axis] = face_b - 0.04 * EPS
        parts += [pa, pb]
    noise = rng.uniform(-0.5, 1.5, (300, 3))
    noise = noise[(noise[:, axis] < face_a) | (noise[:, axis] > face_b)]   # none in the gap: it would bridge
    P = np.concatenate(parts + [noise])
    return _f32(P[rng.permutation(P.shape[0])])


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("gap,bridged", [(0.95, True), (1.0, True), (1.05, True), (0.95, False), (1.0, False), (1.05, False)])
def test_seams_through_dense_slabs(gpu, axis, gap, bridged):
    P = _slabs(axis, gap, bridged, seed=10 * axis + int(round(gap * 100)))
    _check(P, EPS, 10, gpu)


# ---- randomised differential -----------------------------------------------------------------

def _clump_cloud(seed):
    """2-6 k points in clumps of 5-40, the clumps on random walks with steps of U(0.7, 1.3) eps."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2000, 6001))
    P, centre = [], np.zeros(3)
    total = 0
    while total < n:
        if rng.random() < 0.05:
            centre = rng.uniform(-1, 1, 3) * 12 * EPS          # a new walk somewhere else
        else:
            d = rng.normal(size=3)
            centre = centre + d / np.linalg.norm(d) * rng.uniform(0.7, 1.3) * EPS
        k = int(rng.integers(5, 41))
        P.append(centre + rng.normal(size=(k, 3)) * 0.08 * EPS)
        total += k
    P = np.concatenate(P)[:n]
    return _f32(P[rng.permutation(n)])


@pytest.mark.parametrize("seed", range(20))
def test_randomised_differential(gpu, seed):
    P = _clump_cloud(seed)
    _check(P, EPS, (1, 3, 10)[seed % 3], gpu, radius_inclusive=seed % 2 == 0)


# ---- list lengths around the grouping of four ------------------------------------------------

@pytest.mark.parametrize("m", [1, 3, 4, 5, 7, 8, 9])
def test_list_lengths_around_the_grouping(gpu, m, capfd):
    # m isolated clumps, each within one sub-cell: m listed sub-cells (the trace says how many). The first
    # is a single point at the origin, which pins the grid; the others sit well inside their sub-cells.
    base = np.zeros((m - 1, 3))
    base[:, 0] = np.arange(m - 1) * 10.13 * EPS
    base += 5.2 * EPS
    step = np.arange(3)[None, :, None] * 1e-3 * EPS
    P = np.concatenate([np.zeros((1, 3)), _f32((base[:, None, :] + step).reshape(-1, 3))])
    lab0, core0 = _check(P, EPS, 1, gpu)
    assert lab0.max() + 1 == m
    os.environ["PYQSM_DBSCAN_TRACE"] = "1"
    try:
        capfd.readouterr()
        lab, core, cnt, _ = _call(P, EPS, 1, gpu)
        err = capfd.readouterr().err
    finally:
        del os.environ["PYQSM_DBSCAN_TRACE"]
    assert np.array_equal(lab, lab0) and cnt == m
    listed = [int(x) for x in re.findall(r"hook pass: (\d+) sub-cells", err)]
    assert listed and listed[-1] == m


@pytest.mark.parametrize("m", [1, 3, 4, 5, 7, 8, 9])
def test_list_lengths_single_points(gpu, m):
    P = np.zeros((m, 3))
    P[:, 1] = np.arange(m) * 3.0 * EPS
    lab0, _ = _check(_f32(P), EPS, 1, gpu)
    assert lab0.max() + 1 == m


# ---- fp64 records ----------------------------------------------------------------------------

def _not_f32(P):
    Q = P.copy()
    Q[0, 0] += 1e-9
    assert not np.array_equal(_f32(Q), Q)
    return Q


@pytest.mark.parametrize("direction", ["x", "z", "xy"])
def test_far_offsets_fp64_records(gpu, direction):
    _check(_not_f32(_far_row(direction, seed=1)), EPS, 4, gpu, paths=("miss", "miss"))


def test_mixed_cells_fp64_records(gpu):
    P, _ = _bridged_lines(4)
    _check(_not_f32(P), EPS, 3, gpu, paths=("miss", "miss"))


def test_fp64_records_forced(gpu, monkeypatch):
    monkeypatch.setenv("PYQSM_COORD_F32", "0")
    _check(_far_row("y", seed=2), EPS, 4, gpu, paths=("miss", "miss"))
    P, _ = _bridged_lines(5)
    _check(P, EPS, 3, gpu, paths=("miss", "miss"))


# ---- grids the host plans --------------------------------------------------------------------

def test_mixed_cells_host_planned(gpu):
    P, _ = _bridged_lines(6)
    _check(P, EPS, 3, gpu, paths=("miss", "miss"), always_host=True)


def test_two_groups_a_kilometre_apart(gpu):
    P, _ = _bridged_lines(7)
    Q = P.copy()
    Q[:, 0] += 1000.0
    _check(_f32(np.concatenate([P, Q])), EPS, 3, gpu, paths=None)   # compressed axis: the host plans it
