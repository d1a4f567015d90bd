"""The shared grid's plan, restated on the CPU (pyqsm_amd/csrc/grid.hip), and the clouds of
tests/test_gpu_grid_classes.py.

The size of the cell directory decides which binning kernels run. The classes, by the number of
cells of the dense grid (border included):

``fused``     ncell < 2^24                    k_bk_scatter scans the bucket totals itself
``scan``      2^24 <= ncell, ncell + 1 <= 2^26  k_bk_scan, k_bk_scatter reading bstart
``bucket13``  ncell + 1 > 2^26, ncell < 2^27  buckets of 8192 cells (k_bk_sort<13, .>)
``atomic``    2^27 <= ncell <= 2^28           one atomic per point, the directory scanned

``dbscan_plan``     follows bin_octants_host: cells of eps (1 + 2^-20) from the cloud's minimum, one
                    border cell on every side, per-axis compression (k_axis_occ / k_axis_keep /
                    k_axis_shift) when the dense grid would exceed 2^28 cells, the edge doubled when
                    the compressed grid is still too large.
``build_grid_plan`` follows build_grid (kNN, the fixed-radius queries, features, normals): no
                    compression, the edge doubled until the dense grid fits.
``robust_box_cuts`` the first round of robust_box, which the callers of build_grid run on the
                    bounding box: whether it would cut an axis.

Every GPU test of the grid's classes asserts from here that its cloud is in the class it claims and
has the bucket and cell populations it claims; tests/test_grid_restatement_host.py asserts the same
for every cloud without a GPU. Plain NumPy; nothing here touches the library.
"""
from collections import namedtuple

import numpy as np

MAX_CELLS = 1 << 28          # dbscan.hip, radius_grid, feature_grid, normals.hip: max_cells
BK_MAX = 16384               # grid.hip: kBkMax, buckets of a launch
BK_FUSED = 4096              # grid.hip: kBkFusedScan
BK_PER = 12                  # grid.hip: kBkPer, points per thread of k_bk_sort in registers
BK_BIG = 255                 # grid.hip: kBkBig, cells above it are ordered by the whole block
BIG_CELL = 128               # grid.hip: kBigCell, the same on the atomic path
CLASSES = ("fused", "scan", "bucket13", "atomic")

Plan = namedtuple("Plan", "cls mapped doubled dims ncell bits nbk cell mn cells")


def tile(bits):
    """Points of a bucket that k_bk_sort<bits, .> keeps in registers: (2^bits / 8) threads * kBkPer."""
    return ((1 << bits) // 8) * BK_PER


def size_class(ncell):
    """(class, bits, nbk) of a directory of ncell cells (grid.hip: bucket_shape, as bin_octants_host,
    bucketed_fits and the device's write_plan read it)."""
    ncell = int(ncell)
    bits = 12 if ncell + 1 <= (BK_MAX << 12) else 13
    nbk = (ncell + (1 << bits)) >> bits
    if nbk > BK_MAX:
        cls = "atomic"
    elif bits == 13:
        cls = "bucket13"
    elif nbk > BK_FUSED:
        cls = "scan"
    else:
        cls = "fused"
    return cls, bits, nbk


def _axis_map(c, m):
    """k_axis_occ / k_axis_keep / exclusive scan / k_axis_shift for one axis: c the raw slab of
    every point, m the number of raw slabs. A slab is kept when it holds a point or follows one that
    does; (compressed index of every raw slab with the border's + 1, slabs kept)."""
    occ = np.bincount(c, minlength=m)[:m] > 0
    keep = occ.copy()
    keep[1:] |= occ[:-1]
    keep = keep.astype(np.int64)
    return np.cumsum(keep) - keep + 1, int(keep.sum())


def dbscan_plan(P, eps, max_cells=MAX_CELLS):
    P = np.asarray(P, np.float64)
    mn, mx = P.min(0), P.max(0)
    cell = eps * (1.0 + 2.0 ** -20)
    doubled = False
    while True:
        raw = (np.floor((mx - mn) / cell) + 1.0).astype(np.int64)
        dims = raw + 2
        c = np.floor((P - mn) * (1.0 / cell)).astype(np.int64)
        c = np.clip(c, 0, raw - 1)
        if float(np.prod(dims.astype(np.float64))) <= float(max_cells):
            mapped = False
            c = c + 1
            break
        if int(raw.sum()) <= (1 << 27):
            maps = [_axis_map(c[:, a], int(raw[a])) for a in range(3)]
            cdims = np.array([kept + 2 for _, kept in maps], np.int64)
            if float(np.prod(cdims.astype(np.float64))) <= float(max_cells):
                mapped = True
                dims = cdims
                c = np.stack([maps[a][0][c[:, a]] for a in range(3)], 1)
                break
        cell *= 2.0
        doubled = True
    ncell = int(dims[0]) * int(dims[1]) * int(dims[2])
    cls, bits, nbk = size_class(ncell)
    cells = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    return Plan(cls, mapped, doubled, tuple(int(d) for d in dims), ncell, bits, nbk, cell, mn, cells)


def build_grid_plan(box, cell, max_cells=MAX_CELLS, P=None):
    """box = (mn[3], mx[3]); with P, the cell of every point as well (clamped_cell)."""
    mn, mx = np.asarray(box[0], np.float64), np.asarray(box[1], np.float64)
    cell = float(cell)
    doubled = False
    while True:
        dims = np.floor((mx - mn) / cell) + 3.0
        if float(np.prod(dims)) <= float(max_cells):
            break
        cell *= 2.0
        doubled = True
    dims = dims.astype(np.int64)
    ncell = int(dims[0]) * int(dims[1]) * int(dims[2])
    cls, bits, nbk = size_class(ncell)
    cells = None
    if P is not None:
        cells = point_cells(P, mn, cell, dims)
    return Plan(cls, False, doubled, tuple(int(d) for d in dims), ncell, bits, nbk, cell, mn, cells)


def point_cells(Q, mn, cell, dims):
    """grid.hpp: cell_index, for source points and for queries alike (clamped into the interior)."""
    dims = np.asarray(dims, np.int64)
    c = np.floor((np.asarray(Q, np.float64) - mn) * (1.0 / cell))
    c = np.clip(c, 0.0, (dims - 3).astype(np.float64)).astype(np.int64) + 1
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]


def radius_plan(P, radius):
    """The grid radius_grid / feature_grid / normals.hip build over P, given that robust_box leaves
    the bounding box alone (robust_box_cuts says whether it does)."""
    P = np.asarray(P, np.float64)
    return build_grid_plan((P.min(0), P.max(0)), radius * (1.0 + 2.0 ** -20), MAX_CELLS, P)


def robust_box_cuts(P):
    """robust_box's first round on the bounding box with the budget its callers give it: histograms
    of 64 bins per axis over every fourth point (counted four times); an axis is cut when bins
    holding at most budget / 3 points at either end make up a quarter of its length."""
    P = np.asarray(P, np.float64)
    n = len(P)
    budget = min(8192, max(256, n // 256))
    if n < 64:
        return False
    side = budget // 3
    mn, mx = P.min(0), P.max(0)
    S = P[::4]
    for a in range(3):
        e = mx[a] - mn[a]
        if not e > 0:
            continue
        b = np.clip(np.floor((S[:, a] - mn[a]) * (64.0 / e)), 0, 63).astype(np.int64)
        h = 4 * np.bincount(b, minlength=64)
        lo, hi, acc = 0, 63, 0
        while lo < hi and acc + h[lo] <= side:
            acc += h[lo]
            lo += 1
        acc = 0
        while hi > lo and acc + h[hi] <= side:
            acc += h[hi]
            hi -= 1
        if hi - lo + 1 <= 48:
            return True
    return False


def populations(plan):
    """(points per bucket, the largest cell's population) of a plan that carries its points' cells."""
    bucket = np.bincount(plan.cells >> plan.bits, minlength=plan.nbk)
    return bucket, int(np.bincount(np.unique(plan.cells, return_inverse=True)[1]).max())


# ---- the clouds ------------------------------------------------------------------------------------

def _f32(P):
    return np.ascontiguousarray(np.asarray(P, np.float64).astype(np.float32).astype(np.float64))


def clumps(n_clumps, per, extent, sigma, seed, nudge=False):
    """n_clumps centres uniform in [0, extent]^3 (extent a number or one per axis), `per` Gaussian
    points of deviation sigma around each; coordinates fp32-representable. nudge: one coordinate
    moved by 1e-9, which makes the cloud non-representable in fp32."""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(0.0, 1.0, (n_clumps, 3)) * np.asarray(extent, np.float64)
    P = _f32(np.repeat(ctr, per, axis=0) + rng.normal(0.0, sigma, (n_clumps * per, 3)))
    return nudged(P) if nudge else P


def nudged(P, row=123, axis=1):
    Q = P.copy()
    Q[row, axis] += 1e-9
    assert np.float64(np.float32(Q[row, axis])) != Q[row, axis]
    return Q


EPS, MIN_PTS = 0.02, 6
# extent of the clumps' box and points of the dense slab, per class
CLASS_EXTENT = {"scan": 8.0, "bucket13": 9.5, "atomic": 12.0}
CLASS_SLAB = {"scan": 20_000, "bucket13": 40_000, "atomic": 8_000}


def class_cloud(cls, nudge=False, light=False):
    """One cloud per large class at eps (or radius) 0.02: 1500 sparse clumps (buckets of at most 64
    points), a dense slab along x (a bucket beyond the register tile), a short slab (a bucket
    between 65 points and the tile), a blob with cells of more than 255 points, and a clump in each
    of the box's two corners (points in the first and the last interior cell). light: the same
    box without the slabs and with a blob of 600 points, for the slower CPU restatements."""
    ext = CLASS_EXTENT[cls]
    rng = np.random.default_rng(int(ext * 10))
    parts = [clumps(1500, 16, ext - 0.4, 0.012, seed=int(ext * 10) + 1) + 0.2]
    parts.append(rng.uniform(0, 1, (CLASS_SLAB[cls], 3)) * [ext - 0.4, 0.1, 0.01] + [0.2, 0.37 * ext, 0.61 * ext])
    parts.append(rng.uniform(0, 1, (1500, 3)) * [1.0, 0.05, 0.01] + [0.2 * ext, 0.8 * ext, 0.15 * ext])
    parts.append(rng.uniform(0, 1, (2500, 3)) * 0.03 + [0.7 * ext, 0.2 * ext, 0.3 * ext])
    if light:
        parts[1:] = [parts[3][:600]]
    parts.append(rng.uniform(0, 1, (8, 3)) * 0.008)
    parts.append(rng.uniform(0, 1, (8, 3)) * 0.008 + (ext - 0.008))
    P = _f32(np.concatenate(parts))
    P = P[rng.permutation(len(P))]
    return nudged(P) if nudge else P


# dims of the directory on either side of every threshold -> (class, bits, nbk)
THRESHOLD_DIMS = {
    (255, 256, 257): ("fused", 12, 4096),
    (256, 256, 256): ("scan", 12, 4097),
    (406, 406, 407): ("scan", 12, 16379),
    (407, 407, 406): ("bucket13", 13, 8210),
    (511, 512, 513): ("bucket13", 13, 16384),
    (512, 512, 512): ("atomic", 13, 16385),
    (645, 645, 645): ("atomic", 13, 32756),
}
THRESHOLD_NCELL = {(255, 256, 257): 16_776_960, (256, 256, 256): 16_777_216, (406, 406, 407): 67_088_252,
                   (407, 407, 406): 67_253_494, (511, 512, 513): 134_217_216, (512, 512, 512): 134_217_728,
                   (645, 645, 645): 268_336_125}


def threshold_cloud(dims, eps=EPS):
    """A directory of exactly `dims` cells: two corner points (noise, far from everything) at the
    origin and at (d - 3 + 0.5) cells per axis, 150 clumps inside, and 24 points in the
    highest-numbered interior cells (the last y row of the last z slab), 1.7 cells and more from the
    corner point."""
    cell = eps * (1.0 + 2.0 ** -20)
    d = np.asarray(dims, np.float64)
    top = (d - 2.5) * cell
    rng = np.random.default_rng(int(d.sum()))
    inner = clumps(150, 16, top - 0.3, 0.012, seed=int(d.sum()) + 1) + 0.15
    last = (d - 3.0) * cell + rng.uniform(0.05, 0.45, (24, 3)) * cell
    last[:, 0] = (d[0] - 3.0 - rng.uniform(1.3, 4.0, 24)) * cell
    return _f32(np.concatenate([[[0.0, 0.0, 0.0]], inner, last, [top]]))


# dash and gap in cells, slabs along the diagonal -> class of the compressed directory
DASHES = {"atomic": (3, 5, 900), "scan": (2, 6, 700), "bucket13": (3, 6, 900)}


def dashed_diagonal(cls, eps=EPS, per=40, nudge=False):
    """Dashes along the space diagonal: `per` points on every run of `dash` cells, jittered by 0.3
    cell, `gap` empty cells between runs; every axis compresses by the same ratio."""
    dash, gap, slabs = DASHES[cls]
    cell = eps * (1.0 + 2.0 ** -20)
    rng = np.random.default_rng(dash * 100 + gap)
    start = np.arange(0, slabs - dash, dash + gap, dtype=np.float64)
    t = np.repeat(start, per) + rng.uniform(0.3, dash - 0.3, len(start) * per)
    P = _f32((t[:, None] + rng.uniform(-0.3, 0.3, (len(t), 3))) * cell)
    return nudged(P) if nudge else P


def query_set(P, plan, m, seed):
    """m queries for a grid over P: source points with a jitter, queries in the grid's last interior
    cells, and queries outside the box on every side, within reach of it and far away."""
    rng = np.random.default_rng(seed)
    mn, mx = P.min(0), P.max(0)
    r = plan.cell
    special = [mx - rng.uniform(0.0, 0.5, (8, 3)) * r]                     # the last interior cells
    for a in range(3):
        for sign, edge in ((-1.0, mn), (1.0, mx)):
            near = edge.copy()
            near[a] += sign * 0.4 * r                                       # outside, points within reach
            far = 0.5 * (mn + mx)
            far[a] = edge[a] + sign * 50.0                                  # outside, nothing in reach
            special += [near[None], far[None]]
    special = np.concatenate(special)
    pick = rng.choice(len(P), m - len(special), replace=False)
    Q = np.concatenate([P[pick] + rng.normal(0.0, 0.3 * r, (len(pick), 3)), special])
    return _f32(Q[rng.permutation(len(Q))])


def big_cell_cloud():
    """tests/test_gpu_dbscan_plan.py::test_cells_of_more_than_255_points (eps 0.1, min_pts 10)."""
    rng = np.random.default_rng(3)
    P = _f32(rng.uniform(0, 0.15, (8000, 3)))
    return np.concatenate([P, _f32(rng.uniform(0.5, 1.0, (2000, 3)))])


def axis_mapped_cloud():
    """tests/test_gpu_dbscan_plan.py::test_axis_mapped_cloud_after_the_forest (eps 0.03, min_pts 4)."""
    rng = np.random.default_rng(11)
    blob = rng.uniform(0, 0.6, (6000, 3))
    far = rng.uniform(-50, 50, (40, 3))
    return _f32(np.concatenate([blob, far]))


# populations of one bucket on either side of the 4096 cells of a bucket and of tile(12), the points
# k_bk_sort_plain<12, .> keeps in registers, up to ten rounds of the tile (below 1500 points
# robust_box cuts the slab's box)
ONE_BUCKET_SIZES = (1500, 4096, 4097, 6143, 6144, 6145, 8193, 60_000)
ONE_BUCKET_RADIUS = 0.1


def one_bucket_slab(m, seed=0):
    """tests/test_gpu_dbscan_buckets.py::slab: 40 x 0.3 x 0.1, a single bucket of a grid of edge 0.1."""
    rng = np.random.default_rng(seed)
    return _f32(rng.uniform(0, 1, (m, 3)) * [40, 0.3, 0.1])


# ---- what every cloud claims -----------------------------------------------------------------------

def claim_class_cloud(P, cls):
    """The DBSCAN grid and the radius grid of a class cloud; returns both plans."""
    pl = dbscan_plan(P, EPS)
    assert (pl.cls, pl.mapped, pl.doubled) == (cls, False, False), pl[:7]
    pop, big = populations(pl)
    assert big > BK_BIG > BIG_CELL, "a cell beyond kBkBig (and kBigCell)"
    if cls != "atomic":                                    # (the atomic path has no buckets)
        assert pl.bits == (12 if cls == "scan" else 13)
        assert ((pop > 0) & (pop <= 64)).sum() >= 1000, "buckets of a wave's worth of points"
        assert ((pop > 64) & (pop <= tile(pl.bits))).sum() >= 2, "buckets between 65 points and the tile"
        assert pop.max() > tile(pl.bits), "a bucket beyond the register tile"
    last = pl.ncell - 1 - (pl.dims[0] * pl.dims[1] + pl.dims[0] + 1)
    assert (pl.cells == last).sum() >= 1, "a point in the highest-numbered interior cell"
    rp = radius_plan(P, EPS)
    assert not robust_box_cuts(P), "the radius grid is built over the bounding box"
    assert (rp.cls, rp.doubled) == (cls, False), rp[:7]
    last = rp.ncell - 1 - (rp.dims[0] * rp.dims[1] + rp.dims[0] + 1)
    assert (rp.cells == last).sum() >= 1
    return pl, rp


def claim_threshold_cloud(P, dims):
    pl = dbscan_plan(P, EPS)
    assert pl.dims == tuple(dims) and pl.ncell == THRESHOLD_NCELL[tuple(dims)]
    assert (pl.cls, pl.bits, pl.nbk) == THRESHOLD_DIMS[tuple(dims)]
    assert not pl.mapped and not pl.doubled
    nx, ny, nz = pl.dims
    last_row = ((nz - 2) * ny + (ny - 2)) * nx               # the last y row of the last z slab
    in_row = (pl.cells >= last_row + 1) & (pl.cells <= last_row + nx - 2)
    assert in_row.sum() >= 20 and (pl.cells == last_row + nx - 2).sum() == 1
    # (the buckets after this row's hold border cells alone: their directory entries are all n)
    assert (pl.cells >> pl.bits).max() == (last_row + nx - 2) >> pl.bits
    return pl


def claim_dashed(P, cls):
    pl = dbscan_plan(P, EPS)
    assert (pl.cls, pl.mapped, pl.doubled) == (cls, True, False), pl[:7]
    assert 3500 <= len(P) <= 6000
    return pl


def claim_one_bucket_slab(P, m):
    """The radius grid of the slab is of the fused class, over the whole bounding box, and all m
    points share one bucket of it."""
    rp = radius_plan(P, ONE_BUCKET_RADIUS)
    assert (rp.cls, rp.bits, rp.doubled) == ("fused", 12, False), rp[:7]
    pop, _ = populations(rp)
    assert pop[pop > 0].tolist() == [m] == [len(P)], "exactly one bucket holds points: all of them"
    assert not robust_box_cuts(P), "the radius grid is built over the bounding box"
    return rp


def claim_queries(Q, P, rp):
    """The query set reaches the last interior cells and lies outside the box on every side."""
    mn, mx = P.min(0), P.max(0)
    last = rp.ncell - 1 - (rp.dims[0] * rp.dims[1] + rp.dims[0] + 1)
    assert (point_cells(Q, rp.mn, rp.cell, rp.dims) == last).sum() >= 4
    for a in range(3):
        assert (Q[:, a] < mn[a]).sum() >= 2 and (Q[:, a] > mx[a]).sum() >= 2
