"""NumPy/SciPy restatement of the detail-recovery contract (include/pyqsm_hip.h, "voxel-grid
occupancy" and pyqsm_radius_reduce).

Open3D's VoxelGrid.create_from_point_cloud / check_if_included, recollected from Open3D, parity
unpinned: this file is what defines them for pyqsm_amd/csrc/voxelgrid.hip.

* A voxel index is ``floor((p - origin) / voxel_size)`` with ``origin = min_bound - voxel_size / 2``,
  one fp64 division per coordinate: the arithmetic of tests/clean_restatement.py, so a cloud's grid
  and its down-sampling have the same voxels in the same row order (rows by smallest member index).
* Colour means are accumulated with ``np.add.at`` into zeros: one member at a time, ascending index.
* The reduction takes its neighbours from ``cKDTree.query`` with a distance bound, recomputes
  ``d2 = ((dx*dx) + dy*dy) + dz*dz`` in fp64, keeps ``d2 < radius*radius``, re-sorts by (d2, index),
  keeps the first k and folds the values one neighbour at a time.
"""
from __future__ import annotations

import functools

import numpy as np

LIMIT_DIM = 2 ** 31 - 1
LIMIT_CELLS = 2 ** 62


class VoxelRangeError(ValueError):
    """A grid dimension above 2^31 - 1, or more than 2^62 cells."""


class Grid:
    """origin f64 [3], voxel_size, dims [3] (Python ints), keys (ascending, one per voxel), rows
    (row of the voxel at each sorted position), grid_index int32 [M,3] and colors in row order."""

    def __init__(self, origin, voxel_size, dims, keys, rows, grid_index, colors):
        self.origin, self.voxel_size, self.dims = origin, voxel_size, dims
        self.keys, self.rows, self.grid_index, self.colors = keys, rows, grid_index, colors
        self.n_voxels = len(keys)
        self.cells = dims[0] * dims[1] * dims[2]


def _key(k3, dims):
    # Python-int strides: up to 2^62 cells fit int64
    return k3[:, 0] + np.int64(dims[0]) * (k3[:, 1] + np.int64(dims[1]) * k3[:, 2])


def voxel_grid(P, voxel_size, C=None) -> Grid:
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    if not (np.isfinite(voxel_size) and voxel_size > 0):
        raise ValueError("voxel_size must be positive and finite")
    if not np.isfinite(P).all():
        raise ValueError("non-finite coordinate")
    n = len(P)
    if n == 0:
        origin = np.zeros(3) - voxel_size * 0.5
        return Grid(origin, float(voxel_size), [0, 0, 0], np.zeros(0, np.int64), np.zeros(0, np.int64),
                    np.zeros((0, 3), np.int32), None if C is None else np.zeros((0, 3)))
    origin = P.min(axis=0) - voxel_size * 0.5
    f3 = np.floor((P - origin) / voxel_size)
    top = f3.max(axis=0)
    if not np.all(top < float(LIMIT_DIM)):
        raise VoxelRangeError("more than 2^31 - 1 voxels along an axis")
    dims = [int(t) + 1 for t in top]
    if dims[0] * dims[1] * dims[2] > LIMIT_CELLS:
        raise VoxelRangeError("more than 2^62 cells")
    k3 = f3.astype(np.int64)
    keys, first, inv_u = np.unique(_key(k3, dims), return_index=True, return_inverse=True)
    inv_u = inv_u.reshape(-1)
    m = len(keys)
    rows = np.empty(m, dtype=np.int64)
    rows[np.argsort(first, kind="stable")] = np.arange(m)   # rank of each voxel's smallest member
    grid_index = np.empty((m, 3), dtype=np.int32)
    grid_index[rows] = k3[first]
    colors = None
    if C is not None:
        inverse = rows[inv_u]
        sums = np.zeros((m, 3))
        np.add.at(sums, inverse, np.asarray(C, dtype=np.float64).reshape(-1, 3))
        colors = sums / np.bincount(inverse, minlength=m)[:, None].astype(np.float64)
    return Grid(origin, float(voxel_size), dims, keys, rows, grid_index, colors)


def query(g: Grid, Q, invert=False):
    """(included bool [m], row int32 [m] (-1: none), idx int64: the ascending indices that are
    included, or with invert those that are not, box bool [m]: inside the grid's box)."""
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 3)
    m = len(Q)
    with np.errstate(invalid="ignore"):
        f3 = np.floor((Q - g.origin) / g.voxel_size)
        box = np.all((f3 >= 0) & (f3 < np.asarray(g.dims, dtype=np.float64)), axis=1)
    row = np.full(m, -1, dtype=np.int32)
    if g.n_voxels and box.any():
        k = _key(f3[box].astype(np.int64), g.dims)
        pos = np.searchsorted(g.keys, k)
        pos[pos == g.n_voxels] = 0
        hit = g.keys[pos] == k
        row[np.flatnonzero(box)[hit]] = g.rows[pos[hit]]
    included = row >= 0
    return included, row, np.flatnonzero(included != bool(invert)).astype(np.int64), box


def neighbours(src, qry, radius, k, workers=-1):
    """(idx int64 [m,k] padded with n, counts int32 [m], in_range [m]): per query the source points
    with d2 < radius*radius, the first k by (d2, index); in_range counts them before the cut at k
    (exact up to k + 8)."""
    from scipy.spatial import cKDTree
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    qry = np.asarray(qry, dtype=np.float64).reshape(-1, 3)
    n, m = len(src), len(qry)
    tree = cKDTree(src)
    full = min(n, k + 8)   # cKDTree's own rounding may order near-ties at the k-th place differently
    kk = min(full, 64)     # a narrow table first: k = 500 at 5 cm finds a few dozen
    while True:
        _, idx = tree.query(qry, kk, distance_upper_bound=radius * (1 + 1e-9), workers=workers)
        idx = np.asarray(idx).reshape(m, kk)
        if kk == full or (idx[:, -1] >= n).all():
            break
        kk = full
    pad = idx >= n
    s = src[np.where(pad, 0, idx)]
    dx, dy, dz = s[..., 0] - qry[:, None, 0], s[..., 1] - qry[:, None, 1], s[..., 2] - qry[:, None, 2]
    d2 = ((dx * dx) + dy * dy) + dz * dz
    out = pad | ~(d2 < radius * radius)
    d2 = np.where(out, np.inf, d2)
    idx = np.where(out, n, idx)
    order = np.lexsort((idx, d2), axis=1)
    idx = np.take_along_axis(idx, order, axis=1)
    in_range = (idx < n).sum(axis=1)
    if kk < k:
        idx = np.concatenate([idx, np.full((m, k - kk), n, dtype=idx.dtype)], axis=1)
    idx = idx[:, :k].astype(np.int64)
    return idx, np.minimum(in_range, k).astype(np.int32), in_range


def reduce_values(idx, counts, values, reducer, empty_row=0):
    """out f64 [m,F]: values [n,F] folded over each row's first counts[j] neighbours, one at a time in
    their order. mean: sum from 0.0, divided by the count. min / max: NaN if any value is NaN, else
    the first value replaced by every strictly smaller / larger one. first: the nearest's row."""
    values = np.asarray(values, dtype=np.float64)
    values = values.reshape(len(values), -1)
    m, F = len(idx), values.shape[1]
    acc = np.zeros((m, F))
    nan = np.zeros((m, F), dtype=bool)
    for t in range(int(counts.max()) if m else 0):
        live = counts > t
        v = values[idx[live, t]]
        if reducer == "mean":
            acc[live] = acc[live] + v
        elif reducer == "first":
            if t == 0:
                acc[live] = v
        else:
            a = acc[live]
            nan[live] |= np.isnan(v)
            with np.errstate(invalid="ignore"):
                take = (v < a) if reducer == "min" else (v > a)
            if t == 0:
                take = np.ones_like(take)
            acc[live] = np.where(take, v, a)
    has = counts > 0
    if reducer == "mean":
        acc[has] = acc[has] / counts[has, None].astype(np.float64)
    acc[nan] = np.nan
    acc[~has] = values[empty_row] if empty_row >= 0 else np.nan
    return acc


def lattice():
    """(points, queries): a 0.25 lattice, every point exactly on voxel faces of a 0.25 grid (origin is
    min - 0.125, all of it exact in binary), every other cell of it left out; queries at the voxels'
    corners, at their centres and half a voxel outside the box on every side."""
    ax = np.arange(6) * 0.25
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    pts = g[(np.rint(g / 0.25).astype(int).sum(axis=1) % 2) == 0]
    cx = np.arange(-1, 7) * 0.25 - 0.125                       # voxel corners, one layer outside included
    corners = np.stack(np.meshgrid(cx, cx, cx, indexing="ij"), -1).reshape(-1, 3)
    centres = corners + 0.125
    lo, hi = -0.125 - 0.125, 1.375 + 0.125
    mid = 0.5
    outside = np.array([[lo, mid, mid], [hi, mid, mid], [mid, lo, mid], [mid, hi, mid], [mid, mid, lo], [mid, mid, hi]])
    return pts, np.concatenate([corners, centres, outside])


# ---- the inputs the GPU tests share (built once per process) ---------------------------------

@functools.lru_cache(maxsize=None)
def detail_inputs():
    """(tile [200000,3], tree [50000,3]: the tile's first tree, comp [12500,3]: every fourth point of
    that tree)."""
    from pyqsm_amd import synth
    tile = synth.forest(200_000, seed=3)
    lo = tile[:, :2].min(axis=0)
    tree = tile[(tile[:, 0] < lo[0] + 8.5) & (tile[:, 1] < lo[1] + 8.5)]
    comp = np.ascontiguousarray(tree[::4])
    for a in (tile, tree, comp):
        a.setflags(write=False)
    return tile, tree, comp


@functools.lru_cache(maxsize=None)
def detail_grid(voxel_size, colored=False):
    tile, _, comp = detail_inputs()
    col = detail_colors() if colored else None
    g = voxel_grid(comp, voxel_size, col)
    return g, query(g, tile)


@functools.lru_cache(maxsize=None)
def detail_colors():
    _, _, comp = detail_inputs()
    c = np.random.default_rng(11).uniform(0, 1, comp.shape)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def detail_neighbours(radius, k):
    _, tree, comp = detail_inputs()
    return neighbours(comp, tree, radius, k)
