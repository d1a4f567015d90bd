"""NumPy/SciPy restatement of the cloud-cleaning contract (include/pyqsm_hip.h, "cloud cleaning").

Open3D's PointCloud.voxel_down_sample and remove_statistical_outlier, recollected from Open3D,
parity unpinned: this file is what defines them for the kernels of pyqsm_amd/csrc/clean.hip.

* Voxel means are accumulated with ``np.add.at`` into zeros, which adds one member at a time in
  ascending index order (``np.sum`` sums pairwise, ``np.add.reduceat`` in no promised order).
* The outlier step takes its neighbours from ``cKDTree.query``, recomputes
  ``d2 = ((dx*dx) + dy*dy) + dz*dz`` in fp64, sorts every row, takes ``sqrt`` and sums column by
  column: the same sequence of roundings the kernel performs.
"""
from __future__ import annotations

import numpy as np

LIMIT_CELLS = 2 ** 62


class VoxelRangeError(ValueError):
    """The voxel grid over the cloud would have more than 2^62 cells."""


def voxel_down_sample(P, voxel_size, C=None):
    """(means [m,3], colour means [m,3] or None, inverse [n], offsets [m+1], members [n])."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = len(P)
    if not (np.isfinite(voxel_size) and voxel_size > 0):
        raise ValueError("voxel_size must be positive and finite")
    if n == 0:
        z = np.zeros((0, 3))
        e = np.zeros(0, dtype=np.int64)
        return z, (None if C is None else z.copy()), e, np.zeros(1, dtype=np.int64), e.copy()
    vmin = P.min(axis=0) - voxel_size * 0.5
    key3 = np.floor((P - vmin) / voxel_size)
    top = key3.max(axis=0)
    if not np.all(top < 2.0 ** 62):
        raise VoxelRangeError("voxel_size too small for this cloud")
    dims = [int(t) + 1 for t in top]
    if dims[0] * dims[1] > LIMIT_CELLS or dims[0] * dims[1] * dims[2] > LIMIT_CELLS:
        raise VoxelRangeError("voxel_size too small for this cloud")
    k = key3.astype(np.int64)
    key = k[:, 0] + np.int64(dims[0]) * (k[:, 1] + np.int64(dims[1]) * k[:, 2])
    _, first, inv_u = np.unique(key, return_index=True, return_inverse=True)
    inv_u = inv_u.reshape(-1)
    m = len(first)
    row_of_u = np.empty(m, dtype=np.int64)
    row_of_u[np.argsort(first, kind="stable")] = np.arange(m)
    inverse = row_of_u[inv_u]
    counts = np.bincount(inverse, minlength=m)
    sums = np.zeros((m, 3))
    np.add.at(sums, inverse, P)
    means = sums / counts[:, None].astype(np.float64)
    cmeans = None
    if C is not None:
        cs = np.zeros((m, 3))
        np.add.at(cs, inverse, np.asarray(C, dtype=np.float64).reshape(-1, 3))
        cmeans = cs / counts[:, None].astype(np.float64)
    offsets = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    members = np.argsort(inverse, kind="stable").astype(np.int64)
    return means, cmeans, inverse.astype(np.int64), offsets, members


def knn_d2(P, k, workers=1):
    """Squared distances [n,k] to the k nearest points (the point itself included), ascending,
    recomputed in fp64 as ((dx*dx) + dy*dy) + dz*dz from cKDTree's indices."""
    from scipy.spatial import cKDTree
    P = np.asarray(P, dtype=np.float64)
    n = len(P)
    _, idx = cKDTree(P).query(P, k, workers=workers)
    idx = np.asarray(idx).reshape(n, k)
    d2 = np.empty((n, k))
    for j in range(k):
        q = P[idx[:, j]]
        dx, dy, dz = q[:, 0] - P[:, 0], q[:, 1] - P[:, 1], q[:, 2] - P[:, 2]
        d2[:, j] = ((dx * dx) + dy * dy) + dz * dz
    d2.sort(axis=1)
    return d2


def stat_avg(P, nb_neighbors, workers=1):
    """Mean distance of every point to its min(nb_neighbors, n) nearest points: sqrt of each d2,
    summed column by column from 0.0, divided by k."""
    n = len(P)
    k = min(int(nb_neighbors), n)
    s = np.sqrt(knn_d2(P, k, workers))
    acc = np.zeros(n)
    for j in range(k):
        acc = acc + s[:, j]
    return acc / float(k)


def stat_threshold(avg):
    """(mean, std) of Open3D's statistics, the threshold being mean + std_ratio * std: mean = the
    positive averages' sum over EVERY point, std from the squared deviations of the positive
    averages only, divisor n - 1."""
    n = len(avg)
    pos = avg[avg > 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = float(np.sum(pos)) / n
        sq = float(np.sum((pos - mean) ** 2))
        std = float(np.sqrt(sq / (n - 1))) if n > 1 else float("nan")
    return mean, std


def stat_outlier(P, nb_neighbors, std_ratio, workers=1):
    """(kept indices ascending, avg, mean, std, thr)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    if int(nb_neighbors) < 1 or not std_ratio > 0:
        raise ValueError("nb_neighbors >= 1 and std_ratio > 0")
    if len(P) == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0), float("nan"), float("nan"), float("nan")
    avg = stat_avg(P, nb_neighbors, workers)
    mean, std = stat_threshold(avg)
    thr = mean + std_ratio * std
    keep = np.nonzero((avg > 0) & (avg < thr))[0].astype(np.int64)
    return keep, avg, mean, std, thr


def clean_cloud(P, voxels, neighbors, ratio, iters, workers=1):
    """pyQSM/geometry/point_cloud_processing.py:97-127 on the restated operations."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    run_stat = all([neighbors, ratio, iters])
    cur = voxel_down_sample(P, voxels)[0] if voxels else P
    if not run_stat:
        return P
    for _ in range(iters):
        keep = stat_outlier(cur, int(neighbors), ratio, workers)[0]
        cur = cur[keep]
        neighbors = neighbors * 2
        ratio = ratio / 1.5
    return cur
