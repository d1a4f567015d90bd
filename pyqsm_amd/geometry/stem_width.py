"""Stem width at a height above ground: what pyQSM's ``canopy_metrics.width_at_height`` measures, with
the percentiles of the pairwise distances taken on the GPU (``hip.pdist_select``).

    pairwise_distance_quantiles(points, q, seg_start)   np.percentile(pdist(points_s), q) per segment
    width_at_height(cloud, height, tolerance, ...)      one slab -> dict of widths
    width_profile(cloud, heights, ...)                  many slabs, one batched device call

pyQSM has no module of this name, so nothing is shadowed: ``canopy_metrics`` keeps resolving to
pyQSM's own file.

The pairwise distances are never stored: an order statistic of them is a radix selection over keys
recomputed from the points, and the percentile is numpy's rule applied on the host to the two order
statistics that bracket it. Every number equals ``np.percentile(scipy.spatial.distance.pdist(p), q)``
bit for bit.

Differences from the reference, all deliberate:

* ``height`` is honoured. The reference overwrites its argument with 2.8 on its first line, a leftover.
* Nothing is drawn, there is no ``input()`` and no ``breakpoint()``: ``width`` is the 95th percentile,
  what the reference returns when nobody types a number.
* The dict also carries what the reference only prints (``p90``, ``p95``, ``median``, ``max_width``),
  the farthest pair and the counts.
"""
from __future__ import annotations

import numpy as np

from .. import hip
from .cloud import PointCloud

MAX_QUANTILES_PER_CALL = hip.PDIST_MAX_RANKS // 2     # two order statistics per percentile


def percentile_ranks(m: int, q):
    """numpy's ``linear`` rule for ``np.percentile(d, q)`` on ``m`` sorted values: the ranks ``lo`` and
    ``hi`` of the two order statistics around the virtual index and the weight ``t`` of the upper one.
    ``q`` may be an array; ``m`` >= 1."""
    q = np.asarray(q, dtype=np.float64)
    if q.size and not ((q >= 0) & (q <= 100)).all():
        raise ValueError("percentiles must be in the range [0, 100]")
    v = (m - 1) * np.true_divide(q, 100)
    lo = np.floor(v)
    t = v - lo
    lo = lo.astype(np.int64)
    hi = np.minimum(lo + 1, m - 1)
    return lo, hi, t


def lerp(a, b, t):
    """numpy's ``_lerp``: ``a + (b - a) t``, ``b - (b - a) (1 - t)`` where t >= 0.5, ``a`` where t == 0."""
    a, b, t = (np.asarray(x, dtype=np.float64) for x in (a, b, t))
    diff = b - a
    out = np.asarray(a + diff * t)
    out = np.where(t >= 0.5, b - diff * (1 - t), out)
    return np.where(t == 0, a, out)


def median_of(a, b):
    """``np.median`` from the two middle order statistics (equal ranks for an odd count): their mean."""
    return (np.asarray(a, dtype=np.float64) + np.asarray(b, dtype=np.float64)) / 2.0


def middle_ranks(m: int):
    """The ranks ``np.median`` averages: (m - 1) // 2 and m // 2."""
    return (m - 1) // 2, m // 2


def _segments(n: int, seg_start) -> np.ndarray:
    seg = np.array([0, n], np.int64) if seg_start is None else np.asarray(seg_start, dtype=np.int64).reshape(-1)
    if seg.size < 1 or seg[0] != 0 or seg[-1] != n or (np.diff(seg) < 0).any():
        raise ValueError("seg_start must ascend from 0 to the number of points")
    return seg


def pairwise_distance_quantiles(points, q, seg_start=None, device=0):
    """``np.percentile(scipy.spatial.distance.pdist(points_s), q)`` for every segment ``s`` of ``points``
    [n, 2] or [n, 3], bit for bit, the distances never stored. ``q`` is a number or a sequence in
    [0, 100]; a segment with fewer than two points gives 0.0. Without ``seg_start`` the result has
    ``np.percentile``'s shape (a scalar or [n_q]); with it, one row per segment in front."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] not in (2, 3):
        raise ValueError(f"expected points of shape [n,2] or [n,3], got {pts.shape}")
    seg = _segments(pts.shape[0], seg_start)
    n_seg = len(seg) - 1
    qs = np.asarray(q, dtype=np.float64)
    flat = qs.reshape(-1)
    cnt = np.diff(seg)
    pairs = cnt * (cnt - 1) // 2
    out = np.zeros((n_seg, flat.size), np.float64)
    for c0 in range(0, flat.size, MAX_QUANTILES_PER_CALL):
        part = flat[c0:c0 + MAX_QUANTILES_PER_CALL]
        ranks = np.full((n_seg, 2 * part.size), -1, np.int64)
        weight = np.zeros((n_seg, part.size), np.float64)
        for s in range(n_seg):
            if pairs[s] > 0:
                lo, hi, t = percentile_ranks(int(pairs[s]), part)
                ranks[s, 0::2], ranks[s, 1::2], weight[s] = lo, hi, t
        res = hip.pdist_select(pts, seg, ranks, device=device)
        val = lerp(res.values[:, 0::2], res.values[:, 1::2], weight)
        out[:, c0:c0 + part.size] = np.where((pairs > 0)[:, None], val, 0.0)
    out = out.reshape((n_seg,) + qs.shape)
    if seg_start is None:
        return out[0] if qs.ndim else np.float64(out[0])
    return out


def _cloud_of(cloud):
    """(points float64 [n,3], seed or None) of an array, a PointCloud or the reference's file_content."""
    seed = None
    if isinstance(cloud, dict):
        seed = cloud.get('seed')
        cloud = cloud['clean_pcd']
    pts = np.asarray(cloud.points if hasattr(cloud, 'points') else cloud, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"expected points of shape [n,3], got {pts.shape}")
    return pts, seed


def plane_axes(axis: int):
    """The two axes the distances are taken in: those other than ``axis``, ascending."""
    if axis not in (0, 1, 2):
        raise ValueError(f"axis must be 0, 1 or 2, got {axis!r}")
    return [a for a in range(3) if a != axis]


def slab_indices(points, height, tolerance, axis=2) -> np.ndarray:
    """Indices of the points with ``ground + height - tolerance <= x[axis] <= ground + height +
    tolerance``, both ends included, ground = the minimum along ``axis`` (the reference's expressions)."""
    pts = np.asarray(points, dtype=np.float64)
    if len(pts) == 0:
        return np.zeros(0, np.int64)
    ground = np.min(pts[:, axis])
    z_min = ground + height - tolerance
    z_max = ground + height + tolerance
    return np.where((pts[:, axis] >= z_min) & (pts[:, axis] <= z_max))[0].astype(np.int64)


def _kept(pts, idx, nb_neighbors, std_ratio, device):
    if nb_neighbors is None or len(idx) == 0:
        return idx
    _, ind = PointCloud(pts[idx]).remove_statistical_outlier(nb_neighbors, std_ratio, device=device)
    return idx[np.asarray(ind, dtype=np.int64)]


def _measure(pts, kept, axis, device):
    """The widths of the slabs ``kept`` (index arrays into ``pts``): one batched selection of the seven
    order statistics per slab (two each for p90, p95 and the median, one for the maximum)."""
    h = len(kept)
    cnt = np.array([len(k) for k in kept], np.int64)
    seg = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    pairs = cnt * (cnt - 1) // 2
    plane = pts[np.concatenate(kept) if h else np.zeros(0, np.int64)][:, plane_axes(axis)]
    ranks = np.full((h, 7), -1, np.int64)
    weight = np.zeros((h, 2), np.float64)
    for s in range(h):
        if pairs[s] > 0:
            m = int(pairs[s])
            lo, hi, t = percentile_ranks(m, [90, 95])
            ranks[s] = [lo[0], hi[0], lo[1], hi[1], *middle_ranks(m), m - 1]
            weight[s] = t
    res = hip.pdist_select(plane, seg, ranks, device=device)
    has = pairs > 0
    v = res.values
    out = {
        'p90': np.where(has, lerp(v[:, 0], v[:, 1], weight[:, 0]), 0.0),
        'p95': np.where(has, lerp(v[:, 2], v[:, 3], weight[:, 1]), 0.0),
        'median': np.where(has, median_of(v[:, 4], v[:, 5]), 0.0),
        'max_width': np.where(has, v[:, 6], 0.0),
        'n_points': cnt,
        'n_pairs': pairs,
    }
    out['width'] = out['p95'].copy()
    far = np.full((h, 2), -1, np.int64)
    bounds = np.zeros((h, 3), np.float64)
    for s in range(h):
        if has[s]:
            far[s] = kept[s][res.max_pair[s]]
        if cnt[s]:
            bounds[s] = pts[kept[s]].max(axis=0) - pts[kept[s]].min(axis=0)
    out['max_pair'] = far
    out['bounds'] = bounds
    return out


def width_profile(cloud, heights, tolerance=0.1, axis=2, nb_neighbors=15, std_ratio=0.95, device=0):
    """:func:`width_at_height` at many heights: the slabs are cut on the host, outliers removed per
    slab, and all slabs measured in one batched device call. Returns a dict of arrays with one row
    per height: ``heights``, ``width``, ``bounds`` [h,3], ``p90``, ``p95``, ``median``, ``max_width``,
    ``max_pair`` [h,2], ``n_points``, ``n_pairs``. An empty slab gives zeros and ``n_points`` 0 (and a
    ``max_pair`` of (-1, -1), as does a slab of one point)."""
    pts, _ = _cloud_of(cloud)
    plane_axes(axis)
    hs = np.asarray(heights, dtype=np.float64).reshape(-1)
    kept = [_kept(pts, slab_indices(pts, float(hgt), tolerance, axis), nb_neighbors, std_ratio, device)
            for hgt in hs]
    out = _measure(pts, kept, axis, device)
    out['heights'] = hs
    return out


def width_at_height(cloud, height=1.37, tolerance=0.1, axis=2, nb_neighbors=15, std_ratio=0.95, seed=None,
                    device=0):
    """pyQSM's ``canopy_metrics.width_at_height``: the width of the cloud in the slab
    ``ground + height ± tolerance`` (closed on both sides, ground = the minimum along ``axis``).

    ``cloud`` is an [n,3] array, a ``PointCloud`` or the reference's ``file_content`` dict, of which
    ``clean_pcd`` and ``seed`` are used. The slab's statistical outliers are removed
    (``PointCloud.remove_statistical_outlier``; ``nb_neighbors=None`` skips it) and the pairwise
    distances of what is left are taken in the two axes other than ``axis`` (for axis 2 the reference's
    ``[:, :2]``). Returns a dict: ``seed``; ``width`` = ``p95``; ``bounds``, max - min of the kept 3-D
    points; ``p90``, ``p95``: ``np.percentile`` of the distances; ``median``: ``np.median``;
    ``max_width``; ``max_pair``: indices into the input cloud of the farthest pair, of equal distances
    the first, (-1, -1) without a pair; ``n_points`` kept; ``n_pairs``. Fewer than two kept points give
    widths of 0.0, as the reference's ``if len(dists) > 0 else 0.0``.

    The reference overwrites its ``height`` argument with 2.8 on its first line, a leftover; here the
    argument is honoured. Nothing is drawn and nothing is asked."""
    pts, dict_seed = _cloud_of(cloud)
    plane_axes(axis)
    kept = _kept(pts, slab_indices(pts, height, tolerance, axis), nb_neighbors, std_ratio, device)
    m = _measure(pts, [kept], axis, device)
    return {
        'seed': dict_seed if seed is None else seed,
        'width': float(m['width'][0]),
        'bounds': m['bounds'][0],
        'p90': float(m['p90'][0]),
        'p95': float(m['p95'][0]),
        'median': float(m['median'][0]),
        'max_width': float(m['max_width'][0]),
        'max_pair': (int(m['max_pair'][0, 0]), int(m['max_pair'][0, 1])),
        'n_points': int(m['n_points'][0]),
        'n_pairs': int(m['n_pairs'][0]),
    }
