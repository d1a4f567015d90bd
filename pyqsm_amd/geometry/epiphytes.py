"""Epiphyte isolation on the GPU: what pyQSM's ``canopy_metrics.identify_epiphytes`` computes between
the contraction's first shift and the projected areas.

    split_on_percentile(pcd, val_list, pctile, comp)   viz.color.split_on_percentile (viz/color.py:348-363)
    split_on_pct(pcd, pct, cmag=None, shift=None)      canopy_metrics.split_on_pct (:228-234)
    shift_components(shift, mag_pct=65, z_pct=60)      both splits of identify_epiphytes in one device call
    identify_epiphytes(file_content, ...)              canopy_metrics.identify_epiphytes (:60-84)
    project_components_in_clusters(...)                canopy_metrics.project_components_in_clusters (:370-423)
    area_indices(metrics, pca)                         EAI, LAI and proposed LAI of data/notes/methods.md

pyQSM has no module of this name, so nothing is shadowed: ``canopy_metrics`` keeps resolving to pyQSM's
own file (tests/test_dropin.py; INTEGRATION.md has the one-line edits), and ``viz.color`` of this package
(the colour path) re-exports ``split_on_percentile`` from here.

The percentiles are exact: an order statistic is a radix selection on the device over keys recomputed
from the rows (``hip.select_values``), and the percentile is NumPy's linear rule applied on the host
to the two order statistics around it (``stem_width.percentile_ranks`` / ``lerp``): every threshold
equals ``np.percentile`` of the same values. The clumps are ``math_utils.clustering.kmeans_pp``.

Differences from the reference, all deliberate:

* Nothing is drawn or coloured (``color_on_percentile`` is accepted and ignored), no GUI, no pickle,
  no file. ``identify_epiphytes`` returns what the reference computes and drops.
* The shift magnitude is ``sqrt(((x*x) + (y*y)) + (z*z))``; ``np.linalg.norm`` of a row may differ in
  the last bit, which moves a row across the percentile only on an exact near-tie.
* k-means: see ``kmeans_pp`` (direct distances, fixed summation order, empty centres stay). A
  component with fewer voxels than ``n_clusters`` gets one cluster per voxel (scikit-learn raises).
"""
from __future__ import annotations

import operator
from collections import defaultdict

import numpy as np

from .. import hip
from ..math_utils.clustering import kmeans_pp
from ..viz.projection import project_by_label
from .cloud import PointCloud, as_points
from .stem_width import lerp, percentile_ranks

DEVICE_COMPARISONS = {operator.gt: "gt", operator.ge: "ge", operator.lt: "lt", operator.le: "le"}


def _subset(pcd, pts, idx, invert=False) -> PointCloud:
    """The rows ``idx`` of a cloud (or the others), colours and normals kept when it has them."""
    if invert:
        mask = np.ones(len(pts), dtype=bool)
        mask[idx] = False
        idx = np.nonzero(mask)[0]
    out = PointCloud(pts[idx])
    for name in ("colors", "normals"):
        a = getattr(pcd, name, None)
        if a is not None and len(np.asarray(a)) == len(pts):
            setattr(out, name, np.asarray(a)[idx])
    return out


def percentile_dev(v_ptr: int, n: int, width: int, q, key=0, device: int = 0) -> float:
    """``np.percentile(keys, q)`` of ``n`` device-resident rows: two selected order statistics, NumPy's
    interpolation on the host."""
    lo, hi, t = percentile_ranks(int(n), q)
    a, b = hip.select_values_dev(v_ptr, n, width, [int(lo), int(hi)], key=key, device=device)
    return float(lerp(a, b, t))


def split_on_percentile(pcd, val_list, pctile, comp=operator.gt, color_on_percentile=False, device: int = 0):
    """pyQSM's ``viz.color.split_on_percentile``: ``(indices, cloud of the rows with
    comp(value, np.percentile(values, pctile)), cloud of the others)``. The percentile is always taken
    on the device; ``comp`` among ``operator.gt / ge / lt / le`` also partitions there
    (``hip.split_above_dev``), any other callable is applied on the host to the values and the
    device's percentile, as the reference applies it. ``color_on_percentile`` is accepted and ignored."""
    pts = as_points(pcd)
    vals = np.ascontiguousarray(np.asarray(val_list, dtype=np.float64).reshape(-1))
    n = len(vals)
    if len(pts) != n:
        raise ValueError("length of val list does not match size of pcd")
    if n == 0:
        return np.zeros(0, np.int64), PointCloud(pts), PointCloud(pts)
    d_vals = hip.DeviceBuffer.from_array(vals, device)
    try:
        val = percentile_dev(d_vals.ptr, n, 1, pctile, device=device)
        cmp = DEVICE_COMPARISONS.get(comp)
        if cmp is None:
            idx = np.where(comp(vals, val))[0].astype(np.int64)
        else:
            d_idx = hip.DeviceBuffer(8 * n, device)
            try:
                cnt = hip.split_above_dev(d_vals.ptr, n, 1, val, cmp=cmp, idx_ptr=d_idx.ptr, device=device)
                idx = d_idx.download((n,), np.int64)[:cnt].copy()
            finally:
                d_idx.free()
    finally:
        d_vals.free()
    return idx, _subset(pcd, pts, idx), _subset(pcd, pts, idx, invert=True)


def split_on_pct(pcd, pct, cmag=None, shift=None, device: int = 0):
    """pyQSM's ``canopy_metrics.split_on_pct``: ``(low cloud, high cloud)`` around the ``pct``-th
    percentile of ``cmag``, or of the row norms of ``shift`` [n,3] when given (taken on the device)."""
    pts = as_points(pcd)
    if shift is not None:
        s = np.ascontiguousarray(np.asarray(shift, dtype=np.float64).reshape(-1, 3))
        if len(s) != len(pts):
            raise ValueError("one shift vector per point")
        if len(s) == 0:
            return PointCloud(pts), PointCloud(pts)
        d_s = hip.DeviceBuffer.from_array(s, device)
        d_idx = hip.DeviceBuffer(8 * len(s), device)
        try:
            val = percentile_dev(d_s.ptr, len(s), 3, pct, key="norm", device=device)
            cnt = hip.split_above_dev(d_s.ptr, len(s), 3, val, key="norm", idx_ptr=d_idx.ptr, device=device)
            idx = d_idx.download((len(s),), np.int64)[:cnt].copy()
        finally:
            d_s.free()
            d_idx.free()
    else:
        idx = split_on_percentile(pcd, cmag, pct, device=device)[0]
    return _subset(pcd, pts, idx, invert=True), _subset(pcd, pts, idx)


def shift_components(shift, mag_pct=65, z_pct=60, device: int = 0):
    """The two splits of ``identify_epiphytes`` in one device call (``hip.shift_components``):
    ``(labels uint8 [n], thresholds [2], counts [3])`` with 0 = shift magnitude not above its
    ``mag_pct``-th percentile (wood), 1 = leaf (of the others, z-shift above their ``z_pct``-th
    percentile), 2 = epiphyte (the rest)."""
    res = hip.shift_components(shift, mag_pct, z_pct, device=device)
    return res.labels, res.thresholds, res.counts


def project_components_in_clusters(in_pcd, clean_pcd, epis, leaves, wood, seed, name='', off_screen=True,
                                   voxel_size=25, eps=120, min_points=30, target_dir='data/projection',
                                   n_clusters=20, every=4, alpha=50, include_epis=False, device: int = 0):
    """pyQSM's ``canopy_metrics.project_components_in_clusters``: per component (leaves, wood; with
    ``include_epis`` also the epiphytes, which the reference has commented out) ``voxel_down_sample``,
    ``n_clusters`` k-means clumps (``kmeans_pp(..., seed=0)``), every ``every``-th point of each clump,
    and the summed projected alpha-shape area of the clumps (``project_by_label``). Returns
    ``{seed: {'leaf_clusters': area, 'wood_clusters': area}}`` as the reference builds it. ``in_pcd``,
    ``clean_pcd``, ``name``, ``off_screen``, ``eps``, ``min_points`` and ``target_dir`` are accepted and
    ignored, as they are unused there; no pickle is written."""
    metrics = defaultdict(dict)
    cases = [(leaves, 'leaf_clusters'), (wood, 'wood_clusters')]
    if include_epis:
        cases.insert(0, (epis, 'epi_clusters'))
    for case_pcd, case_name in cases:
        pts = as_points(case_pcd)
        total_area = 0.0
        if len(pts):
            pts = hip.voxel_down_sample(pts, voxel_size, device=device)[0]
            fit = kmeans_pp(pts, min(int(n_clusters), len(pts)), seed=0, device=device)
            total_area = project_by_label(pts, fit.labels_, alpha, every=every)['total_area']
        metrics[case_name] = total_area
    return {seed: metrics}


def identify_epiphytes(file_content, save_gif=False, out_path=None, mag_pct=65, z_pct=60, voxel_size=25,
                       n_clusters=20, every=4, alpha=50, include_epis=True, device: int = 0):
    """pyQSM's ``canopy_metrics.identify_epiphytes`` on the reference's ``file_content`` (keys ``seed``,
    ``src``, ``clean_pcd``, ``shift_one``: the first contraction step's shift of every point of
    ``clean_pcd``, ``extract_skeleton(..., debug=True)[2][0]``). Returns a dict: ``wood``, ``leaves``,
    ``epis`` (clouds), ``labels`` (0 / 1 / 2 in that order), ``thresholds``, ``counts`` and ``metrics``
    (:func:`project_components_in_clusters`, by default with the epiphytes' own area, which
    :func:`area_indices` needs). ``save_gif`` and ``out_path`` are accepted and ignored."""
    seed, pcd, clean_pcd, shift_one = (file_content['seed'], file_content['src'], file_content['clean_pcd'],
                                       file_content['shift_one'])
    if shift_one is None:
        raise ValueError("no shifts for this seed: pass the first contraction step's shift as 'shift_one'")
    pts = as_points(clean_pcd)
    shift = np.asarray(shift_one, dtype=np.float64).reshape(-1, 3)
    if len(shift) != len(pts):
        raise ValueError("one shift vector per point of clean_pcd")
    labels, thresholds, counts = shift_components(shift, mag_pct, z_pct, device=device)
    wood, leaves, epis = (_subset(clean_pcd, pts, np.nonzero(labels == v)[0]) for v in (0, 1, 2))
    metrics = project_components_in_clusters(pcd, clean_pcd, epis, leaves, wood, seed, voxel_size=voxel_size,
                                             n_clusters=n_clusters, every=every, alpha=alpha,
                                             include_epis=include_epis, device=device)
    return {'seed': seed, 'wood': wood, 'leaves': leaves, 'epis': epis, 'labels': labels,
            'thresholds': thresholds, 'counts': counts, 'metrics': metrics}


def area_indices(metrics, pca):
    """The indices of data/notes/methods.md from component areas and the projected canopy area
    ``pca``: ``{'EAI': epiphyte / pca, 'LAI': (wood + leaf + epiphyte) / pca, 'LAI_proposed':
    (wood + leaf) / pca}``. ``metrics`` is ``{'leaf_clusters', 'wood_clusters', 'epi_clusters'}`` or the
    ``{seed: {...}}`` that :func:`project_components_in_clusters` returns for one seed."""
    if 'wood_clusters' not in metrics and len(metrics) == 1:
        metrics = next(iter(metrics.values()))
    missing = [k for k in ('leaf_clusters', 'wood_clusters', 'epi_clusters') if k not in metrics]
    if missing:
        raise ValueError(f"metrics lack {missing} (project_components_in_clusters(..., include_epis=True))")
    pca = float(pca)
    if not pca > 0:
        raise ValueError("the projected canopy area must be positive")
    wood, leaf, epi = (float(metrics[k]) for k in ('wood_clusters', 'leaf_clusters', 'epi_clusters'))
    return {'EAI': epi / pca, 'LAI': ((wood + leaf) + epi) / pca, 'LAI_proposed': (wood + leaf) / pca}
