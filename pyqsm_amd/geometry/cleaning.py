"""Cloud cleaning on the HIP kernels: pyQSM's ``clean_cloud`` (pyQSM/geometry/
point_cloud_processing.py:97-127) device-resident, and functional forms of the two Open3D
operations it applies, ``voxel_down_sample`` and ``remove_statistical_outlier``.

The semantics are recollected from Open3D, parity unpinned (Open3D is not a dependency of this
package); tests/clean_restatement.py states them in NumPy and is what the kernels are held to.
pyQSM has no module of this name, so nothing is shadowed: pyQSM's own ``clean_cloud`` still
resolves through the fall-through of ``geometry.point_cloud_processing`` and runs on the
``PointCloud`` methods of ``geometry/cloud.py``.
"""
from __future__ import annotations

import numpy as np

try:
    from .. import hip
    from ..set_config import config, log
    from .cloud import PointCloud, as_points
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyqsm_amd import hip
    from pyqsm_amd.set_config import config, log
    from pyqsm_amd.geometry.cloud import PointCloud, as_points

_clean = config.get("initial_clean", {})


def voxel_down_sample(points, voxel_size: float, colors=None, return_trace: bool = False,
                      device: int = 0):
    """Mean of every occupied voxel of edge ``voxel_size``: float64 [m,3], rows ordered by the
    smallest input index of each voxel (Open3D's order is a hash map's, unspecified). With
    ``colors`` [n,3] returns ``(points, colours)``; with ``return_trace`` additionally
    ``(inverse [n], offsets [m+1], members [n])``: the row of every input point and the members
    of every row, ascending."""
    xyz, rgb, *trace = hip.voxel_down_sample(as_points(points), voxel_size, colors=colors,
                                             return_trace=return_trace, device=device)
    out = xyz if colors is None else (xyz, rgb)
    if return_trace:
        return (out, trace[0]) if colors is None else (xyz, rgb, trace[0])
    return out


def remove_statistical_outlier(points, nb_neighbors: int, std_ratio: float, device: int = 0):
    """Indices (int64, ascending) of the points whose mean distance to their ``nb_neighbors``
    nearest points (the point itself among them) is positive and below mean + std_ratio * std
    of those means over the cloud."""
    return hip.stat_outlier(as_points(points), nb_neighbors, std_ratio, device=device)


def clean_cloud(pcd,
                voxels=_clean.get("voxel_size", 0.04),
                neighbors=_clean.get("neighbors", 2),
                ratio=_clean.get("ratio", 4),
                iters=_clean.get("iters", 3),
                device: int = 0):
    """point_cloud_processing.py:97-127 in one device-resident call (``hip.clean_cloud``): the voxel
    step if ``voxels`` is truthy, then, if ``neighbors``, ``ratio`` and ``iters`` are all truthy,
    ``iters`` rounds of statistical outlier removal with ``int(neighbors)`` neighbours, doubling
    ``neighbors`` and dividing ``ratio`` by 1.5 after each round. Accepts an array or anything with
    ``.points``; returns a ``PointCloud``.

    Kept from the reference: when the statistical step is off, the INPUT cloud is returned, not
    the down-sampled one (so ``voxels`` alone changes nothing)."""
    run_voxels = bool(voxels)
    run_stat = all([neighbors, ratio, iters])
    pts = as_points(pcd)
    if not run_stat:
        if not run_voxels:
            log.warning("No cleaning steps were run")
        return pcd if isinstance(pcd, PointCloud) else PointCloud(pts)
    out = hip.clean_cloud(pts, float(voxels) if run_voxels else 0.0, neighbors, ratio, int(iters),
                          device=device)
    return PointCloud(out)


def split_ground(pcd, distance_threshold=0.1, max_slope_deg=30, ransac_n=3, num_iterations=1000,
                 probability=0.99999999, seed=None, draws=None, device: int = 0):
    """The ground as one plane: ``(ground, rest, plane)``, the sub-clouds of the points within
    ``distance_threshold`` of the best plane whose normal lies within ``max_slope_deg`` of +z, of all
    the others, and the refitted plane ``(a, b, c, d)`` with c > 0 (``PointCloud.segment_planes`` with
    one plane and the cone about +z). On sloping ground this takes a slab where a cut by z
    percentiles takes a wedge. No plane inside the cone: an empty ground and a zero plane."""
    pts = as_points(pcd)
    cloud = pcd if isinstance(pcd, PointCloud) else PointCloud(pts)
    seg = cloud.segment_planes(distance_threshold, max_planes=1, min_inliers=1, ransac_n=ransac_n,
                               num_iterations=num_iterations, probability=probability, axis=(0.0, 0.0, 1.0),
                               max_angle_deg=max_slope_deg, seed=seed, draws=draws, device=device)
    plane = seg.planes[0] if len(seg) else np.zeros(4)
    return cloud.select_by_index(seg.indices(0)), cloud.select_by_index(seg.rest()), plane
