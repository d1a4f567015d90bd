"""The DBSCAN entry points of pyQSM/geometry/point_cloud_processing.py
(cluster_plus :169-203, cluster_and_get_largest :205-218) on the HIP kernels, and its
filter_by_norm (:246-256) on the normals they leave.

The reference calls Open3D's ``PointCloud.cluster_dbscan``; its result (noise -1,
clusters numbered in index order of their first core point, border points given
to the first cluster that reaches them) is the same labelling scikit-learn
produces, which is what the kernel is pinned against.
"""
from __future__ import annotations

import numpy as np

try:
    from .. import hip
    from .._shadow import fall_through
    from ..set_config import config, log
    from .cloud import PointCloud, TriangleMesh, as_points
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyqsm_amd import hip
    from pyqsm_amd._shadow import fall_through
    from pyqsm_amd.set_config import config, log
    from pyqsm_amd.geometry.cloud import PointCloud, TriangleMesh, as_points

# names pyQSM's module of the same name defines and this one does not (pyqsm_amd/_shadow.py)
__getattr__ = fall_through(__name__)


def _select(pcd, pts, idx):
    if hasattr(pcd, "select_by_index"):
        return pcd.select_by_index(idx)
    return PointCloud(pts[idx])


# what cluster_plus(ransac=True) seeds its plane hypotheses with (its signature is the reference's)
PLANE_SEED = None


def cluster_plus(pcd, eps=config["trunk"]["cluster_eps"], min_points=config["trunk"]["cluster_nn"],
                 draw_result=True, color_clusters=True, from_points=True, return_pcds=True,
                 ransac=False, device: int = 0, radius_inclusive: bool = True):
    """point_cloud_processing.py:169-203. ``from_points=True`` (the default) means
    ``pcd`` is an array of points. Returns the list of sub-clouds, one per label in
    ascending label order (noise -1 first when present), or ``{label: indices}``
    when ``return_pcds`` is false. ``draw_result`` / ``color_clusters`` are accepted
    and ignored (no GUI). ``ransac=True`` labels by plane segmentation instead of DBSCAN, as the
    reference's ``pcd.segment_plane(distance_threshold=eps, ransac_n=10, num_iterations=1000)`` means
    to (its branch ends in a NameError on ``labels``): label 0 for the inliers of the plane
    (``PointCloud.segment_plane``), -1 for the rest. The hypotheses are drawn from the module's
    ``PLANE_SEED``: None, the reference's unseeded behaviour, or an int for reproducible runs.
    ``radius_inclusive=False`` switches the neighbourhood to d < eps — Open3D's compare if
    nanoflann's radius search is strict (unverifiable here: parity unpinned, default inclusive)."""
    pts = as_points(pcd)
    if from_points:
        pcd = PointCloud(pts)
    if ransac:
        _, inliers = PointCloud(pts).segment_plane(distance_threshold=eps, ransac_n=10, num_iterations=1000,
                                                   seed=PLANE_SEED, device=device)
        labels = np.full(len(pts), -1, dtype=np.int32)
        labels[inliers] = 0
    else:
        labels, _ = hip.dbscan(pts, eps, min_points, device=device, radius_inclusive=radius_inclusive)
    unique_lbs, counts = np.unique(labels, return_counts=True)
    log.info(f"point cloud has {counts} clusters")
    label_to_cluster = {ulabel: np.where(labels == ulabel)[0] for ulabel in unique_lbs}
    if return_pcds:
        return [_select(pcd, pts, idx_list) for idx_list in label_to_cluster.values()]
    return label_to_cluster


def cluster_and_get_largest(pcd, eps=config["trunk"]["cluster_eps"],
                            min_points=config["trunk"]["cluster_nn"], draw_clusters=False,
                            device: int = 0, radius_inclusive: bool = True):
    """point_cloud_processing.py:205-218: the sub-cloud of the most populous label
    (noise counts as a label, as in the reference)."""
    pts = as_points(pcd)
    labels, _ = hip.dbscan(pts, eps, min_points, device=device, radius_inclusive=radius_inclusive)
    log.info(f"point cloud has {labels.max() + 1 if len(labels) else 0} clusters")
    if len(labels) == 0:
        return _select(pcd, pts, np.zeros(0, dtype=np.int64))
    unique_vals, counts = np.unique(labels, return_counts=True)
    largest = unique_vals[np.argmax(counts)]
    return _select(pcd, pts, np.where(labels == largest)[0])


def query_via_bnd_box(pcd, source_pcd, scale=1.1, translation=(0, 0, 1), draw=False, device: int = 0):
    """point_cloud_processing.py:306-343: neighbours of ``pcd`` in ``source_pcd``, found by moving
    and growing ``pcd``'s oriented bounding box. Returns ``(nbrs, new_nbr_idxs)``: the points of
    ``source_pcd`` inside the shifted, scaled box but not inside the box itself, as a cloud, and
    their indices into ``source_pcd``.

    The reference indexes ``pcd`` with these indices and calls ``source_pcd.points()``; the indices
    are into ``source_pcd``, so the neighbours are selected from ``source_pcd`` here. ``draw`` is
    accepted and ignored (no viewer). Both boxes are asked in one pass over the source cloud."""
    from copy import deepcopy
    from pyqsm_amd.geometry.hull import point_indices_within_boxes
    obb = (pcd if isinstance(pcd, PointCloud) else PointCloud(as_points(pcd))).get_oriented_bounding_box(device=device)
    shifted = deepcopy(obb).translate(translation, relative=True)
    shifted.scale(scale, center=obb.center)
    src = as_points(source_pcd)
    in_shifted, in_box = point_indices_within_boxes(src, [shifted, obb], device=device)
    new_nbr_idxs = np.setdiff1d(in_shifted, in_box)
    return _select(source_pcd, src, new_nbr_idxs), new_nbr_idxs


def _angles_deg(normals):
    """pyQSM's np.degrees(get_angles(n)) for every row: get_angles returns arctan(nz / sqrt(nx^2 +
    ny^2)) in radians whenever that is non-zero (its ``radians`` flag is overwritten), 0 when it is
    zero or nx = ny = 0; filter_by_norm then converts to degrees."""
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    a, b, c = n[:, 0], n[:, 1], n[:, 2]
    denom = np.sqrt(a**2 + b**2)
    with np.errstate(divide="ignore", invalid="ignore"):
        rad = np.arctan(c / np.sqrt(a**2 + b**2))
    rad = np.where(denom != 0, rad, 0.0)
    return np.degrees(rad)


def filter_by_norm(pcd, angle_thresh=10, rev=False):
    """point_cloud_processing.py:246-256: the sub-cloud of the points whose normal makes an angle
    strictly inside (-angle_thresh, angle_thresh) degrees with the XY plane (the complement with
    ``rev``). A normal with nx = ny = 0 has angle 0 and is kept. Needs ``pcd.normals``."""
    norms = np.asarray(pcd.normals)
    angles = _angles_deg(norms)
    log.info(f"{angle_thresh=}")
    if rev:
        stem_idxs = np.where((angles < -angle_thresh) | (angles > angle_thresh))[0]
    else:
        stem_idxs = np.where((angles > -angle_thresh) & (angles < angle_thresh))[0]
    return pcd.select_by_index(stem_idxs)


def get_ball_mesh(pcd, radii=[0.005, 0.01, 0.02, 0.04], device: int = 0):
    """point_cloud_processing.py:259-263: the ball-pivoted mesh of a cloud with oriented normals, by
    ``TriangleMesh.create_from_point_cloud_ball_pivoting`` of this package (exact on the snapped
    cloud, order-free; not Open3D's triangle list: DESIGN.md §19)."""
    return TriangleMesh.create_from_point_cloud_ball_pivoting(pcd, radii, device=device)
