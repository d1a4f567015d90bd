"""The neighbour-recovery helpers of pyQSM/geometry/reconstruction.py on the HIP kernels:
``get_neighbors_kdtree`` (:233-263) on the radius kernel, ``overlap_voxel_grid`` and
``get_nbrs_voxel_grid`` (:266-355) on the device voxel grid, and the feature transfer of
pyQSM/canopy_metrics.py:236-252 (``expand_features_to_orig``) on the fused neighbour reduction."""
from __future__ import annotations

import logging
import os
from collections import defaultdict
from glob import glob

import numpy as np

try:
    from .. import hip
    from .._shadow import fall_through
    from .cloud import PointCloud, VoxelGrid, as_points
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyqsm_amd import hip
    from pyqsm_amd._shadow import fall_through
    from pyqsm_amd.geometry.cloud import PointCloud, VoxelGrid, as_points

# names pyQSM's module of the same name defines and this one does not (pyqsm_amd/_shadow.py)
__getattr__ = fall_through(__name__)

log = logging.getLogger("calc")


def get_neighbors_kdtree(src_pcd, query_pcd=None, query_pts=None, kd_tree=None, dist=0.05, k=500,
                         return_pcd=True, device: int = 0):
    """reconstruction.py:233-263: the points of ``src_pcd`` that are among the ``k``
    nearest neighbours within ``dist`` (strict, like SciPy's ``distance_upper_bound``)
    of some query point.

    ``return_pcd=True`` (the default) returns ``(pcd, counts, chained_nbrs)``: the
    sub-cloud, the number of neighbours each query selected (the reference returns the
    padded [m,k] index table here; its callers only use the other two values) and the
    ascending unique source indices; ``(None, None, None)`` when nothing is in range.
    ``return_pcd=False`` returns ``(dists, nbrs)``, the padded [m,k] tables of
    ``KDTree.query`` (missing entries: distance inf, index n), as canopy_metrics.py:238
    uses them. ``kd_tree`` is accepted and ignored."""
    if query_pcd is not None:
        query_pts = as_points(query_pcd)
    src_pts = as_points(src_pcd)
    if not return_pcd:
        return hip.radius_knn(src_pts, as_points(query_pts), dist, k=k, device=device)
    mask, counts = hip.radius_mark(src_pts, as_points(query_pts), dist, k=k, device=device)
    uniques = np.flatnonzero(mask)
    if len(uniques) == 0:
        return None, None, None
    pcd = (src_pcd.select_by_index(uniques) if hasattr(src_pcd, "select_by_index")
           else PointCloud(src_pts[uniques]))
    return pcd, counts, uniques


def _device_grid(grid):
    return grid.device_grid if hasattr(grid, "device_grid") else grid


def overlap_voxel_grid(src_pts, comp_voxel_grid=None, source_pcd=None, invert=False, device: int = 0):
    """reconstruction.py:266-284: the indices of ``src_pts`` that lie in an occupied voxel of
    ``comp_voxel_grid`` (default: the grid of ``source_pcd`` at voxel size 0.2, ``:268``), as an
    ascending int64 array, empty when there are none.

    Deviation: with ``invert=True`` this returns the complement, the points in no occupied voxel.
    The reference computes it and then overwrites it with the included indices on its line 282, so
    its ``invert`` has no effect; the complement is what tree_isolation.py:471-474 builds by hand."""
    if comp_voxel_grid is None:
        if source_pcd is None:
            raise ValueError("overlap_voxel_grid needs comp_voxel_grid or source_pcd")
        comp_voxel_grid = VoxelGrid.create_from_point_cloud(source_pcd, voxel_size=0.2, device=device)
    log.info("querying voxel grid")
    pts = as_points(src_pts)
    _, uniques = _device_grid(comp_voxel_grid).query(pts, indices=True, invert=invert)
    log.info(f"{len(uniques) if not invert else len(pts) - len(uniques)} points in occupied voxels")
    return uniques


def get_nbrs_voxel_grid(comp_pcd, comp_file_name, tile_dir, tile_pattern, invert=False, out_folder="detail",
                        out_file_prefix="detail_feats", device: int = 0):
    """reconstruction.py:286-355: every ``.npz`` tile matching ``tile_dir/tile_pattern`` whose
    bounding box meets that of ``comp_pcd`` is checked against the voxel grid of ``comp_pcd`` (voxel
    size 0.1). One grid is created once and every tile is streamed through it. Per tile the indices
    go to ``tile_dir/color_int_tree_nbrs/<tile>/<out_file_prefix>_<comp_file_name>.npz`` (``nbrs``);
    the tiles' arrays filtered to those indices are joined, written to
    ``out_folder/<comp_file_name>.npz`` and returned. A ``.pcd`` tile raises: there is no reader for
    it here (the reference reads it with Open3D). Tiles are visited in sorted order."""
    comp_pts = as_points(comp_pcd)
    log.info("creating voxel grid")
    grid = VoxelGrid.create_from_point_cloud(comp_pcd, voxel_size=0.1, device=device)
    log.info("voxel grid created")
    comp_min, comp_max = comp_pts.min(axis=0), comp_pts.max(axis=0)
    all_data = defaultdict(list)
    for file in sorted(glob(f"{tile_dir}/{tile_pattern}")):
        if file.endswith(".pcd"):
            raise ValueError(f"{file}: .pcd tiles cannot be read here (no Open3D reader); convert them to .npz")
        file_name = os.path.basename(file).replace(".npz", "")
        log.info(f"processing {file_name}")
        data = np.load(file)
        points = np.asarray(data["points"], dtype=np.float64)
        intersect = len(points) > 0 and np.all((points.max(axis=0) >= comp_min) & (comp_max >= points.min(axis=0)))
        if not intersect:
            log.info("Bounding boxes do not intersect, skipping file.")
            continue
        uniques = overlap_voxel_grid(points, grid, invert=invert)
        nbr_dir = f"{tile_dir}/color_int_tree_nbrs/{file_name}"
        os.makedirs(nbr_dir, exist_ok=True)
        np.savez_compressed(f"{nbr_dir}/{out_file_prefix}_{comp_file_name}.npz", nbrs=uniques)
        for name in data.files:
            all_data[name].append(data[name][uniques])
    grid.device_grid.close()
    for name, parts in all_data.items():
        all_data[name] = np.hstack(parts) if parts[0].ndim == 1 else np.vstack(parts)
    os.makedirs(out_folder, exist_ok=True)
    np.savez_compressed(f"{out_folder}/{comp_file_name}.npz", **all_data)
    return all_data


def transfer_features(src_pts, values, query_pts, dist=0.05, k=500, reducer="mean", empty_row=0,
                      device: int = 0):
    """``values`` ([n] or [n, F]) of the source points carried to ``query_pts``: ``reducer`` (mean,
    min, max, first) over each query's (up to ``k`` nearest) source points within ``dist`` (strict),
    reduced on the GPU (``hip.radius_reduce``). A query with nothing in range gets
    ``values[empty_row]``; NaN with ``empty_row=-1``. float64 [m] or [m, F]."""
    return hip.radius_reduce(as_points(src_pts), as_points(query_pts), values, dist, k=k, reducer=reducer,
                             empty_row=empty_row, device=device)


def expand_features_to_orig(nbr_pcd, orig_pcd, nbr_data, device: int = 0):
    """pyQSM/canopy_metrics.py:236-252: the features of ``nbr_data`` (every key but ``points``,
    ``colors`` and ``labels``, one value per point of ``nbr_pcd``) averaged over the neighbours of
    every point of ``orig_pcd`` in ``nbr_pcd`` (dist 0.05, k 500); a point with no neighbour takes
    row 0, as the reference does. Returns ``{'points': orig points, 'features': f64 [m, F]}``.

    Deviation: the reference drops the padding of the neighbour table with ``x < len(orig_pcd.points)``
    where the padding value is the length of the source, ``nbr_pcd``; the intent (drop the padding,
    keep every real neighbour) is what is implemented."""
    feat_names = [name for name in nbr_data.keys() if name not in ("points", "colors", "labels")]
    src, qry = as_points(nbr_pcd), as_points(orig_pcd)
    out = {"points": getattr(orig_pcd, "points", qry)}
    if not feat_names:
        out["features"] = np.zeros((len(qry), 0))
        return out
    vals = np.stack([np.asarray(nbr_data[name], dtype=np.float64).reshape(len(src)) for name in feat_names], axis=1)
    feats = [transfer_features(src, vals[:, f0:f0 + hip.RADIUS_REDUCE_MAX_F], qry, device=device)
             for f0 in range(0, vals.shape[1], hip.RADIUS_REDUCE_MAX_F)]
    out["features"] = np.concatenate(feats, axis=1)
    return out
