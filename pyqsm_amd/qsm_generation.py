"""The RANSAC caller and the stem stage of ``pyQSM/qsm_generation.py``.

``fit_cyl_to_cluster`` (``qsm_generation.py:138-179``) is the function through which the
sphere-stepping QSM builder reaches ``fit_shape_RANSAC``; ``get_stem_pcd`` (``:71-120``) keeps the
points whose oriented normal is close to horizontal, on one device-resident call. The stepping
driver itself (``sphere_step``, file IO, drawing) is outside the hot-path scope.
"""
from __future__ import annotations

import logging

import numpy as np

try:  # flat import style of the reference (pyqsm_amd on sys.path) or package import
    from ._shadow import fall_through
    from . import hip
    from .geometry.cloud import PointCloud, as_points
    from .geometry.density import Components
    from .math_utils.fit import fit_shape_RANSAC
    from .math_utils.general import get_center
    from .set_config import config
except ImportError:  # pragma: no cover
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyqsm_amd._shadow import fall_through
    from pyqsm_amd import hip
    from pyqsm_amd.geometry.cloud import PointCloud, as_points
    from pyqsm_amd.geometry.density import Components
    from pyqsm_amd.math_utils.fit import fit_shape_RANSAC
    from pyqsm_amd.math_utils.general import get_center
    from pyqsm_amd.set_config import config

# names pyQSM's module of the same name defines and this one does not (pyqsm_amd/_shadow.py)
__getattr__ = fall_through(__name__)

log = logging.getLogger("calc")


def fit_cyl_to_cluster(main_pcd, curr_pts, last_radius, cluster_idxs, cyls=[], cyl_details=[],
                       debug=False, **ransac_kwargs):
    """qsm_generation.py:138-179: fit a circle to the z-projection of ``curr_pts`` (threshold
    0.04, points clamped up to the lowest z, radius at most ``last_radius *
    config['sphere']['radius_multiplier']``); the fit is good when a cylinder came back and its
    radius is below ``bad_fit_radius_factor * last_radius``. A good fit appends 500 points
    sampled on the cylinder to ``cyls`` and ``{center, axis, height, radius}`` to
    ``cyl_details`` (the caller's lists, mutated as in the reference). Returns the flag.
    ``debug`` drew and stopped in the debugger there; it is accepted and ignored.
    ``ransac_kwargs`` (``seed=``, ``samples=``) reach ``fit_shape_RANSAC``."""
    curr_pts = np.asarray(curr_pts)
    log.info("Attempting to fit a 2D circle to projection of points")
    prev_neighbor_height = np.min(curr_pts[:, 2])
    cyl_mesh, fit_pcd, inliers, fit_radius, axis = fit_shape_RANSAC(
        pts=curr_pts,
        shape="circle",
        threshold=0.04,
        lower_bound=prev_neighbor_height,
        max_radius=last_radius * config["sphere"]["radius_multiplier"],
        **ransac_kwargs,
    )
    good_fit_found = (cyl_mesh is not None
                      and fit_radius < config["sphere"]["bad_fit_radius_factor"] * last_radius)
    if good_fit_found:
        log.info("good fit found, adding cyl to list")
        cyls.append(cyl_mesh.sample_points_uniformly(500))
        cyl_details.append({"center": get_center(curr_pts), "axis": axis,
                            "height": prev_neighbor_height, "radius": fit_radius})
    return good_fit_found


def exclude_dense_areas(pcd, radius=.1, top=500, max_size=100, device: int = 0):
    """qsm_generation.py:526-556: the radius graph of the cloud at ``radius``, its connected
    components sorted by size, and of the ``top`` largest those with fewer than ``max_size`` points
    (``[x for x in conn_comps[0:500] if len(x) < 100]``, the selection the reference ends on).
    Returns ``(sub_cloud, components)``: the points of the selected components as a ``PointCloud``, in
    rank order, and the :class:`~pyqsm_amd.geometry.density.Components` of the whole cloud. The
    reference overrides its ``radius`` argument with ``.1``, which is the default here; it draws the
    line sets and then names undefined variables (``trim``, ``new_pts``): neither is reproduced. No
    pair list is built."""
    pts = as_points(pcd)
    comp, sizes, mem = hip.radius_components(pts, [float(radius)], device=device, members=True)
    comps = Components(comp[0], sizes[0], mem[0])
    return PointCloud(pts[comps.select(top=top, max_size=max_size)]), comps


_stem = config.get("stem", {})


def get_stem_pcd(pcd=None, source_file=None,
                 normals_radius=_stem.get("normals_radius", 0.1),
                 normals_nn=_stem.get("normals_nn", 30),
                 nb_neighbors=_stem.get("stem_neighbors", 10),
                 std_ratio=_stem.get("stem_ratio", 2),
                 angle_cutoff=_stem.get("angle_cutoff", 10),
                 voxel_size=_stem.get("stem_voxel_size", ""),
                 post_id_stat_down=_stem.get("post_id_stat_down", False),
                 orient_k: int = 100, device: int = 0):
    """qsm_generation.py:71-120 on ``hip.stem_cloud``: crop away z <= min z + 0.5 (skipped when that
    bound is exactly 0, as pyQSM's ``crop`` does), estimate normals with a hybrid search
    (``normals_radius``, ``normals_nn``), orient them over the ``orient_k`` = 100 nearest and keep
    the points ``filter_by_norm(angle_cutoff)`` keeps; all in HBM. Then, if ``voxel_size`` is
    truthy, ``voxel_down_sample``; if ``post_id_stat_down``, ``remove_statistical_outlier``
    (``nb_neighbors``, ``std_ratio``) on the stem cloud (the reference names an undefined
    ``test`` there; its evident intent). The reference's drawing and debugger block is dropped.
    Returns a ``PointCloud`` with the kept points and their oriented normals. Previous normals of
    ``pcd`` set the normals' sign, as Open3D's estimate_normals does."""
    if source_file:
        raise NotImplementedError("reading point cloud files is not part of this package: pass pcd")
    if pcd is None:
        raise ValueError("get_stem_pcd needs a cloud (pcd)")
    pts = as_points(pcd)
    prev = getattr(pcd, "normals", None)
    if prev is not None and (not hasattr(pcd, "has_normals") or not pcd.has_normals()):
        prev = None
    log.info("Estimating and orienting normals")
    idx, nrm = hip.stem_cloud(pts, normals_radius, normals_nn, orient_k, angle_cutoff,
                              crop_offset=0.5, normals=prev, device=device)
    stem_cloud = PointCloud(pts[idx], normals=nrm)
    log.info("cleaning result (if requested)")
    if voxel_size:
        stem_cloud = stem_cloud.voxel_down_sample(voxel_size=voxel_size, device=device)
    if post_id_stat_down:
        _, ind = stem_cloud.remove_statistical_outlier(nb_neighbors=nb_neighbors, std_ratio=std_ratio,
                                                       device=device)
        stem_cloud = stem_cloud.select_by_index(ind)
    return stem_cloud
