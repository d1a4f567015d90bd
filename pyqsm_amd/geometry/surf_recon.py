"""pyQSM's ``geometry/surf_recon.py`` ``pivot_ball_mesh`` on the HIP kernels: nearest-neighbour
distances, normals, their orientation and the ball-pivoted mesh all run on the GPU.

The mesh follows this package's order-free contract: exact for the cloud snapped to a
lattice, the same bits on every run, and not Open3D's triangle list. ``meshfix`` closes its holes on the
GPU too (minimum-area patches, not MeshFix's). Nothing is drawn here; pyQSM's other
reconstructions (``map_density``, the alpha shape of ``get_mesh``) are out of scope and, with pyQSM
behind this package on ``sys.path``, still resolve to pyQSM's own file.
"""
from __future__ import annotations

import numpy as np

try:
    from .._shadow import fall_through
    from ..set_config import log
    from .cloud import KDTreeSearchParamHybrid, PointCloud, TriangleMesh, as_points
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyqsm_amd._shadow import fall_through
    from pyqsm_amd.set_config import log
    from pyqsm_amd.geometry.cloud import KDTreeSearchParamHybrid, PointCloud, TriangleMesh, as_points

# names pyQSM's module of the same name defines and this one does not (pyqsm_amd/_shadow.py)
__getattr__ = fall_through(__name__)


def pivot_ball_mesh(pcd, radii_factors=[0.1, 0.2, 0.3, 0.4, 0.5, 0.7, 1, 1.2, 1.5, 1.7, 2],
                    plot_distribution=False, device: int = 0):
    """surf_recon.py:87-116: radii = ``radii_factors`` times the mean nearest-neighbour distance,
    normals from the 20 nearest within three such distances, oriented along the tangent-plane graph
    (k = 100), then the ball-pivoted mesh with vertex normals. ``pcd``: a ``PointCloud`` of this
    package (an array or anything with ``.points`` is wrapped); its normals are replaced, as in
    pyQSM. ``plot_distribution`` is accepted and ignored: nothing is drawn."""
    if not isinstance(pcd, PointCloud):
        pcd = PointCloud(as_points(pcd))
    log.info("Computing KNN distance")
    avg_dist = float(np.mean(pcd.compute_nearest_neighbor_distance(device=device)))
    log.info(f"{avg_dist=}")
    radii = [f * avg_dist for f in radii_factors]
    log.info("Estimating normals")
    pcd.estimate_normals(search_param=KDTreeSearchParamHybrid(radius=avg_dist * 3, max_nn=20), device=device)
    pcd.orient_normals_consistent_tangent_plane(min(100, len(pcd.points) - 1), device=device)
    log.info("Creating mesh")
    rec_mesh = TriangleMesh.create_from_point_cloud_ball_pivoting(pcd, radii, device=device)
    rec_mesh.compute_vertex_normals()
    return rec_mesh


def meshfix(mesh, algo="pyt", nbe=0, device: int = 0):
    """surf_recon.py:38-85: close the holes of a reconstructed mesh. pyQSM hands the mesh to pymeshfix
    (``algo='pyt'``: ``fill_small_boundaries(nbe)``; ``'repair'``: ``MeshFix.repair``); here both run the
    device fill of DESIGN.md §26 (``TriangleMesh.fill_holes``): every boundary loop of at most ``nbe``
    edges (0: all, which means up to 128 here) gets its minimum-area triangulation over its own
    vertices. ``'repair'`` first keeps only the largest triangle cluster, as MeshFix does (the first of
    several equally large ones). Not MeshFix's triangulation or refinement; nothing is drawn, and no
    pymeshfix, pyvista or Open3D is needed. Returns the new mesh, with ``last_fill``; re-check it with
    ``mesh_processing.check_properties``."""
    if algo not in ("pyt", "repair"):
        raise ValueError(f"algo must be 'pyt' or 'repair', got {algo!r}")
    if not isinstance(mesh, TriangleMesh):
        mesh = TriangleMesh(np.asarray(mesh.vertices), np.asarray(mesh.triangles))
    if algo == "repair" and len(mesh.triangles):
        clusters, n, _ = mesh.cluster_connected_triangles(device=device)
        kept = TriangleMesh(mesh.vertices, mesh.triangles[clusters == int(np.argmax(n))])
        for name in ("vertex_normals", "vertex_colors"):
            if getattr(mesh, name, None) is not None:
                setattr(kept, name, getattr(mesh, name))
        mesh = kept
    log.info("Filling holes")
    out = mesh.fill_holes(max_edges=None if not nbe else int(nbe), device=device)
    log.info(f"{out.last_fill.stats}")
    return out
