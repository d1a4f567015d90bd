"""Mesh checks on the HIP kernels: pyQSM's ``geometry/mesh_processing.py`` (``check_properties``,
``get_surface_clusters``, ``cluster_and_remove_triangles``), which asks Open3D whether a
reconstructed mesh is closed, manifold and free of self-intersections before rays are cast at it.

Open3D is not a dependency of this package and its answers depend on hash-map and search order, so
the results follow a contract of their own (tests/mesh_restatement.py states it in
NumPy): integer decisions only, a fixed output order, the same bits on every run.

Differences from Open3D, all deliberate:

* Clusters are numbered by their smallest triangle; edges, vertices and intersecting pairs are
  returned in ascending order.
* Self-intersection is decided exactly, on the mesh SNAPPED to an integer lattice
  (:func:`quantize_mesh`); Open3D tests in floating point.
* A mesh with an edge of more than two triangles is reported as not orientable.
* Holes are closed by :func:`fill_small_boundaries` (``hip.mesh_fill_holes``): minimum-area
  patches over the loops' own vertices in a fixed order, not MeshFix's or Open3D's triangulation; no
  refinement, no welding, no joining of components, and a patch is not tested against the mesh.
* ``map_density``, ``subdivide_mesh`` and all drawing are out of scope: nothing is plotted here, and
  with pyQSM behind this package on ``sys.path`` those names still resolve to pyQSM's own file.
"""
from __future__ import annotations

import numpy as np

try:
    from .. import hip
    from .._shadow import fall_through
    from ..viz.projection import _check_quantum, _quantum_for
    from .cloud import TriangleMesh
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyqsm_amd import hip
    from pyqsm_amd._shadow import fall_through
    from pyqsm_amd.viz.projection import _check_quantum, _quantum_for
    from pyqsm_amd.geometry.cloud import TriangleMesh

# names pyQSM's module of the same name defines and this one does not (pyqsm_amd/_shadow.py)
__getattr__ = fall_through(__name__)


def quantize_mesh(vertices, quantum=None):
    """Snap ``vertices`` [V,3] to an integer lattice. Returns ``(ijk, quantum, origin)``: int32
    [V,3] with every axis starting at 0, the lattice pitch, and the lattice node ``ijk = 0`` stands
    for (float64 [3], a multiple of the pitch). Host NumPy.

    The pitch is ``quantum`` if given (a power of two), else the smallest power of two at which the
    largest extent spans at most 2^20 lattice units, the rule of ``viz.projection.quantize_plane``:
    2^-14 m, about 0.06 mm, for a 50 m crown. ``ijk = rint(v / quantum)`` on the absolute lattice,
    shifted by its minimum, so quantising lattice output again changes nothing.

    What follows for the self-intersection test: its answers are exact for the SNAPPED mesh, not
    for the floating-point one. A feature smaller than the pitch may close or open, vertices that
    snap to one node count as touching (their triangles intersect unless they share an index), and
    a sliver may snap to a degenerate triangle, which is then reported by no pair."""
    v = np.asarray(vertices, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"expected vertices of shape [V,3], got {v.shape}")
    if not np.isfinite(v).all():
        raise ValueError("vertex coordinates must be finite")
    if v.shape[0] == 0:
        q = 1.0 if quantum is None else _check_quantum(quantum)
        return np.zeros((0, 3), np.int32), q, np.zeros(3)
    q = _quantum_for(float((v.max(axis=0) - v.min(axis=0)).max())) if quantum is None else _check_quantum(quantum)
    scaled = np.rint(v / q)                       # q is a power of two: the division is exact
    if np.abs(scaled).max() >= 2.0 ** 62:
        raise ValueError("quantum is too small for these coordinates")
    lat = scaled.astype(np.int64)
    low = lat.min(axis=0)
    lat -= low
    if lat.max() > hip.MESH_MAX_EXTENT:
        raise ValueError(f"the mesh spans {int(lat.max())} lattice units at quantum {q!r}, more than 2^20: "
                         "use a larger quantum")
    return lat.astype(np.int32), q, low.astype(np.float64) * q


def _as_mesh(mesh) -> TriangleMesh:
    """A ``TriangleMesh`` of this package from anything with ``.vertices`` and ``.triangles``."""
    if isinstance(mesh, TriangleMesh):
        return mesh
    return TriangleMesh(np.asarray(mesh.vertices), np.asarray(mesh.triangles))


def check_properties(mesh, draw_result=False, max_tests=None, device: int = 0) -> dict:
    """pyQSM's ``check_properties``: the six answers it prints (``edge_manifold``,
    ``edge_manifold_boundary``, ``vertex_manifold``, ``self_intersecting``, ``watertight``,
    ``orientable``) and what offends, as arrays: ``non_manifold_edges`` (more than two triangles),
    ``boundary_edges``, ``non_manifold_vertices``, ``self_intersecting_pairs``; plus the ``quantum``
    the intersection test snapped to. One topology call and one sweep. Triangles that repeat a
    vertex index are refused: ``remove_degenerate_triangles`` first. ``max_tests`` caps the sweep's
    T (T - 1) / 2 triangle pairs (``hip.mesh_self_intersections``). Nothing is drawn: ``draw_result`` is
    accepted and ignored."""
    m = _as_mesh(mesh)
    top = hip.mesh_topology(m.triangles, len(m.vertices), device=device)
    ijk, q, _ = quantize_mesh(m.vertices)
    hits = hip.mesh_self_intersections(ijk, m.triangles, return_pairs=True, max_tests=max_tests, device=device)
    s = top.summary
    edge_manifold = s["over_two_edges"] == 0
    edge_manifold_boundary = edge_manifold and s["boundary_edges"] == 0
    vertex_manifold = s["non_manifold_vertices"] == 0
    self_intersecting = hits.n_pairs > 0
    return {
        "edge_manifold": edge_manifold,
        "edge_manifold_boundary": edge_manifold_boundary,
        "vertex_manifold": vertex_manifold,
        "self_intersecting": self_intersecting,
        "watertight": edge_manifold_boundary and vertex_manifold and not self_intersecting,
        "orientable": bool(s["orientable"]),
        "non_manifold_edges": top.edges[top.edge_count > 2],
        "boundary_edges": top.edges[top.edge_count == 1],
        "non_manifold_vertices": np.nonzero(top.vertex_flags)[0],
        "self_intersecting_pairs": hits.pairs,
        "quantum": q,
    }


def surface_cluster_mask(cluster_n, cluster_area, top_n_clusters=10, min_cluster_area=None,
                         max_cluster_area=None) -> np.ndarray:
    """bool [C]: the clusters :func:`get_surface_clusters` keeps. With ``top_n_clusters`` those with
    at least as many triangles as the ``top_n_clusters``-th largest (ties are kept); with
    ``min_cluster_area`` / ``max_cluster_area`` those whose area lies inside the closed bounds."""
    n = np.asarray(cluster_n)
    area = np.asarray(cluster_area)
    keep = np.ones(len(n), bool)
    if top_n_clusters and len(n) > int(top_n_clusters):
        keep &= n >= np.sort(n)[-int(top_n_clusters)]
    if min_cluster_area is not None:
        keep &= area >= float(min_cluster_area)
    if max_cluster_area is not None:
        keep &= area <= float(max_cluster_area)
    return keep


def get_surface_clusters(mesh, top_n_clusters=10, min_cluster_area=None, max_cluster_area=None, device: int = 0):
    """pyQSM's ``get_surface_clusters``: the connected components of the mesh, filtered by size and
    area (:func:`surface_cluster_mask`). Returns ``(kept, removed, triangle_clusters)``: two new
    meshes over the same vertices, and the cluster of every triangle of the input. pyQSM's area
    filters are unfinished (the minimum is computed and dropped, the maximum removes what lies
    below it); here both bounds mean what their names say."""
    m = _as_mesh(mesh)
    clusters, n, area = m.cluster_connected_triangles(device=device)
    keep = surface_cluster_mask(n, area, top_n_clusters, min_cluster_area, max_cluster_area)[clusters]
    return (TriangleMesh(m.vertices, m.triangles[keep]), TriangleMesh(m.vertices, m.triangles[~keep]), clusters)


def fill_small_boundaries(mesh, nbe=0, device: int = 0):
    """pymeshfix's ``fill_small_boundaries`` by this package's contract: closes every
    boundary loop of at most ``nbe`` edges (0: all, which here means up to ``hip.FILL_MAX_LOOP`` = 128)
    with its minimum-area triangulation, without new vertices or refinement. Returns ``(mesh,
    n_filled)``: a new mesh (``TriangleMesh.fill_holes``) and the number of loops closed. A larger
    ``nbe`` than 128 is refused."""
    m = _as_mesh(mesh).fill_holes(max_edges=None if not nbe else int(nbe), device=device)
    return m, m.last_fill.stats["loops_filled"]


def cluster_and_remove_triangles(mesh, min_triangles=200, device: int = 0) -> TriangleMesh:
    """pyQSM's ``cluster_and_remove_triangles`` (which draws its result and returns the input): a
    new mesh without the clusters of fewer than ``min_triangles`` triangles. The input is left as
    it is."""
    m = _as_mesh(mesh)
    clusters, n, _ = m.cluster_connected_triangles(device=device)
    return TriangleMesh(m.vertices, m.triangles[n[clusters] >= int(min_triangles)])
