"""Minimal stand-ins for the Open3D containers the hot path passes around.

The reference hands ``open3d.geometry.PointCloud`` / ``TriangleMesh`` objects to
its hot functions; Open3D is optional here. Every wrapper accepts NumPy arrays or
anything exposing ``.points`` (``np.asarray``-able) and returns these light
classes, which offer the few methods the reference's callers use on the results
(``select_by_index``, ``paint_uniform_color``, ``sample_points_uniformly`` ...).
"""
from __future__ import annotations

import numpy as np


def _hip():
    """The HIP bindings, imported on first use: this module imports without the library."""
    try:
        from .. import hip
    except ImportError:  # flat import (pyqsm_amd/ on sys.path)
        import os
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
        from pyqsm_amd import hip
    return hip


def as_points(obj) -> np.ndarray:
    """float64 [n,3] view/copy of an array or of an object with ``.points``."""
    if hasattr(obj, "points"):
        obj = obj.points
    pts = np.asarray(obj, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"expected [n,3] points, got shape {pts.shape}")
    return pts


class KDTreeSearchParamHybrid:
    """Open3D's ``KDTreeSearchParamHybrid``: up to ``max_nn`` nearest within ``radius``."""

    def __init__(self, radius, max_nn):
        self.radius = float(radius)
        self.max_nn = int(max_nn)


class KDTreeSearchParamKNN:
    """Open3D's ``KDTreeSearchParamKNN``: the ``knn`` nearest."""

    def __init__(self, knn=30):
        self.knn = int(knn)


def _search_param(param):
    """(radius or None, max_nn) of a search parameter object, read by duck typing so that Open3D's
    own classes work too: ``.radius`` and ``.max_nn`` (hybrid), or ``.knn``."""
    if param is None:
        return None, 30
    if hasattr(param, "radius") and hasattr(param, "max_nn"):
        return float(param.radius), int(param.max_nn)
    if hasattr(param, "knn"):
        return None, int(param.knn)
    raise TypeError(f"unsupported search parameter {param!r}: expected .radius/.max_nn or .knn")


def _normalized(v):
    """Rows divided by their length; zero rows stay zero (Eigen's normalize)."""
    v = np.asarray(v, dtype=np.float64)
    ln = np.linalg.norm(v, axis=1)
    out = v.copy()
    nz = ln > 0
    out[nz] = v[nz] / ln[nz, None]
    return out


class PointCloud:
    def __init__(self, points=None, colors=None, normals=None):
        self.points = np.zeros((0, 3)) if points is None else np.asarray(points, dtype=np.float64)
        self.colors = colors
        self.normals = None if normals is None else np.asarray(normals, dtype=np.float64)

    def __len__(self):
        return len(self.points)

    def __repr__(self):
        return f"PointCloud with {len(self.points)} points."

    def select_by_index(self, idx, invert: bool = False) -> "PointCloud":
        """The rows ``idx`` (or the others, in their order); normals and colours are carried when they have
        the cloud's length, as Open3D carries them."""
        idx = np.asarray(idx, dtype=np.int64)
        nrm = self.normals if self.has_normals() else None
        col = np.asarray(self.colors) if self.has_colors() else None
        if invert:
            mask = np.ones(len(self.points), dtype=bool)
            mask[idx] = False
            idx = mask
        return PointCloud(self.points[idx], colors=None if col is None else col[idx],
                          normals=None if nrm is None else nrm[idx])

    def has_colors(self) -> bool:
        return self.colors is not None and len(self.points) > 0 and len(self.colors) == len(self.points)

    def has_normals(self) -> bool:
        return self.normals is not None and len(self.normals) == len(self.points) and len(self.points) > 0

    def estimate_normals(self, search_param=None, fast_normal_computation: bool = True, device: int = 0):
        """Open3D's ``estimate_normals`` on the GPU (``hip.estimate_normals``). ``search_param``:
        anything with ``.radius`` and ``.max_nn`` (hybrid) or ``.knn`` (KNN), Open3D's own classes
        included; the default is the 30 nearest. Existing normals set the sign and are kept where a
        neighbourhood is degenerate; without them the sign makes n_z >= 0. Recollected from Open3D,
        parity unpinned. ``fast_normal_computation`` is accepted: there is one solver."""
        radius, max_nn = _search_param(search_param)
        prev = self.normals if self.has_normals() else None
        self.normals = _hip().estimate_normals(self.points, radius, max_nn, normals=prev, device=device)
        return True

    def orient_normals_consistent_tangent_plane(self, k, *args, device: int = 0, **kwargs):
        """Open3D's ``orient_normals_consistent_tangent_plane(k)`` on the GPU: signs made consistent
        along the minimum spanning forest of the kNN graph, every component rooted at its highest
        point with n_z >= 0 there (no Delaunay EMST edges: components are oriented apart). Open3D's
        newer ``lambda`` and ``cos_alpha_tol`` are accepted at their defaults (0, 1) only."""
        extra = dict(zip(("lambda", "cos_alpha_tol"), args))
        extra.update(kwargs)
        unknown = set(extra) - {"lambda", "lambda_", "cos_alpha_tol"}
        if unknown:
            raise TypeError(f"unexpected arguments {sorted(unknown)}")
        lam = extra.get("lambda", extra.get("lambda_", 0.0))
        tol = extra.get("cos_alpha_tol", 1.0)
        if float(lam) != 0.0 or float(tol) != 1.0:
            raise ValueError("only lambda = 0 and cos_alpha_tol = 1 are supported")
        if not self.has_normals():
            raise RuntimeError("the cloud has no normals: call estimate_normals first")
        self.normals = _hip().orient_normals_tangent_plane(self.points, self.normals, k, device=device)

    def normalize_normals(self) -> "PointCloud":
        if self.has_normals():
            self.normals = _normalized(self.normals)
        return self

    def paint_uniform_color(self, rgb):
        self.colors = np.tile(np.asarray(rgb, dtype=np.float64), (len(self.points), 1))
        return self

    def get_center(self):
        return self.points.mean(axis=0)

    def voxel_down_sample(self, voxel_size, device: int = 0) -> "PointCloud":
        """Open3D's ``voxel_down_sample`` on the GPU (``hip.voxel_down_sample``): the mean of every
        occupied voxel, colours and normals averaged the same way when present (normals then
        normalised). Recollected from Open3D,
        parity unpinned. Unlike Open3D (whose order comes from a hash map) the voxels are ordered
        by the smallest input index they hold."""
        col = None
        if self.colors is not None and len(np.asarray(self.colors)) == len(self.points):
            col = self.colors
        xyz, rgb = _hip().voxel_down_sample(self.points, voxel_size, colors=col, device=device)
        nrm = None
        if self.has_normals():  # the same per-voxel means, normalised (a zero mean stays zero)
            nrm = _normalized(_hip().voxel_down_sample(self.points, voxel_size, colors=self.normals,
                                                       device=device)[1])
        return PointCloud(xyz, rgb, nrm)

    def remove_statistical_outlier(self, nb_neighbors, std_ratio, print_progress: bool = False,
                                   device: int = 0):
        """Open3D's ``remove_statistical_outlier`` on the GPU (``hip.stat_outlier``): returns
        ``(cloud of the kept points, ind)``. ``ind`` is an int64 array of the kept indices in
        ascending order, not Open3D's list; ``select_by_index(ind)`` takes it as it is.
        Recollected from Open3D, parity unpinned. ``print_progress`` is accepted and ignored."""
        ind = _hip().stat_outlier(self.points, nb_neighbors, std_ratio, device=device)
        return self.select_by_index(ind), ind

    def compute_nearest_neighbor_distance(self, device: int = 0) -> np.ndarray:
        """Open3D's ``compute_nearest_neighbor_distance``: float64 [n], the distance from every point
        to its nearest other point (``hip.knn`` with k = 1; 0 for coincident points). Open3D returns
        a list; fewer than two points give zeros, as there."""
        if len(self.points) < 2:
            return np.zeros(len(self.points))
        return np.sqrt(_hip().knn(self.points, 1, exclude_self=True, device=device)[1][:, 0])

    def get_min_bound(self):
        return self.points.min(axis=0)

    def get_max_bound(self):
        return self.points.max(axis=0)

    def compute_convex_hull(self, quantum=None, device: int = 0):
        """Open3D's ``compute_convex_hull``: ``(TriangleMesh, vertex indices)``, the mesh over the
        hull's vertices only (re-indexed, outward triangles), the indices ascending into this cloud.
        The hull is the exact one of ``geometry.hull.convex_hull`` (on the GPU, no SciPy)."""
        from .hull import convex_hull
        h = convex_hull(self.points, quantum=quantum, device=device)
        if h.dim < 3:
            raise ValueError(f"the cloud has no 3-D convex hull (affine dimension {h.dim})")
        remap = np.full(len(self.points), -1, np.int32)
        remap[h.vertices] = np.arange(len(h.vertices), dtype=np.int32)
        return TriangleMesh(self.points[h.vertices], remap[h.simplices]), h.vertices

    def get_oriented_bounding_box(self, quantum=None, device: int = 0):
        """Open3D's ``get_oriented_bounding_box``: the PCA box of the convex hull's vertices, as a
        ``geometry.hull.OrientedBoundingBox``."""
        from .hull import OrientedBoundingBox
        return OrientedBoundingBox.create_from_points(self.points, quantum=quantum, device=device)

    def segment_plane(self, distance_threshold=0.01, ransac_n=3, num_iterations=100, probability=0.99999999,
                      seed=None, samples=None, device: int = 0):
        """Open3D's ``segment_plane`` on the GPU (``hip.segment_plane``): returns ``(plane_model [4],
        inliers)``, the least-squares plane ``(a, b, c, d)`` through the inliers of the best of
        ``num_iterations`` hypotheses of ``ransac_n`` points each, and the inliers as an int64 array
        in ascending order (``select_by_index`` takes it). Recollected from Open3D, parity unpinned
        (DESIGN.md §20): the normal's sign makes c > 0, hypotheses with equal counts keep the earlier
        one (Open3D compares an error sum whose value depends on the summation order), and the
        hypotheses are drawn from ``seed`` (``math_utils.fit.draw_plane_samples``) or given as
        ``samples`` int64 [num_iterations, ransac_n]. No hypothesis with an inlier: a zero plane and
        no inliers."""
        if samples is None:
            samples = _fit().draw_plane_samples(len(self.points), int(num_iterations), int(ransac_n), seed=seed)
        fit, _, inliers, _, _ = _hip().segment_plane(self.points, samples, distance_threshold, probability,
                                                     device=device)
        return fit, inliers

    def segment_planes(self, distance_threshold, max_planes=4, min_inliers=100, ransac_n=3, num_iterations=1000,
                       probability=0.99999999, axis=None, max_angle_deg=None, seed=None, draws=None,
                       device: int = 0):
        """Up to ``max_planes`` planes peeled off the cloud in one device-resident call
        (``hip.segment_planes``): every round is ``segment_plane`` on the points no earlier plane
        took, until a round's best plane has fewer than ``min_inliers`` inliers. With ``axis`` and
        ``max_angle_deg`` only planes whose normal lies within that angle of ``axis`` (either sign)
        are considered. Returns a ``hip.PlaneSegments``: ``.planes``, ``.hypothesis_planes``,
        ``.labels``, ``.counts``, ``.indices(i)``, ``.rest()``. ``draws``: uint64 [max_planes,
        num_iterations, ransac_n] (``math_utils.fit.draw_u64``), drawn from ``seed`` when omitted."""
        if draws is None:
            draws = _fit().draw_u64((int(max_planes), int(num_iterations), int(ransac_n)), seed=seed)
        axis, cos_limit = cone_args(axis, max_angle_deg)
        return _hip().segment_planes(self.points, draws, distance_threshold, probability, min_inliers, axis=axis,
                                     cos_limit=cos_limit, device=device)


def _fit():
    """``math_utils.fit``, imported on first use (it imports this module)."""
    try:
        from ..math_utils import fit
    except ImportError:  # flat import (pyqsm_amd/ on sys.path)
        _hip()
        from pyqsm_amd.math_utils import fit
    return fit


def cone_args(axis, max_angle_deg):
    """``(unit axis or None, cos_limit)`` as the plane kernels take them: ``cos_limit =
    cos(radians(max_angle_deg))``, 0 (no cone) without an axis or an angle."""
    import math
    if axis is None or max_angle_deg is None:
        return None, 0.0
    ax = np.asarray(axis, dtype=np.float64).reshape(3)
    ln = float(np.sqrt((ax * ax).sum()))
    if not ln > 0 or not np.isfinite(ln):
        raise ValueError("the cone's axis must be a finite non-zero vector")
    return ax / ln, math.cos(math.radians(float(max_angle_deg)))


class Voxel:
    """Open3D's ``Voxel``: ``grid_index`` int32 [3] and ``color`` f64 [3]."""

    def __init__(self, grid_index, color=None):
        self.grid_index = np.asarray(grid_index, dtype=np.int32)
        self.color = np.zeros(3) if color is None else np.asarray(color, dtype=np.float64)

    def __repr__(self):
        return f"Voxel with grid_index: ({', '.join(str(int(v)) for v in self.grid_index)})"


class VoxelGrid:
    """Open3D's ``VoxelGrid`` as pyQSM uses it, on the GPU (``hip.VoxelGrid``): the occupied voxels
    of a cloud stay on the device and tiles are checked against them. Recollected from Open3D,
    parity unpinned. The voxels are ordered by the smallest input index they hold (Open3D's order
    comes from a hash map), and a query far outside the box is simply not included (Open3D's cast
    to int wraps there)."""

    def __init__(self, device_grid=None):
        self._grid = device_grid

    @staticmethod
    def create_from_point_cloud(input, voxel_size, device: int = 0) -> "VoxelGrid":
        col = getattr(input, "colors", None)
        pts = as_points(input)
        if col is not None and len(np.asarray(col)) != len(pts):
            col = None
        return VoxelGrid(_hip().VoxelGrid(pts, voxel_size, colors=col, device=device))

    @property
    def origin(self):
        return self._grid.origin

    @property
    def voxel_size(self):
        return self._grid.voxel_size

    @property
    def device_grid(self):
        """The ``hip.VoxelGrid`` behind this one (rows, indices, inverted queries)."""
        return self._grid

    def check_if_included(self, queries) -> np.ndarray:
        """bool [m] (Open3D returns a list of bool)."""
        return self._grid.query(as_points(queries))

    def get_voxels(self):
        gi, col = self._grid.voxels()
        return [Voxel(gi[r], None if col is None else col[r]) for r in range(len(gi))]

    def __repr__(self):
        return f"VoxelGrid with {self._grid.n_voxels} voxels."


class TriangleMesh:
    """vertices f64/f32 [V,3], triangles int [T,3]."""

    def __init__(self, vertices, triangles):
        self.vertices = np.asarray(vertices)
        self.triangles = np.asarray(triangles, dtype=np.int64)

    # ---- surface reconstruction on the GPU (hip.ball_pivot)

    @staticmethod
    def create_from_point_cloud_ball_pivoting(pcd, radii, quantum=None, device: int = 0, *, max_tests=None):
        """Open3D's ``create_from_point_cloud_ball_pivoting`` by a contract of its own: every triangle
        of cloud points on which a ball of one of the ``radii`` can rest from the normals' side
        without holding another point, decided exactly on the cloud SNAPPED to a lattice
        (``hip.ball_pivot``). Order-free and the same bits on every run; it is NOT
        Open3D's triangle list, whose front depends on its traversal order, and parity with it is
        unverified. Non-manifold configurations are not repaired:
        ``mesh_processing.check_properties`` reports them.

        ``pcd`` needs ``.points`` and ``.normals``. ``radii`` (any order) are processed ascending.
        ``quantum``: the lattice pitch, a power of two; default the larger of
        ``mesh_processing.quantize_mesh``'s (extent / 2^20) and the smallest at which the largest
        radius is at most 2^11 lattice units, the kernel's bound. Points snap to
        ``rint(p / quantum)``, normals to ``rint(n * 2^14)``, a radius to
        ``floor((r / quantum)^2)`` as its square. ``max_tests``: ``hip.ball_pivot``'s work cap. The result keeps the cloud's points as vertices
        (all of them, in order) and carries ``triangle_levels`` (index into the ascending radii),
        ``n_unresolved_ties`` and ``quantum``."""
        import math
        from .mesh_processing import _check_quantum, _quantum_for
        hip = _hip()
        pts = as_points(pcd)
        nrm = getattr(pcd, "normals", None)
        if nrm is None or len(np.asarray(nrm)) != len(pts):
            raise ValueError("the cloud has no normals: estimate_normals and "
                             "orient_normals_consistent_tangent_plane first")
        if not np.isfinite(pts).all():
            raise ValueError("point coordinates must be finite")
        r = np.sort(np.asarray(list(radii), dtype=np.float64).reshape(-1))
        if r.size == 0 or not np.isfinite(r).all() or r[0] <= 0:
            raise ValueError("radii must be positive and finite")
        max_rho = float(1 << 11)
        m, e = math.frexp(float(r[-1]) / max_rho)          # the smallest power of two >= r / 2^11
        q_fit = math.ldexp(1.0, e - 1 if m == 0.5 else e)
        if quantum is None:
            ext = float((pts.max(axis=0) - pts.min(axis=0)).max()) if len(pts) else 0.0
            q = max(_quantum_for(ext), q_fit)
        else:
            q = _check_quantum(quantum)
            if r[-1] / q > max_rho:
                raise ValueError(f"radius {float(r[-1])!r} is {r[-1] / q:.0f} lattice units at quantum {q!r}, more "
                                 f"than 2^11: a quantum of {q_fit!r} would fit")
        rho2 = [int(np.floor((x / q) ** 2)) for x in r]
        if rho2[0] < 1:
            raise ValueError(f"radius {float(r[0])!r} is below the quantum {q!r}")
        scaled = np.rint(pts / q)
        if len(pts) and np.abs(scaled).max() >= 2.0 ** 62:
            raise ValueError("quantum is too small for these coordinates")
        lat = scaled.astype(np.int64)
        if len(pts):
            lat -= lat.min(axis=0)
            if lat.max() >= 1 << 31:
                raise ValueError(f"the cloud spans {int(lat.max())} lattice units at quantum {q!r}, more than "
                                 "2^31: use a larger quantum")
        res = hip.ball_pivot(lat.astype(np.int32), hip.snap_normals(_normalized(nrm)), rho2, max_tests=max_tests,
                             device=device)
        mesh = TriangleMesh(pts, res.triangles)
        mesh.triangle_levels = res.levels
        mesh.n_unresolved_ties = res.n_unresolved_ties
        mesh.quantum = q
        mesh.stats = res.stats
        return mesh

    # ---- the 3-D alpha shape on the GPU (hip.alpha_shape3)

    @staticmethod
    def create_from_point_cloud_alpha_shape(pcd, alpha, tetra_mesh=None, pt_map=None, quantum=None,
                                            device: int = 0, *, max_tests=None):
        """Open3D's ``create_from_point_cloud_alpha_shape`` by a contract of its own: the triangles of cloud
        points with exactly one empty ball of radius ``alpha`` through them, oriented out of the solid and
        decided exactly on the cloud SNAPPED to a lattice (``geometry.hull.alpha_shape``). In
        general position that is the boundary of the Delaunay tetrahedra of circumradius below alpha, which
        Open3D extracts; triangle-for-triangle parity with it is unverified. ``tetra_mesh`` and ``pt_map``
        are accepted and ignored: no tetrahedral mesh is built. It needs no normals.

        The result keeps the cloud's points as vertices (all of them, in order) and carries ``volume`` and
        ``six_volume`` (meaningful only when ``n_unresolved_ties`` is 0), ``n_unresolved_ties``, ``quantum``
        and ``stats``."""
        try:
            from .hull import alpha_shape
        except ImportError:  # flat import (pyqsm_amd/ on sys.path)
            _hip()
            from pyqsm_amd.geometry.hull import alpha_shape
        shape = alpha_shape(pcd, alpha, quantum=quantum, device=device, max_tests=max_tests)
        mesh = shape.to_mesh()
        mesh.volume = shape.volume
        mesh.six_volume = shape.six_volume
        mesh.n_unresolved_ties = shape.n_unresolved_ties
        mesh.quantum = shape.quantum
        mesh.stats = shape.stats
        return mesh

    def compute_vertex_normals(self, normalized: bool = True) -> "TriangleMesh":
        """Open3D's ``compute_vertex_normals``, minimal: the sum of the (area-weighted) normals of
        the triangles at each vertex, normalised; a vertex without triangles gets (0, 0, 1) as in
        Open3D. Host NumPy; sets ``vertex_normals`` and ``triangle_normals``."""
        v = np.asarray(self.vertices, dtype=np.float64)
        t = self.triangles
        fn = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]) if len(t) else np.zeros((0, 3))
        vn = np.zeros_like(v)
        for k in range(3):
            np.add.at(vn, t[:, k], fn)
        if normalized:
            ln = np.linalg.norm(vn, axis=1)
            vn[ln > 0] /= ln[ln > 0, None]
            vn[ln == 0] = (0.0, 0.0, 1.0)
        self.triangle_normals = _normalized(fn)
        self.vertex_normals = vn
        return self

    def get_center(self):
        return self.vertices.mean(axis=0)

    def get_surface_area(self) -> float:
        v = self.vertices.astype(np.float64)
        a, b, c = (v[self.triangles[:, k]] for k in range(3))
        return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())

    def select_by_triangle(self, tri_idx) -> "TriangleMesh":
        tris = self.triangles[np.asarray(tri_idx, dtype=np.int64)]
        used, inv = np.unique(tris, return_inverse=True)
        return TriangleMesh(self.vertices[used], inv.reshape(-1, 3))

    def select_by_index(self, vertex_idx) -> "TriangleMesh":
        """Open3D's legacy ``TriangleMesh.select_by_index``: the listed VERTICES, and every
        triangle whose three vertices are all among them (also triangles nobody asked for,
        on meshes that share vertices) in their original order."""
        vid = np.asarray(vertex_idx, dtype=np.int64).reshape(-1)
        new_of = np.full(len(self.vertices), -1, dtype=np.int64)
        first = np.unique(vid, return_index=True)[1]
        vid = vid[np.sort(first)]                      # duplicates keep their first position
        new_of[vid] = np.arange(len(vid))
        tris = new_of[self.triangles] if len(self.triangles) else np.zeros((0, 3), dtype=np.int64)
        keep = (tris >= 0).all(axis=1)
        return TriangleMesh(self.vertices[vid], tris[keep])

    # ---- mesh checks on the GPU (hip.mesh_topology / hip.mesh_self_intersections).
    # Everything is decided by vertex index, as in Open3D: coincident vertices are not welded.
    # Every method below runs the whole topology call (or the whole sweep) for its one answer: for
    # several answers about one mesh call mesh_processing.check_properties, or hip.mesh_topology, once.

    def _topology(self, areas: bool = False, device: int = 0):
        verts = np.asarray(self.vertices, dtype=np.float64) if areas else None
        return _hip().mesh_topology(self.triangles, len(self.vertices), verts, device=device)

    def _intersections(self, return_pairs: bool, max_tests=None, device: int = 0):
        from .mesh_processing import quantize_mesh
        ijk = quantize_mesh(self.vertices)[0]
        return _hip().mesh_self_intersections(ijk, self.triangles, return_pairs=return_pairs, max_tests=max_tests,
                                              device=device)

    def cluster_connected_triangles(self, device: int = 0):
        """Open3D's ``cluster_connected_triangles``: ``(triangle_clusters int32 [T],
        cluster_n_triangles int64 [C], cluster_area float64 [C])``; triangles that share an edge are
        connected. Unlike Open3D (whose numbering follows its search order) the clusters are
        numbered by their smallest triangle."""
        top = self._topology(areas=True, device=device)
        return top.tri_cluster, top.cluster_n, top.cluster_area

    def get_non_manifold_edges(self, allow_boundary_edges: bool = True, device: int = 0) -> np.ndarray:
        """int32 [r, 2]: the edges with more than two triangles, and with
        ``allow_boundary_edges=False`` those with one triangle too; ascending by (a, b)."""
        top = self._topology(device=device)
        bad = top.edge_count > 2 if allow_boundary_edges else top.edge_count != 2
        return top.edges[bad]

    def is_edge_manifold(self, allow_boundary_edges: bool = True, device: int = 0) -> bool:
        """No edge with more than two triangles (nor, with ``allow_boundary_edges=False``, with one).
        One topology call per answer: ``mesh_processing.check_properties`` gives all of them at once."""
        s = self._topology(device=device).summary
        return s["over_two_edges"] == 0 and (allow_boundary_edges or s["boundary_edges"] == 0)

    def get_non_manifold_vertices(self, device: int = 0) -> np.ndarray:
        """int64 indices, ascending, of the vertices whose triangles do not form one fan."""
        return np.nonzero(self._topology(device=device).vertex_flags)[0]

    def is_vertex_manifold(self, device: int = 0) -> bool:
        """The triangles at every vertex form one fan (see ``check_properties`` for several answers)."""
        return self._topology(device=device).summary["non_manifold_vertices"] == 0

    def is_orientable(self, device: int = 0) -> bool:
        """Some choice of flips makes all triangles at shared edges agree. A mesh with an edge of
        more than two triangles is not orientable here (Open3D's answer there depends on its
        search order)."""
        return bool(self._topology(device=device).summary["orientable"])

    def get_self_intersecting_triangles(self, max_tests=None, device: int = 0) -> np.ndarray:
        """int32 [n, 2] pairs ``i < j`` of intersecting triangles, ascending (Open3D's order comes
        from its loop). Exact for the mesh snapped to a lattice: ``mesh_processing.quantize_mesh``."""
        return self._intersections(True, max_tests, device).pairs

    def is_self_intersecting(self, max_tests=None, device: int = 0) -> bool:
        """``max_tests`` caps the brute-force sweep's T (T - 1) / 2 pairs (``hip.mesh_self_intersections``)."""
        return self._intersections(False, max_tests, device).n_pairs > 0

    def is_watertight(self, max_tests=None, device: int = 0) -> bool:
        """Edge-manifold without boundary, vertex-manifold and not self-intersecting (Open3D): one
        topology call and one sweep, as ``mesh_processing.check_properties``, which also says why not."""
        s = self._topology(device=device).summary
        return (s["over_two_edges"] == 0 and s["boundary_edges"] == 0 and s["non_manifold_vertices"] == 0
                and not self.is_self_intersecting(max_tests=max_tests, device=device))

    # ---- hole filling on the GPU (hip.mesh_boundary_loops / hip.mesh_fill_holes)

    def get_boundary_loops(self, device: int = 0):
        """The boundary loops as a list of int32 vertex arrays, each from its smallest vertex in the
        direction a patch would run, ascending by that vertex (``hip.mesh_boundary_loops``)."""
        res = _hip().mesh_boundary_loops(self.triangles, len(self.vertices), device=device)
        return [res.loop(i) for i in range(len(res.ptr) - 1)]

    def fill_holes(self, max_edges=None, device: int = 0) -> "TriangleMesh":
        """A new mesh with every boundary loop of at most ``max_edges`` edges (None: 128, the kernel's
        bound) closed by its minimum-area triangulation; the new rows follow the old ones, no vertex
        is added. Not Open3D's ``fill_holes`` nor MeshFix's patches: a contract of its own (DESIGN.md
        §26). The result carries ``last_fill`` (``hip.HoleFill``: loops, flags, areas, statistics);
        ``vertex_normals`` and ``vertex_colors`` carry over. Loops that repeat a vertex stay open."""
        res = _hip().mesh_fill_holes(self.triangles, np.asarray(self.vertices, dtype=np.float64), max_edges,
                                     device=device)
        out = TriangleMesh(self.vertices, np.concatenate([self.triangles, res.new_tris.astype(np.int64)]))
        for name in ("vertex_normals", "vertex_colors"):
            if getattr(self, name, None) is not None:
                setattr(out, name, getattr(self, name))
        out.last_fill = res
        return out

    def remove_triangles_by_mask(self, mask) -> "TriangleMesh":
        """Open3D's ``remove_triangles_by_mask``: drops the triangles where ``mask`` is true, in
        place; the vertices stay. Host NumPy."""
        m = np.asarray(mask, dtype=bool).reshape(-1)
        if m.shape[0] != len(self.triangles):
            raise ValueError(f"one mask entry per triangle: {m.shape[0]} for {len(self.triangles)}")
        self.triangles = self.triangles[~m]
        return self

    def remove_degenerate_triangles(self) -> "TriangleMesh":
        """Open3D's ``remove_degenerate_triangles``: drops the triangles that repeat a vertex index,
        in place. Host NumPy."""
        t = self.triangles
        return self.remove_triangles_by_mask((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2]))


class Cylinder:
    """The primitive fit_shape_RANSAC returns (the reference builds an Open3D
    cylinder mesh at fit.py:322-332): centre, axis, radius, height."""

    def __init__(self, center, radius, height, axis=(0.0, 0.0, 1.0)):
        self.center = np.asarray(center, dtype=np.float64)
        self.radius = float(radius)
        self.height = float(height)
        ax = np.asarray(axis, dtype=np.float64)
        nrm = np.linalg.norm(ax)
        self.axis = ax / nrm if nrm > 0 else np.array([0.0, 0.0, 1.0])

    def __repr__(self):
        return (f"Cylinder(center={self.center.tolist()}, radius={self.radius:.4f}, "
                f"height={self.height:.4f}, axis={self.axis.tolist()})")

    def _frame(self):
        helper = np.array([1.0, 0, 0]) if abs(self.axis[0]) < 0.9 else np.array([0, 1.0, 0])
        u = np.cross(self.axis, helper)
        u /= np.linalg.norm(u)
        return u, np.cross(self.axis, u)

    def sample_points_uniformly(self, number_of_points: int = 100, seed: int = 0) -> PointCloud:
        """Points on the lateral surface (area-uniform)."""
        rng = np.random.default_rng(seed)
        ang = rng.uniform(0, 2 * np.pi, number_of_points)
        h = rng.uniform(-self.height / 2, self.height / 2, number_of_points)
        u, v = self._frame()
        pts = (self.center + self.radius * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * v)
               + h[:, None] * self.axis)
        return PointCloud(pts)
