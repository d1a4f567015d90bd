"""Convex hulls and oriented bounding boxes on the HIP kernels.

    convex_hull(points)            what scipy.spatial.ConvexHull(points) is to pyQSM: .simplices,
                                   .vertices, .volume, .area (utils/lib_integration.py:31)
    convex_hulls(points, seg_start)    the same for many clouds in one call
    alpha_shape(points, alpha)     the 3-D alpha shape, what Open3D's create_from_point_cloud_alpha_shape is
                                   to pyQSM (surf_recon.py get_mesh, skeletonize.py): .triangles, .kinds,
                                   .vertices, .volume, .area of a surface that follows the concavities
    alpha_shapes(points, seg_start, alpha)   the same for many clouds in one call
    OrientedBoundingBox            Open3D's PCA box of the hull's vertices, what
                                   pcd.get_oriented_bounding_box() returns (skeletonize.py:240,
                                   point_cloud_processing.py:306, reconstruction.py:56), with
                                   get_point_indices_within_bounding_box on the GPU

The hull is exact for the points snapped to a lattice (``mesh_processing.quantize_mesh``: a
power-of-two pitch, at most 2^20 units over the largest extent) and canonical: on degenerate
input it is the same answer on every run (``pyqsm_convex_hull``). Volume and
area are host work over the few facets, from exact integers.
"""
from __future__ import annotations

import numpy as np

try:
    from .. import hip
    from .cloud import TriangleMesh, as_points
    from .mesh_processing import quantize_mesh
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyqsm_amd import hip
    from pyqsm_amd.geometry.cloud import TriangleMesh, as_points
    from pyqsm_amd.geometry.mesh_processing import quantize_mesh


def six_volume(ijk, tris) -> int:
    """Six times the volume enclosed by outward triangles over lattice points: the exact integer
    sum of the fan determinants from the first triangle's first vertex (Python integers)."""
    tris = np.asarray(tris)
    if len(tris) == 0:
        return 0
    p = np.asarray(ijk, dtype=np.int64)
    o = p[tris[0, 0]]
    a, b, c = (p[tris[:, k]] - o for k in range(3))      # differences below 2^20
    det = (np.cross(a, b) * c).sum(axis=1)               # below 6 * 2^60 each
    return sum(int(d) for d in det)


def twice_area_normals(ijk, tris) -> np.ndarray:
    """The exact integer normals (b - a) x (c - a) of the triangles, int64 [T, 3]: their lengths are
    twice the areas."""
    p = np.asarray(ijk, dtype=np.int64)
    tris = np.asarray(tris)
    return np.cross(p[tris[:, 1]] - p[tris[:, 0]], p[tris[:, 2]] - p[tris[:, 0]])


class ConvexHull:
    """One cloud's hull. ``simplices`` int32 [T, 3]: outward triangles, the smallest index first,
    ascending; ``vertices``: ascending indices, as Qhull lists them in 3-D; ``six_volume``: Python
    int in lattice units^3; ``volume`` / ``area`` in the points' units; ``dim``: the affine
    dimension of the distinct lattice points (below 3: no simplices, volume and area 0);
    ``quantum`` / ``origin``: the lattice; ``stats``: the call's counters."""

    def __init__(self, points, ijk, simplices, dim, quantum, origin, stats=None):
        self.points = points
        self.ijk = ijk
        self.simplices = simplices
        self.dim = int(dim)
        self.quantum = float(quantum)
        self.origin = origin
        self.stats = stats or {}
        self.vertices = np.unique(simplices).astype(np.int64)
        self.six_volume = six_volume(ijk, simplices)
        self.volume = self.six_volume / 6.0 * self.quantum ** 3
        nrm = twice_area_normals(ijk, simplices) if len(simplices) else np.zeros((0, 3), np.int64)
        # |n|^2 < 3 * 2^82 does not fit int64: squared in Python integers, then one rounding to fp64
        n2 = [int(x) * int(x) + int(y) * int(y) + int(z) * int(z) for x, y, z in nrm]
        self.area = 0.5 * self.quantum ** 2 * float(sum(np.sqrt(float(v)) for v in n2))

    def to_mesh(self) -> TriangleMesh:
        """The hull as a mesh over ALL the points (indices unchanged), pyQSM's ``sps_hull_to_mesh``."""
        return TriangleMesh(self.points, self.simplices.astype(np.int32))


def _lattice(points, quantum):
    pts = as_points(points)
    ijk, q, origin = quantize_mesh(pts, quantum)
    return pts, ijk, q, origin


def convex_hull(points, quantum=None, device: int = 0, max_tests=None) -> ConvexHull:
    """The convex hull of ``points`` ([n, 3], or anything with ``.points``) on the GPU, exact for
    the points snapped to the lattice of pitch ``quantum`` (default: the smallest power of two at
    which the largest extent spans at most 2^20 units)."""
    pts, ijk, q, origin = _lattice(points, quantum)
    r = hip.convex_hull(ijk, None, max_tests=max_tests, device=device)
    return ConvexHull(pts, ijk, r.tris, r.dim[0] if len(r.dim) else -1, q, origin, r.stats)


def convex_hulls(points, seg_start, quantum=None, device: int = 0, max_tests=None) -> list:
    """One :class:`ConvexHull` per segment ``points[seg_start[s]:seg_start[s + 1]]`` from a single
    call; one lattice for all of them (a segment may span 2^20 units, the whole cloud any number).
    The simplices of each hull index into its own segment."""
    pts = as_points(points)
    seg = np.asarray(seg_start, dtype=np.int64)
    if quantum is None:
        ext = max((float(np.ptp(pts[a:b], axis=0).max()) for a, b in zip(seg[:-1], seg[1:]) if b > a), default=0.0)
        from .mesh_processing import _quantum_for
        quantum = _quantum_for(ext)
    scaled = np.rint(pts / quantum)
    if scaled.size and np.abs(scaled).max() >= 2.0 ** 31:
        scaled -= np.floor(scaled.min(axis=0))
    if scaled.size and np.abs(scaled).max() >= 2.0 ** 31:
        raise ValueError("quantum is too small for these coordinates")
    ijk = scaled.astype(np.int32)
    r = hip.convex_hull(ijk, seg, max_tests=max_tests, device=device)
    out = []
    for s, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        t = r.tris[r.tri_ptr[s]:r.tri_ptr[s + 1]] - np.int32(a)
        out.append(ConvexHull(pts[a:b], ijk[a:b], t, r.dim[s], quantum, np.zeros(3), r.stats))
    return out


class AlphaShape:
    """One cloud's alpha shape (``hip.alpha_shape3``). ``triangles`` int32 [T, 3]: the
    smallest index first, ascending; regular ones (``kinds`` 1) are oriented out of the solid, singular ones
    (``kinds`` 2, only with ``faces="all"``) are sheets with ``b < c`` and no part of volume or area.
    ``vertices``: ascending indices of the points some triangle uses; ``six_volume``: Python int in lattice
    units^3; ``volume`` / ``area`` (of the regular triangles) in the points' units. ``n_unresolved_ties``:
    triangles kept although a point off their plane lies exactly on their empty ball; the surface may then
    fail to close, and ``volume`` means something only when it is 0. ``quantum`` / ``rho2``: the lattice and
    the squared radius on it; ``stats``: the call's counters."""

    def __init__(self, points, ijk, rows, six_volume, quantum, rho2, n_unresolved_ties, stats=None):
        self.points = points
        self.ijk = ijk
        self.triangles = np.ascontiguousarray(rows[:, :3])
        self.kinds = np.ascontiguousarray(rows[:, 3])
        self.quantum = float(quantum)
        self.rho2 = int(rho2)
        self.n_unresolved_ties = int(n_unresolved_ties)
        self.stats = stats or {}
        self.vertices = np.unique(self.triangles).astype(np.int64)
        self.six_volume = int(six_volume)
        self.volume = self.six_volume / 6.0 * self.quantum ** 3
        regular = self.triangles[self.kinds == hip.ALPHA3_REGULAR]
        nrm = twice_area_normals(ijk, regular) if len(regular) else np.zeros((0, 3), np.int64)
        n2 = [int(x) * int(x) + int(y) * int(y) + int(z) * int(z) for x, y, z in nrm]     # in row order
        self.area = 0.5 * self.quantum ** 2 * float(sum(np.sqrt(float(v)) for v in n2))

    def to_mesh(self) -> TriangleMesh:
        """The regular triangles as a mesh over ALL the points (indices unchanged)."""
        return TriangleMesh(self.points, self.triangles[self.kinds == hip.ALPHA3_REGULAR])


def snap_for_radius(pts, radius, quantum=None):
    """``(lattice int32 [n,3], quantum, rho2)`` for a ball of ``radius``: ball pivoting's rule (DESIGN section
    19). The quantum is a power of two, by default the larger of ``quantize_mesh``'s (extent / 2^20) and the
    smallest at which the radius is at most 2^11 lattice units; ``rho2 = floor((radius / quantum)^2)``. A given
    quantum that does not fit is refused with the one that would."""
    import math
    from .mesh_processing import _check_quantum, _quantum_for
    radius = float(radius)
    if not np.isfinite(radius) or radius <= 0:
        raise ValueError("alpha must be positive and finite")
    if not np.isfinite(pts).all():
        raise ValueError("point coordinates must be finite")
    max_rho = float(1 << 11)
    m, e = math.frexp(radius / max_rho)                  # the smallest power of two >= radius / 2^11
    q_fit = math.ldexp(1.0, e - 1 if m == 0.5 else e)
    if quantum is None:
        ext = float((pts.max(axis=0) - pts.min(axis=0)).max()) if len(pts) else 0.0
        q = max(_quantum_for(ext), q_fit)
    else:
        q = _check_quantum(quantum)
        if radius / q > max_rho:
            raise ValueError(f"alpha {radius!r} is {radius / q:.0f} lattice units at quantum {q!r}, more than 2^11: "
                             f"a quantum of {q_fit!r} would fit")
    rho2 = int(np.floor((radius / q) ** 2))
    if rho2 < 1:
        raise ValueError(f"alpha {radius!r} is below the quantum {q!r}")
    scaled = np.rint(pts / q)
    if len(pts) and np.abs(scaled).max() >= 2.0 ** 62:
        raise ValueError("quantum is too small for these coordinates")
    lat = scaled.astype(np.int64)
    if len(pts):
        lat -= lat.min(axis=0)
        if lat.max() >= 1 << 31:
            raise ValueError(f"the cloud spans {int(lat.max())} lattice units at quantum {q!r}, more than 2^31: "
                             "use a larger quantum")
    return lat.astype(np.int32), q, rho2


def alpha_shapes(points, seg_start, alpha, quantum=None, faces="regular", device: int = 0, max_tests=None) -> list:
    """One :class:`AlphaShape` per segment ``points[seg_start[s]:seg_start[s + 1]]`` from a single call on
    one lattice: a stand of trees gets its crown volumes at once. A triangle and the points that block it
    belong to one segment; the triangles of each shape index into its own segment."""
    pts = as_points(points)
    seg = np.asarray(seg_start, dtype=np.int64)
    ijk, q, rho2 = snap_for_radius(pts, alpha, quantum)
    r = hip.alpha_shape3(ijk, rho2, seg_start=seg, faces=faces, max_tests=max_tests, device=device)
    first = np.searchsorted(r.rows[:, 0], seg)          # rows ascend by a: grouped by segment
    out = []
    for s, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        rows = r.rows[first[s]:first[s + 1]].copy()
        rows[:, :3] -= np.int32(a)
        # the tie counter is the call's, not kept per segment: every shape of the call carries it
        out.append(AlphaShape(pts[a:b], ijk[a:b], rows, r.vol6[s], q, rho2, r.stats["unresolved_ties"], r.stats))
    return out


def alpha_shape(points, alpha, quantum=None, faces="regular", device: int = 0, max_tests=None) -> AlphaShape:
    """The 3-D alpha shape of ``points`` ([n, 3], or anything with ``.points``) on the GPU at radius ``alpha``
    (the points' units), exact for the points snapped to the lattice (:func:`snap_for_radius`): by a contract
    of its own, NOT Open3D's triangle list, with which parity is unverified."""
    pts = as_points(points)
    return alpha_shapes(pts, np.array([0, len(pts)], np.int64), alpha, quantum, faces, device, max_tests)[0]


def pca_frame(hull_pts):
    """Open3D's oriented box of a set of hull vertices: ``(mean, R, lo, hi)`` with the mean and the
    biased covariance of the vertices, the eigenvectors by descending eigenvalue as R's columns,
    ``R[:, 0] = R[:, 1] x R[:, 2]``, and the extent [lo, hi] of the vertices in that frame."""
    mean = hull_pts.mean(axis=0)
    cov = np.cov((hull_pts - mean).T, bias=True)
    w, v = np.linalg.eigh(cov)
    R = v[:, np.argsort(w)[::-1]]
    R[:, 0] = np.cross(R[:, 1], R[:, 2])
    local = (hull_pts - mean) @ R
    return mean, R, local.min(axis=0), local.max(axis=0)


def frame_corners(mean, R, lo, hi):
    """The 8 corners of the box [lo, hi] of the frame (mean, R)."""
    return np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1])
                     for z in (lo[2], hi[2])]) @ R.T + mean


class OrientedBoundingBox:
    """Open3D's ``OrientedBoundingBox``: ``center``, ``R`` (columns are the box axes) and ``extent``
    (full side lengths)."""

    def __init__(self, center=(0.0, 0.0, 0.0), R=None, extent=(0.0, 0.0, 0.0)):
        self.center = np.array(center, dtype=np.float64)
        self.R = np.eye(3) if R is None else np.array(R, dtype=np.float64)
        self.extent = np.array(extent, dtype=np.float64)
        self.color = (0.0, 0.0, 0.0)
        self._corners = None      # the corners as built from the hull, until the box is moved

    @classmethod
    def create_from_points(cls, points, quantum=None, device: int = 0) -> "OrientedBoundingBox":
        """The PCA box of the convex hull's vertices (the hull on the GPU). A cloud without a 3-D
        hull gets the PCA box of all its points."""
        pts = as_points(points)
        h = convex_hull(pts, quantum=quantum, device=device)
        hull_pts = pts[h.vertices] if h.dim == 3 else pts
        return cls.from_hull_points(hull_pts)

    @classmethod
    def from_hull_points(cls, hull_pts) -> "OrientedBoundingBox":
        mean, R, lo, hi = pca_frame(np.asarray(hull_pts, dtype=np.float64))
        box = cls(mean + R @ (0.5 * (lo + hi)), R, hi - lo)
        box._corners = frame_corners(mean, R, lo, hi)
        return box

    def __repr__(self):
        return f"OrientedBoundingBox: center: {self.center}, extent: {self.extent}"

    def get_box_points(self) -> np.ndarray:
        if self._corners is not None:
            return self._corners.copy()
        h = 0.5 * self.extent
        return np.array([[x, y, z] for x in (-h[0], h[0]) for y in (-h[1], h[1])
                         for z in (-h[2], h[2])]) @ self.R.T + self.center

    def get_min_bound(self) -> np.ndarray:
        return self.get_box_points().min(axis=0)

    def get_max_bound(self) -> np.ndarray:
        return self.get_box_points().max(axis=0)

    def get_center(self) -> np.ndarray:
        return self.center.copy()

    def volume(self) -> float:
        return float(np.prod(self.extent))

    def translate(self, translation, relative: bool = True) -> "OrientedBoundingBox":
        t = np.asarray(translation, dtype=np.float64)
        self.center = self.center + t if relative else t.copy()
        self._corners = None
        return self

    def scale(self, scale: float, center) -> "OrientedBoundingBox":
        c = np.asarray(center, dtype=np.float64)
        self.center = c + float(scale) * (self.center - c)
        self.extent = self.extent * float(scale)
        self._corners = None
        return self

    def as_row(self) -> np.ndarray:
        """The 15 doubles ``pyqsm_points_in_boxes`` takes: centre, R row-major, half-extent."""
        return np.concatenate([self.center, self.R.reshape(-1), 0.5 * self.extent])

    def get_point_indices_within_bounding_box(self, points, device: int = 0) -> np.ndarray:
        """Indices (ascending) of the points inside the box, bounds inclusive; ``points`` [n, 3],
        anything with ``.points`` or a ``hip.DeviceBuffer`` of a cloud already in HBM."""
        src = points if isinstance(points, hip.DeviceBuffer) else as_points(points)
        _, idx = hip.points_in_boxes(src, self.as_row()[None, :], device=device)
        return idx


def point_indices_within_boxes(points, boxes, device: int = 0) -> list:
    """``get_point_indices_within_bounding_box`` of many boxes against one cloud in one pass per 256
    boxes: a list of index arrays, one per box."""
    src = points if isinstance(points, hip.DeviceBuffer) else as_points(points)
    rows = np.array([b.as_row() for b in boxes], dtype=np.float64).reshape(-1, 15)
    ptr, idx = hip.points_in_boxes(src, rows, device=device)
    return [idx[ptr[k]:ptr[k + 1]] for k in range(len(boxes))]
