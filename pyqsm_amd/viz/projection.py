"""Projected area on the GPU: what pyQSM's ``viz.ray_casting.project_pcd(...).area`` reports, as the
exact area of a 2-D alpha shape (``hip.alpha_area``).

    quantize_plane(points, normal, origin, quantum)        project and snap to an integer lattice
    projected_area(points, alpha, ...)                     one cloud -> AlphaShape
    projected_area_batch(points, seg_start | labels, ...)  many clouds, one device call
    project_pcd(point_cloud, pts, alpha, ...)              pyQSM's signature, returns the AlphaShape
    project_in_slices(pcd, seed, ...)                      canopy_metrics.project_in_slices
    project_by_label(points, labels, alpha, every)         project_components_in_clusters after its
                                                           clustering

pyQSM has no module of this name, so nothing is shadowed: ``viz.ray_casting.project_pcd`` and all
of ``canopy_metrics`` keep resolving to pyQSM's own files (tests/test_dropin.py); INTEGRATION.md
has the one-line edit that points ``canopy_metrics`` here.

Differences from the reference, all deliberate:

* The points are snapped to a lattice of pitch ``quantum`` (a power of two, about 0.03 mm for a
  30 m crown) and points that share a lattice node are merged; VTK merges by its own tolerance.
* A cell of the Delaunay subdivision is kept iff its circumradius^2 <= floor((alpha / quantum)^2)
  lattice units, decided with integers; VTK's incremental Delaunay decides in floating point and is
  neither robust nor reproducible. Cocircular points form one cell, so the result is unique.
* There is no triangle list: the result carries the area, the boundary edges and the perimeter.
* ``alpha`` must be positive. VTK's ``alpha = 0`` (no filter, the whole hull) is out of scope.
* Nothing is plotted and no file is written.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from .. import hip

MAX_EXTENT = hip.ALPHA_MAX_EXTENT


class AlphaShape:
    """The alpha shape of one projected cloud.

    area          twice_area_q * quantum^2 / 2, in the units of the points squared (fp64)
    twice_area_q  twice the area in lattice units^2 (exact integer)
    quantum       the lattice pitch
    n_points      points that took part, after merging those that share a lattice node
    boundary      int64 [r, 2] directed boundary edges as indices into the points handed in, kept side
                  on the left, ascending by (a, b); None unless asked for
    perimeter     the summed length of the boundary edges (exactly rounded sum); None without them
    """

    def __init__(self, twice_area_q, quantum, n_points, boundary=None, ij=None):
        self.twice_area_q = int(twice_area_q)
        self.quantum = float(quantum)
        self.n_points = int(n_points)
        self.area = self.twice_area_q * self.quantum * self.quantum / 2.0
        self.boundary = boundary
        self.perimeter = None
        if boundary is not None:
            d = (ij[boundary[:, 1]] - ij[boundary[:, 0]]).astype(np.float64)
            self.perimeter = math.fsum(np.hypot(d[:, 0], d[:, 1]).tolist()) * self.quantum

    def __repr__(self):
        return f"AlphaShape(area={self.area!r}, n_points={self.n_points}, quantum={self.quantum!r})"


def _plane_coords(points, normal, origin) -> np.ndarray:
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"expected points of shape [n,3], got {pts.shape}")
    if not np.isfinite(pts).all():
        raise ValueError("point coordinates must be finite")
    nrm = np.asarray(normal, dtype=np.float64).reshape(3)
    if not np.isfinite(nrm).all() or not nrm.any():
        raise ValueError("the plane normal must be finite and non-zero")
    if nrm[0] == 0 and nrm[1] == 0:
        return pts[:, :2].copy() if nrm[2] > 0 else pts[:, 1::-1].copy()   # (x, y) itself, untouched
    nrm = nrm / np.linalg.norm(nrm)
    axis = np.zeros(3)
    axis[np.argmin(np.abs(nrm))] = 1.0
    u = np.cross(nrm, axis)
    u /= np.linalg.norm(u)
    v = np.cross(nrm, u)
    rel = pts - np.asarray(origin, dtype=np.float64).reshape(1, 3)
    return np.stack([rel @ u, rel @ v], axis=1)


def _pow2_at_least(x: float) -> float:
    """The smallest power of two >= x (x > 0)."""
    m, e = math.frexp(x)
    return math.ldexp(1.0, e - 1 if m == 0.5 else e)


def _quantum_for(extent: float) -> float:
    return _pow2_at_least(extent / MAX_EXTENT) if extent > 0 else 1.0


def _check_quantum(quantum) -> float:
    q = float(quantum)
    if not (q > 0) or not math.isfinite(q) or math.frexp(q)[0] != 0.5:
        raise ValueError("quantum must be a positive power of two")
    return q


def _segments(n: int, seg_start) -> np.ndarray:
    seg = np.array([0, n], np.int64) if seg_start is None else np.asarray(seg_start, dtype=np.int64).reshape(-1)
    if seg.size < 1 or seg[0] != 0 or seg[-1] != n or (np.diff(seg) < 0).any():
        raise ValueError("seg_start must ascend from 0 to the number of points")
    return seg


def _extent(uv: np.ndarray, seg: np.ndarray) -> float:
    ext = 0.0
    for lo, hi in zip(seg[:-1], seg[1:]):
        if hi > lo:
            ext = max(ext, float((uv[lo:hi].max(axis=0) - uv[lo:hi].min(axis=0)).max()))
    return ext


def _snap(uv: np.ndarray, seg: np.ndarray, q: float) -> np.ndarray:
    """rint(uv / q) on the absolute lattice, each segment shifted by its own minimum."""
    scaled = np.rint(uv / q)              # q is a power of two: the division is exact
    if scaled.size and np.abs(scaled).max() >= 2.0 ** 62:
        raise ValueError("quantum is too small for these coordinates")
    lat = scaled.astype(np.int64)
    for lo, hi in zip(seg[:-1], seg[1:]):
        if hi > lo:
            lat[lo:hi] -= lat[lo:hi].min(axis=0)
    if lat.size and lat.max() > MAX_EXTENT:
        raise ValueError(f"a cloud spans {int(lat.max())} lattice units at quantum {q!r}, more than 2^20: "
                         "use a larger quantum")
    return lat.astype(np.int32)


def quantize_plane(points, normal=(0, 0, 1), origin=(0, 0, 0), quantum=None, seg_start=None):
    """Project ``points`` [n,3] onto the plane through ``origin`` with ``normal`` as pyQSM's
    ``project_pcd`` does, take 2-D coordinates in a fixed orthonormal basis of the plane and snap
    them to an integer lattice. Returns ``(ij, q)``: int32 [n,2] and the lattice pitch. Host NumPy.

    For the default normal the basis is (x, y) itself: no arithmetic touches the coordinates before
    the snap. ``q`` is ``quantum`` if given (a power of two), else the smallest power of two with
    max extent / q <= 2^20: 2^-15 m, about 0.03 mm, for a 30 m crown. ``ij = rint(uv / q)`` on the
    absolute lattice, then shifted by the cloud's minimum: the scaling by a power of two is exact, so
    a cloud gets the same ``ij`` alone or as a segment of a batch (``seg_start``) with the same ``q``,
    and quantising lattice output again with the same ``q`` changes nothing."""
    uv = _plane_coords(points, normal, origin)
    seg = _segments(uv.shape[0], seg_start)
    q = _quantum_for(_extent(uv, seg)) if quantum is None else _check_quantum(quantum)
    return _snap(uv, seg, q), q


def lattice_a2(alpha, q: float) -> int:
    """A2 = floor((alpha / q)^2), exactly (rational arithmetic): the integer the kernel receives."""
    if alpha is None or not (float(alpha) > 0) or not math.isfinite(float(alpha)):
        raise ValueError("alpha must be a positive number: alpha = 0 or None (VTK's 'no alpha', the whole "
                         "convex hull) is not supported")
    return math.floor((Fraction(float(alpha)) / Fraction(q)) ** 2)


def projected_area_batch(points, seg_start=None, labels=None, alpha=None, normal=(0, 0, 1), origin=(0, 0, 0),
                         quantum=None, return_boundary=False, max_tests=None, device=0):
    """The alpha shapes of many clouds in one device call: a list of :class:`AlphaShape`.

    The clouds are the segments ``seg_start`` [n_seg + 1] of ``points``, or the points of each
    non-negative label in ascending label order (negative labels are ignored, as
    ``cluster_adjacency_graph`` does; each shape then carries ``.label``). All clouds share one
    ``quantum``: the one given, else the smallest power of two at which the largest cloud and
    ``alpha`` both span at most 2^20 lattice units. Each result equals ``projected_area`` of that
    cloud alone with the same ``quantum`` bit for bit. Boundary indices refer to ``points``."""
    if (seg_start is None) == (labels is None):
        raise ValueError("give exactly one of seg_start and labels")
    uv = _plane_coords(points, normal, origin)
    order = values = None
    if labels is not None:
        lab = np.asarray(labels).reshape(-1)
        if lab.shape[0] != uv.shape[0]:
            raise ValueError(f"one label per point: {lab.shape[0]} labels for {uv.shape[0]} points")
        if lab.size and not np.issubdtype(lab.dtype, np.integer):
            raise ValueError("labels must be integers")
        order = np.nonzero(lab >= 0)[0]
        order = order[np.argsort(lab[order], kind="stable")]
        values, counts = np.unique(lab[order], return_counts=True)
        seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        uv = uv[order]
    else:
        seg = _segments(uv.shape[0], seg_start)
    if quantum is None:
        a = float(alpha) if alpha is not None and float(alpha) > 0 and math.isfinite(float(alpha)) else 0.0
        q = _quantum_for(max(_extent(uv, seg), a))
    else:
        q = _check_quantum(quantum)
    a2 = lattice_a2(alpha, q)
    if a2 > hip.ALPHA_MAX_A2:
        raise ValueError(f"alpha = {alpha!r} is more than 2^20 lattice units at quantum {q!r}: use a larger quantum")
    ij = _snap(uv, seg, q)
    res = hip.alpha_area(ij, a2, seg_start=seg, return_boundary=return_boundary, max_tests=max_tests, device=device)
    shapes = []
    for s in range(len(seg) - 1):
        edges = None
        if return_boundary:
            edges = res.boundary(s)
        shape = AlphaShape(res.twice_area[s], q, res.n_live[s], edges, ij)
        if edges is not None and order is not None:
            shape.boundary = order[edges]
        if values is not None:
            shape.label = int(values[s])
        shapes.append(shape)
    return shapes


def projected_area(points, alpha, normal=(0, 0, 1), origin=(0, 0, 0), quantum=None, return_boundary=False,
                   max_tests=None, device=0) -> AlphaShape:
    """The alpha shape of ``points`` [n,3] projected onto a plane: its ``area`` is the total area of
    the Delaunay cells of the projected, quantised points (:func:`quantize_plane`) whose circumradius
    is at most ``alpha``, more precisely whose circumradius^2 <= A2 = floor((alpha / quantum)^2)
    lattice units, computed exactly on the GPU. ``alpha <= 0`` or None is refused.
    ``max_tests`` caps the work (``hip.alpha_area``): an alpha of many point spacings is cubic work."""
    n = np.asarray(points).shape[0]
    return projected_area_batch(points, seg_start=[0, n], alpha=alpha, normal=normal, origin=origin,
                                quantum=quantum, return_boundary=return_boundary, max_tests=max_tests,
                                device=device)[0]


def _cloud_points(cloud) -> np.ndarray:
    return np.asarray(cloud.points if hasattr(cloud, "points") else cloud, dtype=np.float64)


def project_pcd(point_cloud=None, pts=None, alpha=.1, plot=True, name='', sub_name='', seed='default',
                screen_shots=[], off_screen=False, target_dir='data/projection') -> AlphaShape:
    """pyQSM's ``viz.ray_casting.project_pcd``: project onto the ground plane and take the alpha
    shape. Returns the :class:`AlphaShape`, whose ``.area`` is what every caller reads. ``plot``,
    ``name``, ``sub_name``, ``seed``, ``screen_shots``, ``off_screen`` and ``target_dir`` are
    accepted and ignored: nothing is plotted and no file is written."""
    points = _cloud_points(point_cloud) if point_cloud is not None else np.asarray(pts, dtype=np.float64)
    return projected_area(points, alpha)


def project_in_slices(pcd, seed, name='', alpha=70, percentiles=(0, 20, 40, 60, 80, 100), every=5):
    """pyQSM's ``canopy_metrics.project_in_slices``: every ``every``-th point (Open3D's
    ``uniform_down_sample``), slices between the z percentiles (half-open, the last one closed),
    the projected area of each slice, all in one batched device call. Returns
    ``{'slice_<lo>_<hi>': {'mesh': AlphaShape, 'mesh_area': area}, ..., 'total_area': sum}``,
    the sum taken in slice order. No files are written; ``seed`` and ``name`` are ignored."""
    points = _cloud_points(pcd)[::int(every)]
    z = points[:, 2]
    edges = np.percentile(z, list(percentiles))
    parts, names = [], []
    for i in range(len(percentiles) - 1):
        lo, hi = edges[i], edges[i + 1]
        sel = (z >= lo) & ((z < hi) if i < len(percentiles) - 2 else (z <= hi))
        parts.append(points[sel])
        names.append(f'slice_{percentiles[i]}_{percentiles[i + 1]}')
    seg = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    shapes = projected_area_batch(np.concatenate(parts), seg_start=seg, alpha=alpha)
    metrics = {nm: {'mesh': sh, 'mesh_area': sh.area} for nm, sh in zip(names, shapes)}
    total = 0.0
    for sh in shapes:
        total += sh.area
    metrics['total_area'] = total
    return metrics


def project_by_label(points, labels, alpha, every=4):
    """The body of pyQSM's ``project_components_in_clusters`` after its clustering: per
    non-negative label every ``every``-th of its points, the projected area of each, in one batched
    device call. Returns ``{'areas': {label: area}, 'meshes': {label: AlphaShape}, 'total_area':
    sum in ascending label order}``. Negative labels are ignored."""
    pts = _cloud_points(points)
    lab = np.asarray(labels).reshape(-1)
    if lab.shape[0] != pts.shape[0]:
        raise ValueError(f"one label per point: {lab.shape[0]} labels for {pts.shape[0]} points")
    keep = []
    for value in np.unique(lab[lab >= 0]):
        keep.append(np.nonzero(lab == value)[0][::int(every)])
    keep = np.concatenate(keep) if keep else np.zeros(0, np.int64)
    shapes = projected_area_batch(pts[keep], labels=lab[keep], alpha=alpha) if len(keep) else []
    total = 0.0
    for sh in shapes:
        total += sh.area
    return {'areas': {sh.label: sh.area for sh in shapes}, 'meshes': {sh.label: sh for sh in shapes},
            'total_area': total}
