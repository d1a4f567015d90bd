"""The radius graph of a cloud: degrees (local density) and pair list.

Vertices are the points, an edge joins two points within ``r`` of each other (d2 <= r*r in fp64,
inclusive, coincident points joined: cKDTree's rule). pyQSM builds it with
``KDTree.query_pairs`` and a Python loop over the pairs (``utils/lib_integration.get_pairs``),
and splits a branch cloud into wood and leaf at a percentile of the degree
(``scripts/graph_based_leaf_id.py:28-38``). Here the degrees come from one pass in O(n) memory
(``hip.radius_degrees``), the pair list only when asked for. The connected components of the graph
are ``hip.dbscan(points, r, 1)``'s clusters; ranking them by size is not part of this module.
"""
from __future__ import annotations

import numpy as np

from .cloud import _hip, as_points


class RadiusGraph:
    """What :func:`radius_graph` returns: ``radii`` float64 [R]; ``degree`` int32 [R, n]; ``n_pairs``
    int64 [R]."""

    def __init__(self, points, radii, degree, n_pairs, device):
        self.points = points
        self.radii = radii
        self.degree = degree
        self.n_pairs = n_pairs
        self._device = device
        self._pairs = {}

    def pairs(self, k: int = 0) -> np.ndarray:
        """int32 [n_pairs[k], 2]: the edges at ``radii[k]``, i < j, ascending by (i, j); fetched on
        first use."""
        k = int(k)
        if k not in self._pairs:
            self._pairs[k] = _hip().radius_pairs(self.points, float(self.radii[k]), int(self.n_pairs[k]),
                                                 device=self._device)
        return self._pairs[k]


def radius_graph(points, radii, device: int = 0) -> RadiusGraph:
    """The radius graph of ``points`` at every radius of ``radii`` (a scalar or up to 8 values, any
    order): all degrees in one call."""
    pts = as_points(points)
    rr = np.atleast_1d(np.asarray(radii, dtype=np.float64))
    degree, n_pairs = _hip().radius_degrees(pts, rr, device=device)
    return RadiusGraph(pts, rr, degree, n_pairs, device)


def degree_split(points, radius: float = .3, pct: float = 30, device: int = 0):
    """``(low_idxs, high_idxs, degrees)``: the points whose degree at ``radius`` lies below the
    ``pct``-th percentile of the degrees, the others, and the degrees (int32 [n]); the wood / leaf
    split of ``graph_based_leaf_id.py:28-38``. The percentile is NumPy's, on the host."""
    degrees = _hip().radius_degrees(as_points(points), [float(radius)], device=device)[0][0]
    if len(degrees) == 0:
        empty = np.zeros(0, dtype=np.int64)
        return empty, empty.copy(), degrees
    cut = np.percentile(degrees, pct)
    return np.where(degrees < cut)[0], np.where(degrees >= cut)[0], degrees

