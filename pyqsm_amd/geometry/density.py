"""The radius graph of a cloud: degrees (local density) and pair list.

Vertices are the points, an edge joins two points within ``r`` of each other (d2 <= r*r in fp64,
inclusive, coincident points joined: cKDTree's rule). pyQSM builds it with
``KDTree.query_pairs`` and a Python loop over the pairs (``utils/lib_integration.get_pairs``),
and splits a branch cloud into wood and leaf at a percentile of the degree
(``scripts/graph_based_leaf_id.py:28-38``). Here the degrees come from one pass in O(n) memory
(``hip.radius_degrees``), the pair list only when asked for. The connected components ranked by
size, which pyQSM takes from rustworkx over the pair list
(``sorted(connected_components(g), key=len, reverse=True)``, ``graph_based_leaf_id.py:80-97``,
``qsm_generation.exclude_dense_areas``), come from ``hip.radius_components`` without a pair list:
:class:`Components`, :meth:`RadiusGraph.components`, :func:`dense_components`.
"""
from __future__ import annotations

import numpy as np

from .cloud import _hip, as_points


class Components:
    """The connected components of a radius graph, ranked by (size descending, smallest member
    ascending): ``component`` int32 [n], the rank of every point's component; ``sizes`` int32 [c],
    non-increasing. pyQSM's ``conn_comps[k]`` is ``members(k)``, as ascending point indices."""

    def __init__(self, component, sizes, members=None):
        self.component = np.asarray(component)
        self.sizes = np.asarray(sizes)
        self._members = members       # the point indices ascending by (component, index)
        self._offsets = None

    def __len__(self) -> int:
        return len(self.sizes)

    def _order(self):
        if self._members is None:
            self._members = np.lexsort((np.arange(len(self.component)), self.component))
        if self._offsets is None:
            self._offsets = np.concatenate([[0], np.cumsum(self.sizes, dtype=np.int64)])
        return self._members, self._offsets

    def members(self, rank: int) -> np.ndarray:
        """The point indices of the component of rank ``rank``, ascending."""
        rank = int(rank)
        if not 0 <= rank < len(self.sizes):
            raise IndexError(f"rank {rank} of {len(self.sizes)} components")
        order, off = self._order()
        return order[off[rank]:off[rank + 1]]

    def select(self, top=None, min_size=None, max_size=None) -> np.ndarray:
        """The point indices of the chosen components, concatenated in rank order: pyQSM's
        ``chain.from_iterable(x for x in conn_comps[0:top] if min_size < len(x) < max_size)``, both
        bounds strict, a bound of None not applied."""
        order, off = self._order()
        head = self.sizes[:top]
        keep = np.ones(len(head), dtype=bool)
        if min_size is not None:
            keep &= head > min_size
        if max_size is not None:
            keep &= head < max_size
        if not keep.any():
            return order[:0]
        return np.concatenate([order[off[s]:off[s + 1]] for s in np.flatnonzero(keep)])


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
        self._components = {}

    def components(self, k: int = 0) -> Components:
        """The components at ``radii[k]`` ranked by size; fetched on first use."""
        k = int(k)
        if k not in self._components:
            comp, sizes, mem = _hip().radius_components(self.points, [float(self.radii[k])], device=self._device,
                                                        members=True)
            self._components[k] = Components(comp[0], sizes[0], mem[0])
        return self._components[k]

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


def dense_components(points, radii=(.06, .07, .08, .09), top: int = 500, min_size: int = 100, device: int = 0):
    """The radius sweep of ``graph_based_leaf_id.py:80-97`` as one call: a list with one
    :class:`Components` per radius of ``radii`` (up to 8), each with ``large`` set to its
    ``large_comp_pt_ids``, ``select(top=top, min_size=min_size)``: the points of those of the ``top``
    largest components that hold more than ``min_size`` points."""
    rr = np.atleast_1d(np.asarray(radii, dtype=np.float64))
    comp, sizes, mem = _hip().radius_components(as_points(points), rr, device=device, members=True)
    out = []
    for k in range(len(rr)):
        c = Components(comp[k], sizes[k], mem[k])
        c.large = c.select(top=top, min_size=min_size)
        out.append(c)
    return out


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

