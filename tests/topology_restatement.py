"""NumPy / SciPy statement of what csrc/topology.hip computes: the spanning forest of
the kNN graph, the degree-2 chain collapse, the chain radii and the sampled cylinder surfaces. No
GPU, no package code except the helpers `skeleton_to_QSM` itself uses."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components, minimum_spanning_tree
from scipy.spatial import cKDTree


def knn_graph(points, k):
    """Directed kNN entries (rows, cols, distance) with the point itself excluded; exact duplicates
    of a point are listed at distance 0."""
    P = np.asarray(points, dtype=np.float64)
    n = len(P)
    kk = min(int(k), n - 1)
    if kk < 1:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    d, j = cKDTree(P).query(P, k=kk + 1)
    rows, cols, dist = [], [], []
    for i in range(n):
        others = [(dd, jj) for dd, jj in zip(d[i], j[i]) if jj != i][:kk]
        for dd, jj in others:
            rows.append(i)
            cols.append(jj)
            dist.append(dd)
    return np.array(rows, np.int64), np.array(cols, np.int64), np.array(dist)


def forest_from_entries(rows, cols, dist, n):
    """`minimum_spanning_tree` of the entries: edges [e,2] with a < b, rows ascending, and their
    weights. SciPy unites components across explicit zeros but never lists them (its result matrix
    reads weight 0 as "no entry"): the convention `extract_skeletal_graph` has, and the contract."""
    g = csr_matrix((dist, (rows, cols)), shape=(n, n))
    mst = minimum_spanning_tree(g).tocoo()
    a, b = np.minimum(mst.row, mst.col), np.maximum(mst.row, mst.col)
    order = np.lexsort((b, a))
    return np.stack([a[order], b[order]], axis=1).astype(np.int32).reshape(-1, 2), mst.data[order]


def skeletal_forest(points, k):
    rows, cols, dist = knn_graph(points, k)
    return forest_from_entries(rows, cols, dist, len(points))


def n_components(edges, n):
    e = np.asarray(edges).reshape(-1, 2)
    g = csr_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    return connected_components(g, directed=False)[0]


def collapse_chains(edges, n_nodes):
    """Plain-Python chain walk. Raises ValueError for an edge list that is not a forest."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    m = int(n_nodes)
    if len(e) and (e.min() < 0 or e.max() >= m or (e[:, 0] == e[:, 1]).any()):
        raise ValueError("an edge names a node outside [0, n_nodes) or joins a node to itself")
    if len(e) != (m - n_components(e, m) if m else 0):
        raise ValueError("the edge list is not a forest")
    nbrs = [[] for _ in range(m)]
    for a, b in e.tolist():
        nbrs[a].append(b)
        nbrs[b].append(a)
    kept = [v for v in range(m) if len(nbrs[v]) != 2]
    kept_set = set(kept)
    chains = []
    for u in kept:
        for w in nbrs[u]:
            prev, cur, run = u, w, []
            for _ in range(m):
                if cur in kept_set:
                    break
                run.append(cur)
                n0, n1 = nbrs[cur]
                prev, cur = cur, (n1 if n0 == prev else n0)
            else:
                raise ValueError("a walk met no end: the edge list is not a forest")
            if u < cur:
                chains.append((u, cur, run))
    chains.sort(key=lambda c: (c[0], c[1]))
    ends = np.array([(a, b) for a, b, _ in chains], dtype=np.int32).reshape(-1, 2)
    ptr = np.concatenate([[0], np.cumsum([len(r) for _, _, r in chains])]).astype(np.int64)
    members = np.array([v for _, _, r in chains for v in r], dtype=np.int32)
    return np.array(kept, dtype=np.int32), ends, ptr, members


def chain_radii(shift, chain_ptr, members, index_map=None):
    dist = np.linalg.norm(np.asarray(shift, dtype=np.float64), axis=1)
    out = np.zeros(len(chain_ptr) - 1)
    for c in range(len(out)):
        mem = np.asarray(members[chain_ptr[c]:chain_ptr[c + 1]], dtype=np.int64)
        if len(mem):
            out[c] = np.mean(dist[mem] if index_map is None else dist[np.asarray(index_map)[mem]])
    return out


def cylinder_surface(center, axis_unit, u, v, radius, height):
    """The sampling of `skeleton_to_QSM` for one cylinder."""
    from pyqsm_amd.geometry.skeletonize import _unique_rows_mm
    ang = np.linspace(0.0, 2.0 * np.pi, 20, endpoint=False)
    along = np.linspace(-height / 2.0, height / 2.0, 100)
    ring = radius * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * v)
    pts = (center + ring[None, :, :] + along[:, None, None] * axis_unit).reshape(-1, 3)
    return _unique_rows_mm(pts.round(3))
