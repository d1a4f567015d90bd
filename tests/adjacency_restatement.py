"""CPU statements of the cluster adjacency contract, shared by the host and the
GPU tests.

``adjacency``   NumPy restatement: candidates from ``cKDTree.query_ball_point`` at a slightly larger
                radius, then the library's own fp64 predicate — d2 = ((dx*dx)+dy*dy)+dz*dz,
                d2 <= threshold*threshold — the minimum, the count and the closest point pair (ties:
                smallest source index, then smallest target index).
``scipy_loop``  what pyQSM/cluster_joining.py:139-155 does: one
                ``tree_i.sparse_distance_matrix(tree_j, threshold, output_type='ndarray')`` per
                cluster pair, its row count and the minimum of its 'v'.
Both return {(a, b): (min distance, point pairs[, source index, target index])}.
"""
import itertools

import numpy as np
from scipy.spatial import cKDTree


def block_cloud(seed=3, n=100_000, stride=5, edge=0.8):
    """The labelled test cloud: every `stride`-th point of synth.forest(n, seed), labelled by the
    index of its block of edge `edge` among the occupied blocks (np.unique order)."""
    from pyqsm_amd import synth
    P = np.ascontiguousarray(synth.forest(n, seed=seed)[::stride], dtype=np.float64)
    _, lab = np.unique(np.floor(P / edge).astype(np.int64), axis=0, return_inverse=True)
    return P, lab.reshape(-1).astype(np.int64)


def split_blocks(P, lab):
    """(source points, labels, target points, labels): labels divisible by 3 are the sources."""
    s = lab % 3 == 0
    return P[s], lab[s], P[~s], lab[~s]


def lattice():
    """arange(6)^3 * 0.25, labelled (x >= 0.75) + 2 (y >= 0.75); label 0 is the source, the rest
    are targets, plus a copy of one source point as target label 7."""
    g = np.arange(6) * 0.25
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    lab = (P[:, 0] >= 0.75).astype(np.int64) + 2 * (P[:, 1] >= 0.75)
    src, sl = P[lab == 0], lab[lab == 0]
    tgt = np.concatenate([P[lab != 0], src[0:1]])
    tl = np.concatenate([lab[lab != 0], [7]])
    return src, sl, tgt, tl


def _d2(a, b):
    t = a - b
    d = t[..., 0] * t[..., 0]
    d = d + t[..., 1] * t[..., 1]
    d = d + t[..., 2] * t[..., 2]
    return d


def adjacency(src, src_lab, tgt, tgt_lab, threshold, same_cloud=False, witness=False):
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    src_lab = np.asarray(src_lab).astype(np.int64)
    tgt_lab = np.asarray(tgt_lab).astype(np.int64)
    out = {}
    if len(src) == 0 or len(tgt) == 0:
        return out
    r2 = np.float64(threshold) * np.float64(threshold)
    cand = cKDTree(tgt).query_ball_point(src, threshold * (1.0 + 1e-9) + 1e-12, return_sorted=False)
    si = np.repeat(np.arange(len(src)), [len(c) for c in cand])
    ti = np.fromiter(itertools.chain.from_iterable(cand), dtype=np.int64, count=len(si))
    a, b = src_lab[si], tgt_lab[ti]
    keep = (a >= 0) & (b >= 0)
    if same_cloud:
        keep &= a < b
    si, ti, a, b = si[keep], ti[keep], a[keep], b[keep]
    d2 = _d2(src[si], tgt[ti])
    keep = d2 <= r2
    si, ti, a, b, d2 = si[keep], ti[keep], a[keep], b[keep], d2[keep]
    order = np.lexsort((ti, si, d2, b, a))            # by pair, then distance, source, target
    si, ti, a, b, d2 = si[order], ti[order], a[order], b[order], d2[order]
    first = np.flatnonzero(np.r_[True, (a[1:] != a[:-1]) | (b[1:] != b[:-1])]) if len(a) else np.zeros(0, int)
    counts = np.diff(np.r_[first, len(a)])
    for f, c in zip(first, counts):
        row = (float(np.sqrt(d2[f])), int(c))
        if witness:
            row += (int(si[f]), int(ti[f]))
        out[(int(a[f]), int(b[f]))] = row
    return out


def scipy_loop(src, src_lab, tgt, tgt_lab, threshold, same_cloud=False):
    src_lab, tgt_lab = np.asarray(src_lab), np.asarray(tgt_lab)
    s_trees = [(int(l), cKDTree(src[src_lab == l])) for l in np.unique(src_lab) if l >= 0]
    t_trees = [(int(l), cKDTree(tgt[tgt_lab == l])) for l in np.unique(tgt_lab) if l >= 0]
    out = {}
    for a, ta in s_trees:
        for b, tb in t_trees:
            if same_cloud and not a < b:
                continue
            m = ta.sparse_distance_matrix(tb, threshold, output_type="ndarray")
            if m.shape[0] > 0:
                out[(a, b)] = (float(m["v"].min()), int(m.shape[0]))
    return out


def as_dict(res, witness=False):
    """A pyqsm_amd.hip.ClusterAdjacency as the dict the functions above return."""
    out = {}
    for k in range(len(res.a)):
        row = (float(res.dist[k]), int(res.n_pairs[k]))
        if witness:
            row += (int(res.src_idx[k]), int(res.tgt_idx[k]))
        out[(int(res.a[k]), int(res.b[k]))] = row
    return out


def as_result(d, witness=False):
    """The dict as a ClusterAdjacency (rows ascending by (a, b)): what hip.cluster_adjacency returns."""
    from pyqsm_amd import hip
    keys = sorted(d)
    col = lambda k, dt: np.array([d[key][k] for key in keys], dtype=dt)  # noqa: E731
    return hip.ClusterAdjacency(np.array([k[0] for k in keys], np.int64), np.array([k[1] for k in keys], np.int64),
                                col(0, np.float64), col(1, np.int64),
                                col(2, np.int64) if witness else None, col(3, np.int64) if witness else None)


def restated_cluster_adjacency(points, labels, threshold, targets=None, target_labels=None, return_pairs=False,
                               max_table=1 << 26, device=0):
    """hip.cluster_adjacency's signature on the restatement (for monkeypatching the host tests)."""
    same = targets is None
    P = np.asarray(points, np.float64).reshape(-1, 3)
    d = adjacency(P, labels, P if same else targets, labels if same else target_labels, threshold,
                  same_cloud=same, witness=return_pairs)
    return as_result(d, witness=return_pairs)
