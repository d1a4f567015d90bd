"""Which clusters lie next to which — the compute core of ``pyQSM/cluster_joining.py:84-164``
(``create_kdtrees``, ``determine_adjacency``) and the ranking step its callers repeat
(``join_clusters`` ``:457-459``, ``compare_skio_clusters_to_tl_clusters`` ``:596-598``).

The reference visits every (source cluster, candidate cluster) pair in a Python loop, asks SciPy
for ``tree_i.sparse_distance_matrix(tree_j, threshold)`` and keeps the minimum; to make that
bearable it keeps only every tenth point of each cluster. Here all clusters go through ONE GPU call
(``pyqsm_cluster_adjacency``: the targets binned once, one lane per source point, the results in a
cluster-by-cluster table), which also makes the unsampled form affordable.

Not restated: the interactive and drawing parts of the reference module (``loop_and_ask``,
``user_cluster``, ``join_clusters`` …), its hard-wired data directory and the pickles it writes on
the way. Those names fall through to pyQSM's own module when it is on the path.
"""
from __future__ import annotations

import os
import pickle

import numpy as np

try:  # flat import style of the reference (pyqsm_amd on sys.path) or package import
    from . import hip
    from ._shadow import fall_through
    from .geometry.cloud import as_points
except ImportError:  # pragma: no cover
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyqsm_amd import hip
    from pyqsm_amd._shadow import fall_through
    from pyqsm_amd.geometry.cloud import as_points

# names pyQSM's module of the same name defines and this one does not (pyqsm_amd/_shadow.py)
__getattr__ = fall_through(__name__)


def _cluster_points(x) -> np.ndarray:
    """The points of a ``kdtrees`` entry: a cKDTree / KDTree (``.data``), an [k,3] array or a cloud."""
    data = getattr(x, "data", None)
    if data is not None and hasattr(x, "query"):
        x = np.asarray(data)
    return np.ascontiguousarray(as_points(x), dtype=np.float64).reshape(-1, 3)


def _unique_labels(pairs, what):
    labels = [label for label, _ in pairs]
    if len(set(labels)) != len(labels):
        raise ValueError(f"duplicate labels in {what}")
    return labels


def create_kdtrees(coords, labels, case_name='', sample_every=10):
    """cluster_joining.py:84-97: ``[(label, points of that label[::sample_every])]`` for every
    label of ``np.unique(labels)``, in that order — the reference's sampling, as plain point arrays
    (``determine_adjacency`` needs no KD-tree). ``sample_every=1`` keeps every point: the exact
    form, which one GPU pass over all points makes affordable. ``case_name`` is accepted and
    ignored: no files are written."""
    coords = np.asarray(as_points(coords))
    labels = np.asarray(labels).reshape(-1)
    if labels.shape[0] != coords.shape[0]:
        raise ValueError("one label per point")
    step = int(sample_every)
    if step < 1:
        raise ValueError("sample_every must be >= 1")
    return [(label, coords[labels == label][::step]) for label in np.unique(labels)]


def determine_adjacency(label_list, kdtrees=None, threshold=0.35, case_name='', src_kdtrees=None,
                        save=False, device: int = 0):
    """cluster_joining.py:126-164. ``kdtrees`` and ``src_kdtrees`` (default: ``kdtrees``) are
    ``[(label, X)]`` with X a cKDTree, an [k,3] array or a cloud. Returns
    ``{int(label_i): {int(label_j): float(min_dist)}}``: a key for every ``label_i`` of
    ``src_kdtrees`` that is in ``label_list`` (an empty dict when nothing is near); the inner keys
    are the labels of ``kdtrees`` that are not in ``label_list`` (so never ``label_i``), not 0, and have
    a point within ``threshold`` (inclusive) of cluster i, in the order of ``kdtrees``;
    ``min_dist`` is the smallest point-to-point distance, the value
    ``sparse_distance_matrix(...)['v'].min()`` has. All pairs are evaluated by one GPU call.

    Side effects: none unless ``save=True``, which pickles the dict to ``adj.pkl`` (or
    ``adj_<case_name>.pkl``) in the current directory; the reference always writes it, below its
    hard-wired data directory."""
    if kdtrees is None:
        raise ValueError("kdtrees is required")
    if src_kdtrees is None:
        src_kdtrees = kdtrees
    wanted = set(label_list)
    src_labels = _unique_labels(src_kdtrees, "src_kdtrees")
    tgt_labels = _unique_labels(kdtrees, "kdtrees")
    src = [(k, _cluster_points(x)) for k, (label, x) in enumerate(src_kdtrees) if label in wanted]
    tgt = [(k, _cluster_points(x)) for k, (label, x) in enumerate(kdtrees)
           if not (label in wanted or label == 0)]
    adjacency_dict = {int(src_labels[k]): {} for k, _ in src}
    if src and tgt:
        # cluster = position in its list: rows come back ordered by (source, target) position
        res = hip.cluster_adjacency(
            np.concatenate([p for _, p in src]),
            np.concatenate([np.full(len(p), k, dtype=np.int64) for k, p in src]), float(threshold),
            targets=np.concatenate([p for _, p in tgt]),
            target_labels=np.concatenate([np.full(len(p), k, dtype=np.int64) for k, p in tgt]), device=device)
        for i, j, dist in zip(res.a, res.b, res.dist):
            adjacency_dict[int(src_labels[int(i)])][int(tgt_labels[int(j)])] = float(dist)
    if save:
        file_name = f'adj_{case_name}.pkl' if case_name != '' else 'adj.pkl'
        with open(file_name, 'wb') as f:
            pickle.dump(adjacency_dict, f)
    return adjacency_dict


def closest_clusters(adj, label, num_closest):
    """The ``num_closest`` nearest neighbours of ``label`` in an adjacency dict, nearest first: the
    ``np.array(dists).argsort()[:num_closest]`` step of cluster_joining.py:457-459 and :596-598.
    An array of labels; empty when the cluster has no neighbour or is unknown."""
    closest_list = adj.get(label)
    if not closest_list:
        return np.zeros(0, dtype=np.int64)
    adj_labels, dists = zip(*closest_list.items())
    low_dist_idxs = np.array(dists).argsort()[:num_closest]
    return np.array(adj_labels)[low_dist_idxs]


def cluster_adjacency_graph(pcd_or_points, labels, threshold=0.35, return_pairs=False, device: int = 0):
    """The adjacency of ONE labelled cloud — DBSCAN's output, say — with itself: every pair of
    clusters a < b with a point pair within ``threshold``, as ``hip.ClusterAdjacency`` (a, b, dist,
    n_pairs and, with ``return_pairs``, the closest point pair's indices). Negative labels (noise)
    are ignored."""
    return hip.cluster_adjacency(as_points(pcd_or_points), labels, float(threshold), return_pairs=return_pairs,
                                 device=device)
