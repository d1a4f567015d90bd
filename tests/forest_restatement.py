"""NumPy restatement of the tree-ensemble inference contract (include/pyqsm_hip.h, "tree-ensemble
inference"). It is scikit-learn's own arithmetic (tree/_tree.pyx ``_apply_dense``,
``ForestClassifier.predict_proba`` with ``n_jobs=1``), so tests/test_forest_host.py holds it to a
live scikit-learn and to tests/golden/forest_small.npz bit for bit.

* X is cast to float32; NaN is a value, +-inf is an error of the caller.
* Per tree from the root (node 0): at an internal node with feature f, threshold t (float64) and
  missing_go_to_left m, a NaN x[f] goes left iff m; otherwise left iff float64(x[f]) <= t. A node
  with children_left == -1 is a leaf. ``apply`` [n, T] is the leaf's node number within its tree.
* ``predict_proba``: acc = 0 (float64 [n, C]); for the trees in estimator order acc += value[leaf];
  then acc / T. The order of the additions is part of the contract.
* ``predict_index``: the first maximum of predict_proba (np.argmax).

A tree is (left, right, feature, threshold, missing_left, value [nodes, C]).
"""
from __future__ import annotations

import numpy as np


def trees_of(model):
    """The trees of a fitted scikit-learn classifier (forest or single tree) as plain arrays."""
    ests = getattr(model, "estimators_", None)
    trees = [model.tree_] if ests is None else [e.tree_ for e in ests]
    C = len(model.classes_)
    return [(np.asarray(t.children_left), np.asarray(t.children_right), np.asarray(t.feature),
             np.asarray(t.threshold), np.asarray(t.missing_go_to_left).astype(np.uint8),
             np.asarray(t.value)[:, 0, :C].astype(np.float64)) for t in trees]


def apply_tree(tree, X32, wide_compare=True, t32=None):
    """Leaf node numbers [n] of one tree. ``wide_compare``: float64(x) <= t as scikit-learn;
    otherwise x <= t32 in float32 (the device's record; t32 from :func:`floor_f32`)."""
    left, right, feature, threshold, missing_left, _ = tree
    n = X32.shape[0]
    node = np.zeros(n, dtype=np.int64)
    rows = np.arange(n)
    active = left[node] != -1
    while active.any():
        r = rows[active]
        nd = node[r]
        x = X32[r, feature[nd]]
        if wide_compare:
            le = x.astype(np.float64) <= threshold[nd]
        else:
            le = x <= t32[nd]
        go_left = np.where(np.isnan(x), missing_left[nd] != 0, le)
        node[r] = np.where(go_left, left[nd], right[nd])
        active = left[node] != -1
    return node


def apply(trees, X):
    X32 = np.ascontiguousarray(X, dtype=np.float32)
    return np.stack([apply_tree(t, X32) for t in trees], axis=1)


def predict_proba(trees, X, leaves=None):
    leaves = apply(trees, X) if leaves is None else leaves
    acc = np.zeros((leaves.shape[0], trees[0][5].shape[1]), dtype=np.float64)
    for k, t in enumerate(trees):
        acc += t[5][leaves[:, k]]
    return acc / len(trees)


def predict_index(trees, X, proba=None):
    proba = predict_proba(trees, X) if proba is None else proba
    return np.argmax(proba, axis=1)


def floor_f32(threshold):
    """The largest float32 not above each float64 threshold."""
    t = np.asarray(threshold, dtype=np.float64)
    with np.errstate(over="ignore"):
        f = t.astype(np.float32)
    above = f.astype(np.float64) > t
    return np.where(above, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def max_depth(tree):
    left, right = tree[0], tree[1]
    depth = np.zeros(len(left), dtype=np.int64)
    best, stack = 0, [0]
    while stack:
        i = stack.pop()
        if left[i] == -1:
            best = max(best, int(depth[i]))
            continue
        depth[left[i]] = depth[right[i]] = depth[i] + 1
        stack += [int(left[i]), int(right[i])]
    return best


def chain_tree(depth, n_features, n_classes, seed=0, margin=3.5):
    """A degenerate tree: a chain of ``depth`` internal nodes, each with one leaf child and the
    next link, sides alternating at random; random features, thresholds and leaf distributions."""
    rng = np.random.default_rng(seed)
    m = 2 * depth + 1
    left = np.full(m, -1, np.int64)
    right = np.full(m, -1, np.int64)
    feature = np.full(m, -2, np.int64)
    threshold = np.full(m, -2.0)
    missing = np.zeros(m, np.uint8)
    value = rng.dirichlet(np.ones(n_classes), size=m)
    for d in range(depth):           # internal node 2d; leaf 2d + 1; next link 2d + 2
        i, leaf, nxt = 2 * d, 2 * d + 1, 2 * d + 2
        if rng.random() < 0.5:
            left[i], right[i] = leaf, nxt
        else:
            left[i], right[i] = nxt, leaf
        feature[i] = rng.integers(n_features)
        # standard normal rows leave the chain at about 0.7 % per level at margin 3.5 (half reach
        # depth 100), at 0.02 % at margin 5
        threshold[i] = float(np.float32(rng.normal())) + (margin if left[i] == nxt else -margin)
        missing[i] = rng.integers(2)
    return left, right, feature, threshold, missing, value


def gaussian_classes(n, n_features, n_classes, seed=0, spread=1.0):
    """Overlapping Gaussian classes: float32 rows [n, F] and labels [n]; class centres drawn at
    ``spread`` standard deviations, so neighbouring classes overlap and forests tie on some rows."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, spread, (n_classes, n_features))
    y = rng.integers(n_classes, size=n)
    X = (centres[y] + rng.normal(size=(n, n_features))).astype(np.float32)
    return X, y
