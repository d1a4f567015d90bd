"""Inference of a fitted scikit-learn tree ensemble on the HIP kernel (csrc/forest.hip, DESIGN.md
§12): the ``RandomForestClassifier`` pyQSM labels wood, leaf and epiphyte points with
(pyQSM/exploration.py:460-538). Training stays in scikit-learn on the host.

    GPUForest.from_sklearn(model)      RandomForestClassifier, ExtraTreesClassifier or a single
                                       DecisionTreeClassifier, fitted
    GPUForest.from_arrays(...)         the same from plain arrays (fixtures, other trainers)
    .predict_proba(X) .predict(X) .apply(X)    scikit-learn's shapes, dtypes and bits

The model is read by attribute only (``estimators_[i].tree_`` or ``tree_``: ``children_left``,
``children_right``, ``feature``, ``threshold``, ``value``, ``missing_go_to_left``; ``classes_``,
``n_features_in_``): this module does not import scikit-learn. ``tree_.value`` must hold class
fractions (scikit-learn >= 1.3). The forest is uploaded on the first prediction and stays in HBM
until :meth:`GPUForest.free`. pyQSM has no module of this name, so nothing is shadowed.
"""
from __future__ import annotations

import numpy as np

try:
    from .. import hip
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyqsm_amd import hip


def _tree_arrays(tree, n_classes):
    """(left, right, feature, threshold, missing_left, value [nodes, C]) of one ``tree_``."""
    value = np.asarray(tree.value, dtype=np.float64)
    if value.ndim != 3 or value.shape[1] != 1:
        raise ValueError("multi-output trees are not supported")
    left = np.asarray(tree.children_left)
    missing = getattr(tree, "missing_go_to_left", None)
    missing = np.zeros(left.shape, np.uint8) if missing is None else np.asarray(missing, dtype=np.uint8)
    return (left.astype(np.int32), np.asarray(tree.children_right).astype(np.int32),
            np.asarray(tree.feature).astype(np.int32), np.asarray(tree.threshold, dtype=np.float64), missing,
            np.ascontiguousarray(value[:, 0, :n_classes]))


class GPUForest:
    """A classifier forest: the trees' node arrays concatenated (``tree_offsets`` [T+1]; children
    are node numbers within their tree, -1 at a leaf), ``value`` [nodes, C], ``classes`` [C]."""

    def __init__(self, tree_offsets, left, right, feature, threshold, missing_left, value, classes, n_features,
                 single_tree: bool = False, device: int = 0):
        self.tree_offsets = np.ascontiguousarray(tree_offsets, dtype=np.int64)
        self.left = np.ascontiguousarray(left, dtype=np.int32)
        self.right = np.ascontiguousarray(right, dtype=np.int32)
        self.feature = np.ascontiguousarray(feature, dtype=np.int32)
        self.threshold = np.ascontiguousarray(threshold, dtype=np.float64)
        self.missing_left = np.ascontiguousarray(missing_left, dtype=np.uint8)
        self.value = np.ascontiguousarray(value, dtype=np.float64)
        self.classes_ = np.asarray(classes)
        self.n_features_in_ = int(n_features)
        self.single_tree = bool(single_tree)
        self.device = int(device)
        if self.value.ndim != 2 or self.classes_.ndim != 1 or self.value.shape[1] != self.classes_.size:
            raise ValueError(f"value must be [nodes, C] for the C = {self.classes_.size} classes, got {self.value.shape}")
        if self.single_tree and self.tree_offsets.size != 2:
            raise ValueError("single_tree needs exactly one tree")
        self._dev = None

    # ---- construction ----------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, trees, classes, n_features, single_tree: bool = False, device: int = 0) -> "GPUForest":
        """``trees``: one (left, right, feature, threshold, missing_left, value [nodes, C]) per tree."""
        trees = list(trees)
        if not trees:
            raise ValueError("a forest needs at least one tree")
        sizes = [len(t[0]) for t in trees]
        for t, m in zip(trees, sizes):
            if any(len(a) != m for a in t):
                raise ValueError("the arrays of one tree must have one entry per node")
        cat = [np.concatenate([np.asarray(t[j]) for t in trees]) for j in range(6)]
        return cls(np.concatenate([[0], np.cumsum(sizes)]), *cat, classes, n_features, single_tree, device)

    @classmethod
    def from_sklearn(cls, model, device: int = 0) -> "GPUForest":
        classes = getattr(model, "classes_", None)
        if classes is None:
            raise ValueError(f"{type(model).__name__} has no classes_: regressors (and unfitted models) are not supported")
        if getattr(model, "n_outputs_", 1) != 1 or isinstance(classes, list):
            raise ValueError("multi-output models are not supported")
        classes = np.asarray(classes)
        estimators = getattr(model, "estimators_", None)
        single = estimators is None
        if single and not hasattr(model, "tree_"):
            raise ValueError(f"{type(model).__name__} has neither estimators_ nor tree_")
        trees = [model.tree_] if single else [e.tree_ for e in estimators]
        return cls.from_arrays([_tree_arrays(t, classes.size) for t in trees], classes, int(model.n_features_in_),
                               single, device)

    def unpack(self):
        """The per-tree arrays back: a list of (left, right, feature, threshold, missing_left, value)."""
        o = self.tree_offsets
        return [tuple(a[o[k]:o[k + 1]] for a in (self.left, self.right, self.feature, self.threshold,
                                                 self.missing_left, self.value))
                for k in range(o.size - 1)]

    @property
    def n_trees(self) -> int:
        return self.tree_offsets.size - 1

    # ---- the device ------------------------------------------------------------------------
    def device_forest(self) -> "hip.DeviceForest":
        if self._dev is None:
            self._dev = hip.DeviceForest(self.tree_offsets, self.left, self.right, self.feature, self.threshold,
                                         self.missing_left, self.value, self.n_features_in_, self.device)
        return self._dev

    def free(self) -> None:
        if self._dev is not None:
            self._dev.free()
            self._dev = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    # ---- scikit-learn's methods ------------------------------------------------------------
    def predict_proba(self, X) -> np.ndarray:
        """float64 [n, C]: the trees' class fractions added in estimator order, divided by T."""
        x = hip.forest_rows(X, self.n_features_in_)
        return self.device_forest().predict(x, True, False, False)[0]

    def predict_with_proba(self, X):
        """(labels, probabilities) from one pass over the rows."""
        x = hip.forest_rows(X, self.n_features_in_)
        p, idx, _ = self.device_forest().predict(x, True, True, False)
        return self.classes_.take(idx, axis=0), p

    def predict(self, X) -> np.ndarray:
        """``classes_`` at the first maximum of ``predict_proba``."""
        x = hip.forest_rows(X, self.n_features_in_)
        return self.classes_.take(self.device_forest().predict(x, False, True, False)[1], axis=0)

    def apply(self, X) -> np.ndarray:
        """int64 [n, T] leaf node numbers ([n] for a single decision tree)."""
        x = hip.forest_rows(X, self.n_features_in_)
        lv = self.device_forest().predict(x, False, False, True)[2].astype(np.int64)
        return lv[:, 0] if self.single_tree else lv
