"""The feature stage of ``pyQSM/exploration.py`` on the HIP kernels.

``compute_features`` (``exploration.py:62-68``), ``smooth_feature`` (``:70-90``) and
``random_forest_classification`` (``:460-538``; fitted by scikit-learn on the host, every prediction
on the GPU) are restated; every other name of pyQSM's module (file caching,
drawing) falls through to it (pyqsm_amd/_shadow.py). Two things the reference gets wrong are not copied: its
``replace_nanfeatures`` indexes jakteristics' plain array by feature name (IndexError), where the
intent, done here, is to fill each column's NaNs with that column's nanmean; and its
``np.array_split(query_pts, 100000)`` makes empty pieces below 100 000 queries, on which sklearn
raises.
"""
from __future__ import annotations

import logging
import warnings

import numpy as np

try:  # flat import style of the reference (pyqsm_amd on sys.path) or package import
    from ._shadow import fall_through
    from . import hip
    from .geometry import features as _features
    from .geometry.cloud import as_points
    from .math_utils.forest import GPUForest
except ImportError:  # pragma: no cover
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyqsm_amd._shadow import fall_through
    from pyqsm_amd import hip
    from pyqsm_amd.geometry import features as _features
    from pyqsm_amd.geometry.cloud import as_points
    from pyqsm_amd.math_utils.forest import GPUForest

# names pyQSM's module of the same name defines and this one does not (pyqsm_amd/_shadow.py)
__getattr__ = fall_through(__name__)

log = logging.getLogger("calc")


def fill_nan_columns(features: np.ndarray) -> np.ndarray:
    """Each column's NaNs replaced by that column's nanmean, in place; a column that is all NaN
    stays NaN."""
    for j in range(features.shape[1]):
        col = features[:, j]
        bad = np.isnan(col)
        if bad.any() and not bad.all():
            log.info(f" {int(bad.sum())} points have a null value for feature column {j}.")
            col[bad] = np.nanmean(col)
    return features


def compute_features(points, search_radius=0.6, feature_names=['verticality'], num_threads=4):
    """exploration.py:62-68: float32 [n, F] features of every point's ball (jakteristics'
    formulas on the GPU), each column's NaNs filled with its nanmean."""
    pts = as_points(points)
    log.info(f'Computing features for {len(pts)} points')
    features = _features.compute_features(pts, search_radius=search_radius, num_threads=num_threads,
                                          feature_names=feature_names)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return fill_nan_columns(features.astype(np.float64)).astype(np.float32)


def smooth_feature(points, values, query_pts=None, n_nbrs=25, smoothing_func=np.mean):
    """exploration.py:70-90: ``smoothing_func`` over the values of each query's ``n_nbrs``
    nearest points (the points themselves when ``query_pts`` is None), along the neighbours."""
    q = None if query_pts is None else as_points(query_pts)
    return hip.smooth_values(as_points(points), values, n_nbrs, reducer=smoothing_func, queries=q)


def random_forest_classification(model_feat_names_options, smoothed_feats, all_labeled_idxs, unlabeled_idxs,
                                 group_labels, file_name, num_trees=[200], train_size=.8, *, label_groups=None,
                                 n_estimators=None, save_dir=None, device=0):
    """exploration.py:460-538: per option (a list of feature names) stack those columns of
    ``smoothed_feats`` (name -> [N] values), split the labelled rows with ``train_test_split(
    train_size, random_state=42, stratify=group_labels, shuffle=True)``, fit ``RandomForestClassifier(
    random_state=42, n_jobs=-1)`` with scikit-learn on the host, then predict on the GPU both the
    hold-out rows (accuracy) and the unlabelled rows.

    Returns one dict per option: ``feat_names``, ``model`` (scikit-learn's), ``forest`` (the
    :class:`GPUForest`, resident in HBM until its ``free()``), ``n_estimators``, ``accuracy``,
    ``test_idxs``, ``test_pred``, ``pred_labels`` and ``pred_proba`` of the unlabelled rows, and
    ``predicted_group_idxs``: group -> the ascending indices (values of ``unlabeled_idxs``)
    predicted to be in it, every group present.

    Where the reference slips, on purpose not copied:

    * it reads ``label_groups``, ``pcd`` and ``grped_idxs``, which are not in its scope. Here
      ``label_groups`` is a keyword: a mapping whose keys, in order, name the classes 0, 1, ...
      (the labels must then be those integers, as the reference indexes the names by the
      prediction); without it the groups are keyed by the class labels themselves.
    * its loop trains 201 trees whatever ``num_trees`` says. ``num_trees`` stays in the signature
      and stays ignored; 201 is the default and ``n_estimators=`` overrides it.
    * ``holden.py:62-85`` passes one flat list of names where a list of lists is iterated: both
      are accepted.
    * it pickles every model into the working directory and reads it back, draws the predicted
      clouds and stops in ``breakpoint()``. Nothing is drawn; ``save_dir`` (off by default) writes
      ``rf_model_{option}_{trees}trees.pkl`` there.
    * its ``train_size`` argument is shadowed by a literal .8; here the argument is honoured.
    """
    from sklearn.ensemble import RandomForestClassifier
    from sklearn.model_selection import train_test_split
    options = list(model_feat_names_options)
    if options and all(isinstance(o, str) for o in options):
        options = [options]
    labeled = np.asarray(all_labeled_idxs, dtype=np.int64)
    unlabeled = np.asarray(unlabeled_idxs, dtype=np.int64)
    y = np.asarray(group_labels)
    if labeled.ndim != 1 or unlabeled.ndim != 1 or y.shape != labeled.shape:
        raise ValueError("all_labeled_idxs, unlabeled_idxs and group_labels must be 1-D, one label per labelled index")
    names = None if label_groups is None else list(label_groups.keys() if hasattr(label_groups, "keys")
                                                   else label_groups)
    trees = 201 if n_estimators is None else int(n_estimators)
    if trees < 1:
        raise ValueError(f"n_estimators must be at least 1, got {n_estimators!r}")
    results = []
    for idx, feat_names in enumerate(options):
        feat_names = list(feat_names)
        missing = [f for f in feat_names if f not in smoothed_feats]
        if missing:
            raise ValueError(f"smoothed_feats has no column(s) {missing}")
        all_feats = np.stack([np.asarray(smoothed_feats[f]).reshape(-1) for f in feat_names], axis=1)
        X_train, X_test, y_train, y_test, _, test_idxs = train_test_split(
            all_feats[labeled], y, labeled, train_size=train_size, random_state=42, stratify=y, shuffle=True)
        log.info(f'using {feat_names} for model {idx} with {trees} trees')
        rf = RandomForestClassifier(n_estimators=trees, random_state=42, n_jobs=-1)
        rf.fit(X_train, y_train)
        forest = GPUForest.from_sklearn(rf, device=device)
        if names is not None and not np.array_equal(forest.classes_, np.arange(len(forest.classes_))):
            raise ValueError("label_groups names classes 0, 1, ...: group_labels must be those integers")
        if names is not None and len(names) < len(forest.classes_):
            raise ValueError(f"label_groups names {len(names)} groups, the labels have {len(forest.classes_)}")
        test_pred = forest.predict(X_test)
        acc = float(np.mean(test_pred == y_test))
        log.info(f"RandomForest accuracy on hold-out labeled set: {acc:.3f}")
        log.info('feature importances:\n' + str(rf.feature_importances_))
        log.info(f'predicting groups for {len(unlabeled)} unlabeled points')
        pred, proba = forest.predict_with_proba(all_feats[unlabeled])
        keys = names if names is not None else [c.item() if hasattr(c, "item") else c for c in forest.classes_]
        groups = {g: np.empty(0, dtype=np.int64) for g in keys}
        for ci, c in enumerate(forest.classes_):
            groups[keys[ci]] = np.sort(unlabeled[pred == c])
        if save_dir is not None:
            import os
            import pickle
            with open(os.path.join(save_dir, f'rf_model_{idx}_{trees}trees.pkl'), 'wb') as f:
                pickle.dump(rf, f)
        results.append({"feat_names": feat_names, "model": rf, "forest": forest, "n_estimators": trees,
                        "accuracy": acc, "test_idxs": test_idxs, "test_pred": test_pred, "pred_labels": pred,
                        "pred_proba": proba, "predicted_group_idxs": groups})
    return results
