"""The feature stage of ``pyQSM/exploration.py`` on the HIP kernels.

``compute_features`` (``exploration.py:62-68``) and ``smooth_feature`` (``:70-90``) are restated;
every other name of pyQSM's module (file caching, drawing, the random forest) falls through to it
(pyqsm_amd/_shadow.py). Two things the reference gets wrong are not copied: its
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
except ImportError:  # pragma: no cover
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyqsm_amd._shadow import fall_through
    from pyqsm_amd import hip
    from pyqsm_amd.geometry import features as _features
    from pyqsm_amd.geometry.cloud import as_points

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
