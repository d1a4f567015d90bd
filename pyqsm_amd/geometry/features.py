"""jakteristics' ``compute_features`` on the HIP kernels (csrc/features.hip), with its signature.

pyQSM computes its per-point wood / leaf features through ``jakteristics.compute_features``
(pyQSM/exploration.py:62-68). jakteristics is not a dependency of this package: the formulas are
recollected from it (Hackel et al. 2016), parity unpinned; tests/features_restatement.py states
the contract in NumPy/SciPy and DESIGN.md §11 lists where it deliberately differs.
pyQSM has no module of this name, so nothing is shadowed.
"""
from __future__ import annotations

import numpy as np

try:
    from .. import hip
    from .cloud import as_points
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyqsm_amd import hip
    from pyqsm_amd.geometry.cloud import as_points

FEATURE_NAMES = list(hip.FEATURE_NAMES)


def compute_features(points, search_radius, *, kdtree=None, num_threads=-1, max_k_neighbors=50000,
                     euclidean_distance=True, feature_names=FEATURE_NAMES):
    """float32 [n, F]: the eigenvalue features of every point's neighbourhood (all points within
    ``search_radius``, the point itself included; the ``max_k_neighbors`` first by (distance,
    index) when more qualify), columns in the order of ``feature_names``, NaN where fewer than 3
    points were kept or lambda1 == 0. ``euclidean_distance=False``: the L1 ball. ``kdtree`` and
    ``num_threads`` are accepted for jakteristics' signature and ignored."""
    del kdtree, num_threads
    out = hip.geometric_features(as_points(points), search_radius, feature_names=feature_names,
                                 max_k=max_k_neighbors,
                                 metric="euclidean" if euclidean_distance else "manhattan")
    return out.astype(np.float32)
