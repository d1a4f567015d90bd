"""``pyQSM/utils/algo.py``'s ``smooth_feature`` (``:8-22``) on the HIP kNN and reduce kernels
(csrc/features.hip); every other name falls through to pyQSM's module
(pyqsm_amd/_shadow.py)."""
from __future__ import annotations

import numpy as np

try:
    from .. import hip
    from .._shadow import fall_through
    from ..geometry.cloud import as_points
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyqsm_amd import hip
    from pyqsm_amd._shadow import fall_through
    from pyqsm_amd.geometry.cloud import as_points

__getattr__ = fall_through(__name__)


def smooth_feature(points, values, query_pts=None, n_nbrs=25, nbr_func=np.mean):
    """utils/algo.py:8-22: ``nbr_func`` over the values of each query's ``n_nbrs`` nearest points
    (the points themselves when ``query_pts`` is None), along the neighbours."""
    q = None if query_pts is None else as_points(query_pts)
    return hip.smooth_values(as_points(points), values, n_nbrs, reducer=nbr_func, queries=q)
