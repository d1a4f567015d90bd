"""Sphere-following branch tracing: pyQSM's ``sphere_step`` (pyQSM/qsm_generation.py:182-316,
called from ``find_low_order_branches`` at :480) with the cloud resident in HBM.

pyQSM's ``qsm_generation.sphere_step`` itself keeps resolving to the reference through the
fall-through of ``qsm_generation`` (tests/test_dropin.py), which is why this lives in a module of
its own, as ``clean_cloud`` lives in ``geometry/cleaning.py``.

A :class:`SphereTracer` uploads the main cloud once and keeps the ``found`` byte mask on the
device. Each step's ball (``pyqsm_ball_excl_dev``) leaves the unfound neighbours gathered in a
device buffer, which DBSCAN (``pyqsm_dbscan_dev_ex``) or the fused k-means selection
(``pyqsm_kmeans_select_dev``) reads where it lies: only the neighbour indices, the labels and the
core flags cross the bus.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np

try:
    from . import hip
    from .geometry.cloud import as_points
    from .math_utils import clustering
    from .math_utils.fit import _group_labels
    from .math_utils.general import get_center, get_radius
    from .qsm_generation import fit_cyl_to_cluster
    from .set_config import config, log
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pyqsm_amd import hip
    from pyqsm_amd.geometry.cloud import as_points
    from pyqsm_amd.math_utils import clustering
    from pyqsm_amd.math_utils.fit import _group_labels
    from pyqsm_amd.math_utils.general import get_center, get_radius
    from pyqsm_amd.qsm_generation import fit_cyl_to_cluster
    from pyqsm_amd.set_config import config, log


class SphereTracer:
    """One tracing session on one device: the main cloud and the ``found`` mask in HBM, and the
    buffers every step reuses (neighbour indices, their gathered xyz, DBSCAN labels and core
    flags). ``cloud_uploads`` counts uploads of the main cloud (one per session)."""

    def __init__(self, main_pts, total_found=(), device: int = 0):
        self.pts = as_points(main_pts)
        self.n = len(self.pts)
        self.device = int(device)
        cap = max(self.n, 1)
        self.xyz = hip.DeviceBuffer.from_array(self.pts, device)
        self.cloud_uploads = 1
        self.found = hip.DeviceBuffer.from_array(np.zeros(cap, dtype=np.uint8), device)
        self.idx = hip.DeviceBuffer(cap * 8, device)
        self.nn_xyz = hip.DeviceBuffer(cap * 24, device)
        self.labels = hip.DeviceBuffer(cap * 8, device)
        self.core = hip.DeviceBuffer(cap, device)
        self.mark(total_found)

    def mark(self, idxs) -> None:
        idxs = np.asarray(idxs, dtype=np.int64).reshape(-1)
        if len(idxs):
            hip.mark_found_dev(self.found.ptr, self.n, idxs, device=self.device)

    def ball(self, center, radius: float) -> np.ndarray:
        """Indices (ascending) of the unfound points within ``radius`` of ``center``; their xyz
        stay gathered on the device for :meth:`cluster`."""
        m = hip.ball_excl_dev(self.xyz.ptr, self.n, self.found.ptr, center, radius, self.idx.ptr,
                              self.nn_xyz.ptr, device=self.device)
        self.m = m
        return self.idx.download(m, np.int64) if m else np.zeros(0, dtype=np.int64)

    def cluster(self, new_neighbors, cluster_type: str, rng):
        """``choose_and_cluster(new_neighbors, main_pts, cluster_type)`` (fit.py:58-85, the package's
        form in math_utils/fit.py) on the neighbours of the last :meth:`ball`."""
        m = len(new_neighbors)
        returned = []
        if cluster_type == "kmeans":
            log.info("clustering via kmeans")
            ks = clustering.candidate_ks(1)
            xy = self.pts[new_neighbors, :2]
            inits = [clustering.krandinit(xy, k, rng) for k in ks]
            lab, scores, present = hip.kmeans_select_dev(self.nn_xyz.ptr, m, ks[0], inits, device=self.device)
            labels, local = clustering.select(ks, lab, scores, present, m)
            returned = [new_neighbors[c] for c in local]
        if cluster_type != "kmeans" or len(returned) < 2:
            log.info("clustering via DBSCAN")
            hip.dbscan_dev(self.nn_xyz.ptr, m, config["dbscan"]["epsilon"], config["dbscan"]["min_neighbors"],
                           self.labels.ptr, self.core.ptr, device=self.device)
            dl = self.labels.download(m, np.int64)
            core = self.core.download(m, np.uint8).astype(bool)
            labels, returned, _noise = _group_labels(dl, core, new_neighbors)
        return labels, returned

    def free(self) -> None:
        for b in (self.xyz, self.found, self.idx, self.nn_xyz, self.labels, self.core):
            b.free()


def sphere_step(curr_pts, last_radius, main_pcd, cluster_idxs, branch_order=0, branch_num=0,
                total_found=None, run=0, branches=None, id_to_num=None, cyls=None, cyl_details=None,
                spheres=None, draw_every=10, debug=False, seed=None, device: int = 0, tracer=None):
    """qsm_generation.py:182-316 on one :class:`SphereTracer`. Returns ``(branches, id_to_num,
    cyls, cyl_details)``, or ``[]`` when the first step finds nothing to follow, as the reference.

    Followed line by line: ``fit_cyl_to_cluster`` on ``curr_pts`` (which it clamps in place, as the
    reference does); the ball around their centroid with radius ``get_radius x radius_multiplier``
    clamped to ``[min_radius, max_radius]``; ``choose_and_cluster`` (k-means after a bad fit,
    DBSCAN after a good one); every cluster added to ``total_found`` before any recursion; then for
    each ``zip(labels, clusters)`` the branch bookkeeping, the radius clamps and the step into the
    cluster. ``branches[0][0]`` is the ``total_found`` list itself (:211-212). ``seed`` feeds one
    NumPy Generator consumed in visiting order: each step's RANSAC samples, then its k-means
    initialisations.

    Differences from the reference, all deliberate:

    1. Points already found are excluded from the ball, as the comment at :219 intends (the
       reference's find_neighbors_in_ball returns the unfiltered neighbours, so the recursion walks
       the same points again until Python's recursion limit).
    2. An explicit stack replaces the recursion and visits the clusters in the same order, so no
       recursion limit applies.
    3. The state (branches, id_to_num, cyls, cyl_details, spheres) is fresh for every top-level
       call unless passed in; the reference's mutable defaults carry it from call to call.
    4. The drawing and ``breakpoint()`` blocks are dropped (``draw_every``, ``debug`` and ``run``
       are accepted and ignored). The reference's recursive call hands ``debug`` to ``draw_every``,
       so its drawing test divides by zero there.
    ``spheres`` receives ``(center, radius)`` pairs instead of Open3D meshes; ``cyls`` the 500
    points sampled on each good fit's cylinder."""
    sph = config["sphere"]
    total_found = [] if total_found is None else total_found
    branches = [[]] if branches is None else branches
    id_to_num = defaultdict(int) if id_to_num is None else id_to_num
    cyls = [] if cyls is None else cyls
    cyl_details = [] if cyl_details is None else cyl_details
    spheres = [] if spheres is None else spheres
    rng = clustering.as_generator(seed)
    if branches == [[]]:
        branches[0].append(total_found)
    own = tracer is None
    if own:
        tracer = SphereTracer(as_points(main_pcd), total_found, device=device)
    main_pts = tracer.pts

    def enter(curr_pts, last_radius, cluster_idxs):
        """The body of one call up to its loop: the (label, cluster) pairs to follow, or None."""
        curr_pts = np.asarray(curr_pts)
        good = fit_cyl_to_cluster(main_pcd, curr_pts, last_radius, cluster_idxs, cyls=cyls,
                                  cyl_details=cyl_details, seed=rng, device=tracer.device)
        log.info("getting new neighbors ")
        center = get_center(curr_pts)
        radius = get_radius(curr_pts) * sph["radius_multiplier"]
        radius = min(max(radius, sph["min_radius"]), sph["max_radius"])
        new_neighbors = tracer.ball(center, radius)
        spheres.append((center, radius))
        clusters = ()
        if len(new_neighbors) > 0:
            labels, clusters = tracer.cluster(new_neighbors, "DBSCAN" if good else "kmeans", rng)
        if clusters == [] or len(new_neighbors) < sph["min_contained_points"]:
            return None
        for c in clusters:
            total_found.extend(c)
        tracer.mark(np.concatenate(clusters) if len(clusters) else [])
        return list(zip(labels, clusters))

    try:
        pairs = enter(curr_pts, last_radius, cluster_idxs)
        if pairs is None:
            return []
        # a frame: [pairs, next position, branch_order, branch_num, last_radius]
        stack = [[pairs, 0, branch_order, branch_num, last_radius]]
        while stack:
            frame = stack[-1]
            pairs, pos, order, num, radius_in = frame
            if pos == len(pairs):
                stack.pop()
                continue
            frame[1] += 1
            label, c = pairs[pos]
            cluster_branch = order
            if label != 0:
                cluster_branch += 1
                branches.append([])
            branch_id = num + cluster_branch
            id_to_num.update({i: branch_id for i in c})
            branches[cluster_branch].extend(c)
            cluster_pts = main_pts[c]
            r = get_radius(cluster_pts)
            r = min(max(r, sph["min_radius"]), sph["max_radius"])
            if r < radius_in / 2:
                r = radius_in / 2
            frame[3] += 1   # the caller's branch_num += 1 after the step returns
            child = enter(cluster_pts, r, c)
            if child is not None:
                stack.append([child, 0, cluster_branch, num, r])
        return branches, id_to_num, cyls, cyl_details
    finally:
        if own:
            tracer.free()
