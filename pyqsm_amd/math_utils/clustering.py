"""k-means and the silhouette score on the HIP kernels: pyQSM's ``kmeans`` (pyQSM/math_utils/
fit.py:168-214) and the two library calls it makes, ``scipy.cluster.vq.kmeans2`` and
``sklearn.metrics.silhouette_score``.

    kmeans2(data, k, iter=10, seed=None)     scipy kmeans2(data, k, iter), minit='random'
    silhouette_score(points, labels)         sklearn silhouette_score(points, labels)
    kmeans(points, min_clusters, seed=None)  fit.py:168-214
    kmeans_pp(points, n_clusters, seed=0)    sklearn KMeans(n_clusters, random_state=seed, n_init="auto").fit
    kmeanspp_draws(n, k, seed)               the random numbers that fit draws, in its order
    kmeans_feature(smoothed_feature, seed=0) fit.py:160-166 (two clusters of one feature column)

The last three are DESIGN.md §22 (``hip.kmeans_pp``: up to 64 centres, d <= 3, many workgroups).

pyQSM has no module of this name, so nothing is shadowed: ``math_utils.fit.kmeans`` keeps
resolving to pyQSM's own function through the fall-through (tests/test_dropin.py), and this
package's ``choose_and_cluster`` calls the ``kmeans`` defined here.

Differences from the reference, all deliberate:

* The initial centroids are drawn on the host as scipy's ``_krandinit`` draws them, from a NumPy
  ``Generator`` made from ``seed``: ``standard_normal((k, d))`` times the Cholesky factor of the
  data's covariance, plus the mean (the SVD form when m < d). When Cholesky fails on singular data
  the same draws take the SVD form instead of raising (scipy raises ``LinAlgError``); a single
  point is its own centroid (scipy divides 0 by 0 there and raises).
* The centroid sums and the mean silhouette use a fixed chunked order (include/pyqsm_hip.h), not
  scipy's running sum or NumPy's pairwise mean; distances are direct coordinate differences, not
  sklearn's dot-product expansion.
* ``kmeans`` returns every label 0 .. max(best) that has members; the reference's
  ``range(max(best))`` drops the last cluster. No plotting. With ``min_clusters > 1`` and no
  score above 0.4 it returns no clusters (the reference fails on ``max(None)``).
"""
from __future__ import annotations

import numpy as np

try:
    from .. import hip
    from ..geometry.cloud import as_points
    from ..set_config import log
except ImportError:  # flat import (pyqsm_amd/ on sys.path)
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pyqsm_amd import hip
    from pyqsm_amd.geometry.cloud import as_points
    from pyqsm_amd.set_config import log

SCORE_THRESHOLD = 0.4   # fit.py:184 (best_score, never raised)
CANDIDATES = 4          # fit.py:175-180: min_clusters .. min_clusters + 3


def as_generator(seed) -> np.random.Generator:
    return seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)


def krandinit(data, k: int, rng: np.random.Generator) -> np.ndarray:
    """k initial centroids [k,d] drawn like scipy's ``_krandinit`` (module docstring)."""
    data = np.asarray(data, dtype=np.float64)
    m, d = data.shape
    mu = np.mean(data, axis=0)
    if m < d:
        return _svd_form(data, mu, rng.standard_normal(size=(k, min(m, d))))
    cov = np.atleast_2d(np.cov(data.T))
    x = rng.standard_normal(size=(k, d))
    try:
        return x @ np.linalg.cholesky(cov).T + mu
    except np.linalg.LinAlgError:
        return _svd_form(data, mu, x)


def _svd_form(data, mu, x):
    _, s, vh = np.linalg.svd(data - mu, full_matrices=False)
    sVh = s[:, None] * vh / np.sqrt(max(data.shape[0] - 1.0, 1.0))
    return x[:, :len(s)] @ sVh + mu


def kmeans2(data, k: int, iter: int = 10, seed=None, device: int = 0):
    """``scipy.cluster.vq.kmeans2(data, k, iter)`` on d = 2 (the xy pyQSM clusters): returns
    ``(centroids [k,2], labels int32 [m])``. ``k`` may also be an initial centroid array [k,2]
    (minit='matrix'). Labels come from the last assignment, before the last update."""
    data = np.asarray(data, dtype=np.float64)
    if data.ndim != 2 or data.shape[1] != 2:
        raise ValueError("kmeans2 here clusters 2-D data [m,2]")
    if len(data) == 0:
        raise ValueError("Empty input is not supported.")
    init = np.asarray(k, dtype=np.float64) if np.ndim(k) else krandinit(data, int(k), as_generator(seed))
    return hip.kmeans(data, init, iters=int(iter), device=device)


def _valid_count(n_labels: int, m: int) -> bool:
    return 2 <= n_labels <= m - 1


def silhouette_score(points, labels, device: int = 0) -> float:
    """``sklearn.metrics.silhouette_score(points, labels)`` (euclidean): the mean over the points
    of (b - a) / max(a, b), 0 for singletons. Raises ``ValueError`` unless 2 <= number of labels
    <= m - 1, like sklearn."""
    pts = as_points(points)
    uniq, enc = np.unique(np.asarray(labels).reshape(-1), return_inverse=True)
    if len(enc) != len(pts):
        raise ValueError("one label per point")
    if not _valid_count(len(uniq), len(pts)):
        raise ValueError(f"Number of labels is {len(uniq)}. Valid values are 2 to n_samples - 1 "
                         "(inclusive)")
    score, _ = hip.silhouette(pts, enc.astype(np.int32), k=len(uniq), device=device)
    return score


def select(ks, labels, scores, present, m: int):
    """fit.py:181-213 on the candidates' results: the k = 1 labelling is the start; a later one
    replaces it when its silhouette is > 0.4 (an invalid labelling scores 0); the last such wins.
    Returns ``(labels, cluster_idxs)``: every label that has members, and their local indices."""
    best = None
    for q, k in enumerate(ks):
        if k == 1:
            best = labels[q]
            continue
        score = float(scores[q]) if _valid_count(int(present[q]), m) else 0.0
        log.info(f"{k} clusters: silhouette {score}")
        if score > SCORE_THRESHOLD:
            best = labels[q]
    if best is None:
        return [], []
    counts = np.bincount(best)
    out_labels = [int(c) for c in np.flatnonzero(counts)]
    order = np.argsort(best, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(counts)])
    return out_labels, [order[bounds[c]:bounds[c + 1]] for c in out_labels]


def candidate_ks(min_clusters: int):
    ks = [k for k in range(min_clusters, min_clusters + CANDIDATES) if k > 0]
    if ks and ks[-1] > hip.KMEANS_MAX_K:
        raise ValueError(f"at most {hip.KMEANS_MAX_K} clusters")
    return ks


def kmeanspp_draws(n: int, k: int, seed=0):
    """The random numbers scikit-learn's ``KMeans(n_clusters=k, random_state=seed, n_init=1)`` draws on
    ``n`` unweighted samples, in its order, from ``np.random.RandomState(seed)``: the first centre's
    index by ``choice(n, p=uniform)``, then ``uniform(size=T)`` for each further centre,
    T = 2 + int(log(k)). They do not depend on the data. Returns ``(first, uniforms [(k-1)*T])``."""
    rs = seed if isinstance(seed, np.random.RandomState) else np.random.RandomState(seed)
    weight = np.ones(int(n))
    first = int(rs.choice(int(n), p=weight / weight.sum()))
    T = hip.kmeanspp_trials(int(k))
    draws = [rs.uniform(size=T) for _ in range(int(k) - 1)]
    return first, (np.concatenate(draws) if draws else np.zeros(0))


class KMeansResult:
    """What the reference reads off a fitted ``sklearn.cluster.KMeans``, and what the kernel adds."""

    def __init__(self, res):
        self.labels_ = res.labels
        self.cluster_centers_ = res.centres
        self.inertia_ = res.inertia
        self.n_iter_ = res.n_iter
        self.n_empty_ = res.n_empty            # centres without members (scikit-learn relocates those)
        self.seed_indices_ = res.seeds         # the points the k-means++ seeding chose

    def __repr__(self):
        return (f"KMeansResult(n_clusters={len(self.cluster_centers_)}, n_iter_={self.n_iter_}, "
                f"inertia_={self.inertia_!r})")


def kmeans_pp(points, n_clusters: int, seed=0, max_iter: int = 300, tol: float = 1e-4, device: int = 0):
    """``sklearn.cluster.KMeans(n_clusters, random_state=seed, n_init="auto").fit(points)`` on the GPU
    (``hip.kmeans_pp``) for ``points`` [n,d], d <= 3, up to 64 clusters: k-means++
    seeding from scikit-learn's own draws, Lloyd iterations with its stopping rules. Returns a
    :class:`KMeansResult` with ``labels_``, ``cluster_centers_``, ``inertia_`` and ``n_iter_``.

    Differences from scikit-learn, all deliberate: distances are direct coordinate differences (no
    dot-product expansion), sums have the kernel's fixed chunk order, and a centre that loses all its
    members keeps its place (``n_empty_`` says how many; scikit-learn relocates them). On clouds in
    general position the labels are scikit-learn's; exact distance ties may fall differently."""
    pts = np.asarray(points.points if hasattr(points, "points") else points, dtype=np.float64)
    if pts.ndim == 1:
        pts = pts[:, None]
    first, uniforms = kmeanspp_draws(len(pts), int(n_clusters), seed)
    return KMeansResult(hip.kmeans_pp(pts, int(n_clusters), first, uniforms, max_iter=max_iter, tol=tol,
                                      device=device))


def kmeans_feature(smoothed_feature, pcd=None, seed=0, device: int = 0):
    """pyQSM's ``math_utils.fit.kmeans_feature`` (fit.py:160-166): two clusters of one feature column.
    Returns ``(cluster_idxs, cluster_features)``, one entry per label that has members. ``pcd`` is
    accepted and ignored, as there."""
    feature = np.asarray(smoothed_feature, dtype=np.float64).reshape(-1)
    fit = kmeans_pp(feature[:, None], 2, seed=seed, device=device)
    unique_vals, counts = np.unique(fit.labels_, return_counts=True)
    log.info(f'{unique_vals=} {counts=}')
    cluster_idxs = [np.where(fit.labels_ == val)[0] for val in unique_vals]
    return cluster_idxs, [feature[idxs] for idxs in cluster_idxs]


def kmeans(points, min_clusters: int, seed=None, device: int = 0):
    """fit.py:168-214: k-means of the xy of ``points`` [m,3] for k = min_clusters .. +3 (k > 0),
    scored by the silhouette of the 3-D points, all candidates in one device pass
    (``pyqsm_kmeans_select``). The initial centroids are drawn from ``seed`` in the order of k.
    Returns ``(labels, cluster_idxs)``, indices local to ``points``."""
    pts = as_points(points)
    ks = candidate_ks(int(min_clusters))
    if not ks or len(pts) == 0:
        return [], []
    rng = as_generator(seed)
    inits = [krandinit(pts[:, :2], k, rng) for k in ks]
    labels, scores, present = hip.kmeans_select(pts, ks[0], inits, device=device)
    return select(ks, labels, scores, present, len(pts))
