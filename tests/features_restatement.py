"""NumPy/SciPy restatement of the geometric-feature and smoothing contract (include/pyqsm_hip.h,
"geometric features and neighbour smoothing").

jakteristics' compute_features, recollected (Hackel et al. 2016), parity unpinned, and pyQSM's
smooth_feature: this file is what defines them for the kernels of pyqsm_amd/csrc/features.hip.

* Neighbourhood of i: every j (i included) with ((dx*dx) + dy*dy) + dz*dz <= r*r in fp64, or
  (|dx| + |dy|) + |dz| <= r for the L1 ball. Candidates come from cKDTree.query_ball_point with a
  slightly widened bound and are then decided on the exact test. More than max_k: the max_k first
  by (distance, index).
* Covariance on offsets o = p_j - p_i: m = (sum o) / N, C = (sum (o - m)(o - m)^T) / (N - 1).
* numpy.linalg.eigh; lambda1 >= lambda2 >= lambda3 clamped to >= 0; e3 the eigenvector of lambda3
  with e3_z >= 0. N < 3 or lambda1 == 0: NaN.
* Smoothing: the k nearest by (d2, index), d2 = ((dx*dx) + dy*dy) + dz*dz, from cKDTree.query with
  some spare neighbours, re-sorted on the exact d2; mean = fp64 sum in neighbour order / k, median,
  min and max as NumPy's.
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

FEATURE_NAMES = ("eigenvalue_sum", "omnivariance", "eigenentropy", "anisotropy", "planarity", "linearity",
                 "PCA1", "PCA2", "surface_variation", "sphericity", "verticality", "nx", "ny", "nz")

_CHUNK_PAIRS = 8_000_000


def _balls(P, Q, radius, p, tree):
    """Neighbour lists of the queries Q (ragged: counts, flat indices ascending per query)."""
    lists = tree.query_ball_point(Q, radius * (1.0 + 1e-9), p=p, workers=16)
    cnt = np.fromiter((len(l) for l in lists), dtype=np.int64, count=len(lists))
    flat = np.fromiter((j for l in lists for j in l), dtype=np.int64, count=int(cnt.sum()))
    row = np.repeat(np.arange(len(Q)), cnt)
    d = P[flat] - Q[row]
    if p == 2:
        dist = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = dist <= radius * radius
    else:
        dist = (np.abs(d[:, 0]) + np.abs(d[:, 1])) + np.abs(d[:, 2])
        keep = dist <= radius
    return row[keep], flat[keep], dist[keep]


def neighbourhood_moments(P, qidx, radius, max_k=50000, p=2, tree=None):
    """(counts before the cap, N kept, covariance [m, 6] as (c00, c01, c02, c11, c12, c22)) of the
    points P[qidx] against the whole cloud P."""
    P = np.asarray(P, dtype=np.float64)
    tree = cKDTree(P) if tree is None else tree
    m = len(qidx)
    counts = np.zeros(m, dtype=np.int64)
    used = np.zeros(m, dtype=np.int64)
    cov = np.zeros((m, 6))
    est = max(1, int(tree.query_ball_point(P[qidx[:min(m, 200)]], radius, p=p, return_length=True).mean()))
    step = max(1, _CHUNK_PAIRS // est)
    for a in range(0, m, step):
        sl = slice(a, min(m, a + step))
        Q = P[qidx[sl]]
        row, col, dist = _balls(P, Q, radius, p, tree)
        cnt = np.bincount(row, minlength=len(Q))
        counts[sl] = cnt
        if (cnt > max_k).any():  # the max_k first by (distance, index)
            order = np.lexsort((col, dist, row))
            row, col, dist = row[order], col[order], dist[order]
            start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            rank = np.arange(len(row)) - start[row]
            keep = rank < max_k
            row, col = row[keep], col[keep]
            cnt = np.bincount(row, minlength=len(Q))
        used[sl] = cnt
        o = P[col] - Q[row]
        n = np.maximum(cnt, 1).astype(np.float64)
        mean = np.stack([np.bincount(row, o[:, t], minlength=len(Q)) for t in range(3)], 1) / n[:, None]
        c = o - mean[row]
        C = np.stack([np.bincount(row, c[:, a_] * c[:, b_], minlength=len(Q))
                      for a_, b_ in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], 1)
        cov[sl] = C / np.maximum(cnt - 1, 1)[:, None]
    return counts, used, cov


def eig_desc(cov):
    """(lambda [m, 3] descending clamped to >= 0, e3 [m, 3] with e3_z >= 0)."""
    A = np.empty((len(cov), 3, 3))
    A[:, 0, 0], A[:, 0, 1], A[:, 0, 2] = cov[:, 0], cov[:, 1], cov[:, 2]
    A[:, 1, 0], A[:, 1, 1], A[:, 1, 2] = cov[:, 1], cov[:, 3], cov[:, 4]
    A[:, 2, 0], A[:, 2, 1], A[:, 2, 2] = cov[:, 2], cov[:, 4], cov[:, 5]
    w, V = np.linalg.eigh(A)
    lam = np.maximum(w[:, ::-1], 0.0)
    e3 = V[:, :, 0].copy()
    e3[e3[:, 2] < 0] *= -1.0
    return lam, e3


def features_from(lam, e3, used, names=FEATURE_NAMES):
    l1, l2, l3 = lam[:, 0], lam[:, 1], lam[:, 2]
    S = (l1 + l2) + l3
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = np.zeros(len(lam))
        for s in range(3):
            ls = lam[:, s]
            pos = ls > 0
            ent[pos] = ent[pos] + ls[pos] * np.log(ls[pos])
        table = {
            "eigenvalue_sum": S,
            "omnivariance": np.cbrt((l1 * l2) * l3),
            "eigenentropy": -ent,
            "anisotropy": (l1 - l3) / l1,
            "planarity": (l2 - l3) / l1,
            "linearity": (l1 - l2) / l1,
            "PCA1": l1 / S,
            "PCA2": l2 / S,
            "surface_variation": l3 / S,
            "sphericity": l3 / l1,
            "verticality": 1.0 - np.abs(e3[:, 2]),
            "nx": e3[:, 0],
            "ny": e3[:, 1],
            "nz": e3[:, 2],
        }
        out = np.stack([table[f] for f in names], 1)
    out[(used < 3) | ~(l1 > 0)] = np.nan
    return out


def compute_features(P, radius, names=FEATURE_NAMES, max_k=50000, p=2, qidx=None, tree=None):
    """(features [m, F], counts before the cap [m], lambda [m, 3]) of P[qidx] (all points when None)."""
    P = np.asarray(P, dtype=np.float64)
    qidx = np.arange(len(P)) if qidx is None else np.asarray(qidx)
    counts, used, cov = neighbourhood_moments(P, qidx, radius, max_k, p, tree)
    lam, e3 = eig_desc(cov)
    return features_from(lam, e3, used, names), counts, lam


def knn(P, Q, k, tree=None):
    """[m, k] indices of the k nearest of every query, ascending by (d2, index)."""
    P = np.asarray(P, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    tree = cKDTree(P) if tree is None else tree
    kk = min(len(P), k + 16)
    while True:
        _, idx = tree.query(Q, k=kk, workers=16)
        idx = idx.reshape(len(Q), kk)
        d = P[idx] - Q[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        order = np.lexsort((idx, d2), axis=1)
        d2 = np.take_along_axis(d2, order, 1)
        # cKDTree cuts a tie group at kk wherever it likes: take more until the ties at the k-th
        # place all lie inside the table (a lattice ties in groups of more than 16)
        if kk == len(P) or (d2[:, k - 1] < d2[:, kk - 1]).all():
            return np.take_along_axis(idx, order, 1)[:, :k]
        kk = min(len(P), 2 * kk)


def smooth(values, idx, reducer):
    """reducer ("mean", "median", "min", "max") over values[idx] along the neighbours."""
    V = np.asarray(values, dtype=np.float64)[idx]
    if reducer == "mean":
        s = np.zeros(V.shape[:1] + V.shape[2:])
        for t in range(idx.shape[1]):
            s = s + V[:, t]
        return s / idx.shape[1]
    return {"median": np.median, "min": np.min, "max": np.max}[reducer](V, axis=1)
