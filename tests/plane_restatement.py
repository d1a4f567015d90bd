"""The plane-segmentation contract in NumPy: what pyqsm_plane_models,
pyqsm_plane_count, pyqsm_segment_plane and pyqsm_segment_planes are held to.

Modelled on Open3D's SegmentPlane, recollected and parity unpinned: Open3D is not a dependency, so
this is the project's own contract. Deliberate deviations: the normal's sign is fixed (c > 0, then
b > 0, then a > 0), hypotheses with equal counts keep the lower row (Open3D compares an error sum
whose value depends on the summation order), the samples come from the caller, and where f ** m
vanishes next to 1 the early-stop bound is H (Open3D divides by log(1) = 0 there).
"""
from __future__ import annotations

import math

import numpy as np

from tests.normals_restatement import jacobi_smallest

M64 = (1 << 64) - 1


def mulhi64(u: int, n: int) -> int:
    """The high 64 bits of the 128-bit product, on Python integers."""
    return ((int(u) & M64) * (int(n) & M64)) >> 64


def orient(p):
    """The sign rule on one plane (a, b, c, d)."""
    a, b, c = p[0], p[1], p[2]
    keep = c > 0 or (c == 0 and (b > 0 or (b == 0 and a > 0)))
    return np.array(p, dtype=np.float64) if keep else -np.array(p, dtype=np.float64)


def _cross(a, b):  # ransac.hip cross
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def hypothesis(P, idx, axis=None, cos_limit=0.0):
    """The plane of one row of samples: float64 [4], zeros when invalid."""
    P = np.asarray(P, dtype=np.float64)
    n, m = len(P), len(idx)
    zero = np.zeros(4)
    if any(i < 0 or i >= n for i in idx):
        return zero
    with np.errstate(all="ignore"):
        if m == 3:
            p0, p1, p2 = P[idx[0]], P[idx[1]], P[idx[2]]
            nrm = _cross(p1 - p0, p2 - p0)
            L = np.sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2])
            if not L > 0:
                return zero
            nn = nrm / L
            d = -((nn[0] * p0[0] + nn[1] * p0[1]) + nn[2] * p0[2])
        else:
            s = np.zeros(3)
            for i in idx:
                s = s + P[i]
            cen = s / float(m)
            C = np.zeros(6)
            for i in idx:
                o = P[i] - cen
                C = C + np.array([o[0] * o[0], o[0] * o[1], o[0] * o[2], o[1] * o[1], o[1] * o[2], o[2] * o[2]])
            nn = jacobi_smallest((C / float(m))[None, :])[0]
            d = -((nn[0] * cen[0] + nn[1] * cen[1]) + nn[2] * cen[2])
    p = np.array([nn[0], nn[1], nn[2], d])
    if not np.all(np.isfinite(p)):
        return zero
    p = orient(p)
    if cos_limit > 0 and abs((p[0] * axis[0] + p[1] * axis[1]) + p[2] * axis[2]) < cos_limit:
        return zero
    return p


def models(P, samples, axis=None, cos_limit=0.0):
    return np.array([hypothesis(P, list(map(int, row)), axis, cos_limit) for row in samples]).reshape(-1, 4)


def distance(P, plane):
    """|((a x + b y) + c z) + d|, every product and sum rounded on its own."""
    P = np.asarray(P, dtype=np.float64)
    return np.abs(((plane[0] * P[:, 0] + plane[1] * P[:, 1]) + plane[2] * P[:, 2]) + plane[3])


def count(P, planes, thresh):
    """int32 [H]: points strictly within thresh; a row of zeros counts 0."""
    out = np.zeros(len(planes), dtype=np.int32)
    for h, p in enumerate(planes):
        if p[0] != 0 or p[1] != 0 or p[2] != 0:
            out[h] = int((distance(P, p) < thresh).sum())
    return out


def select(counts, n, m, probability):
    """(best, best count, used) by the selection rule over the H counts of n points."""
    H = len(counts)
    best, bc, stop, used = -1, 0, H, H
    for h in range(H):
        if h > stop:
            used = h
            break
        if counts[h] > bc:
            best, bc = h, int(counts[h])
            f = bc / n
            if f >= 1:
                stop = 0
            elif probability == 1:
                stop = H
            else:
                den = math.log(1 - f ** int(m))
                stop = H if den == 0 else min(math.log(1 - probability) / den, H)
    return best, bc, used


def refit(P, inliers):
    """The least-squares plane through the inliers by NumPy's centroid / eigh, under the sign rule
    (what the device's exact-moment refit is compared with, within a tolerance)."""
    Q = np.asarray(P, dtype=np.float64)[inliers]
    cen = Q.mean(axis=0)
    O = Q - cen
    w, v = np.linalg.eigh(O.T @ O / len(Q))
    nn = v[:, 0] / np.linalg.norm(v[:, 0])
    return orient(np.array([nn[0], nn[1], nn[2], -float(nn @ cen)]))


def segment(P, planes, thresh, probability, m):
    """Given the hypothesis planes: (best, used, inliers int64 ascending, hypothesis plane)."""
    P = np.asarray(P, dtype=np.float64)
    best, bc, used = select(count(P, planes, thresh), len(P), m, probability)
    if best < 0:
        return -1, used, np.zeros(0, dtype=np.int64), np.zeros(4)
    inl = np.flatnonzero(distance(P, planes[best]) < thresh).astype(np.int64)
    return best, used, inl, np.array(planes[best])


def local_samples(draws_r, n_alive):
    """The samples of one peeling round as indices into the alive points: int64 [H,m]."""
    d = np.asarray(draws_r, dtype=np.uint64)
    return np.array([[mulhi64(int(u), n_alive) for u in row] for row in d], dtype=np.int64).reshape(d.shape)


def scene(seed=0):
    """The 2500-point peeling scene, shuffled: 1500 ground points on z = 0.05 x - 0.02 y over
    [0, 10]^2 (sigma 0.01 along z), 700 wall points on x = 10.5 (y in [0, 10], z in [0, 4], sigma 0.01
    along x), three rings of 100 points of radius 0.15 (stems at 1 m height). Returns (points [2500,3],
    kind [2500]) with kind 0 ground, 1 wall, 2 stem."""
    rng = np.random.default_rng(seed)
    gx, gy = rng.uniform(0, 10, 1500), rng.uniform(0, 10, 1500)
    ground = np.stack([gx, gy, 0.05 * gx - 0.02 * gy + rng.normal(0, 0.01, 1500)], axis=1)
    wall = np.stack([10.5 + rng.normal(0, 0.01, 700), rng.uniform(0, 10, 700), rng.uniform(0, 4, 700)], axis=1)
    rings = []
    for cx, cy in ((2.0, 3.0), (5.0, 7.0), (8.0, 2.0)):
        t = rng.uniform(0, 2 * np.pi, 100)
        rings.append(np.stack([cx + 0.15 * np.cos(t), cy + 0.15 * np.sin(t), 1.0 + rng.uniform(0, 2, 100)], axis=1))
    P = np.concatenate([ground, wall] + rings)
    kind = np.concatenate([np.zeros(1500, int), np.ones(700, int), np.full(300, 2)])
    perm = rng.permutation(len(P))
    return np.ascontiguousarray(P[perm]), kind[perm]
