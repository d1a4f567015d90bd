"""Clouds that put a candidate count on each side of the boundaries of csrc/wave_select.hpp: the
64-candidate step of a wave, the power-of-two padding of its sort and the 512-pair cap of the normals
and of k_query_knn. NumPy and SciPy only; tests/test_wave_select_host.py checks the preconditions the
GPU cases rely on, so that a change here cannot silently empty one of them."""
import numpy as np
from scipy.spatial import cKDTree

SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 700)
RADIUS = 0.1                                   # the ball of every clump point is exactly its clump
QUERY_SHIFT = np.array([0.001, -0.002, 0.0005])
FAR = 50.0                                     # metres from the cloud's centre to a far query
SMOOTH_KS = (1, 64, 192)


def clumps(sizes=SIZES, jitter=False):
    """(points [n, 3], size [n]): one clump per entry of sizes, centres 10 m apart along x, points uniform
    in a cube of edge 0.04 around the centre, rows shuffled; size[i] is the size of point i's clump.
    jitter False: coordinates rounded through float32 (the grid's fp32 records); True: 1e-9 * random
    added, so they are not float32-representable (fp64 arrays). Asserts that within RADIUS every
    point has exactly its clump."""
    rng = np.random.default_rng(20 + int(jitter))
    P = np.concatenate([rng.uniform(-0.02, 0.02, (s, 3)) + [10.0 * c, 0.0, 0.0] for c, s in enumerate(sizes)])
    size = np.repeat(np.asarray(sizes), sizes)
    P = P.astype(np.float32).astype(np.float64)
    if jitter:
        P = P + 1e-9 * rng.random(P.shape)
    perm = rng.permutation(len(P))
    P, size = P[perm], size[perm]
    assert np.array_equal(P.astype(np.float32).astype(np.float64), P) == (not jitter)
    assert np.array_equal(cKDTree(P).query_ball_point(P, RADIUS, return_length=True), size)
    return P, size


def clump_queries(P):
    """Every point shifted by QUERY_SHIFT (still RADIUS from its whole clump and no other), plus one query 1 km
    away."""
    Q = np.concatenate([P + QUERY_SHIFT, [[1000.0, 1000.0, 1000.0]]])
    return Q


def lattice_clump(m):
    """The first m sites (x fastest, then y, then z) of a lattice of pitch 0.125 that is 8 x 8 sites wide,
    shuffled: 512 sites fill an 8 x 8 x 8 cube, the 513th starts a ninth layer. Every coordinate is a
    multiple of 2^-3, so squared distances are exact and tie in large groups."""
    s = np.arange(m)
    P = np.stack([s % 8, (s // 8) % 8, s // 64], 1) * 0.125
    return P[np.random.default_rng(m).permutation(m)]


def random_cube(n=700):
    return np.random.default_rng(n).uniform(0.0, 1.0, (n, 3))


def sqdist(P, Q):
    """[m, n] squared distances of the queries Q to the points P, accumulated as the kernels do."""
    d = P[None, :, :] - Q[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def far_queries(src):
    """Six points FAR from the centre of src's bounding box along +-x, +-y, +-z, then the centre itself."""
    c = 0.5 * (src.min(0) + src.max(0))
    return np.concatenate([c + FAR * np.r_[np.eye(3), -np.eye(3)], [c]])


def brute_knn(P, Q, k):
    """[m, k] indices of the k nearest of every query by (d2, index), from all m * n distances."""
    d2 = sqdist(P, Q)
    idx = np.broadcast_to(np.arange(len(P)), d2.shape)
    return np.take_along_axis(idx, np.lexsort((idx, d2), axis=1), 1)[:, :k]


def tie_at(P, Q, k):
    """bool [m]: the k-th and (k + 1)-th smallest squared distances of the query are equal."""
    d2 = np.sort(sqdist(P, Q), axis=1)
    return d2[:, k - 1] == d2[:, k] if k < len(P) else np.zeros(len(Q), bool)


def first_sufficient_radius(P, q, k):
    """The radius at which the query kNN serves q: 0.5 * extent * sqrt(k / n), doubled until at least k points
    lie within it (features.hip query_knn_device); and how many points lie within it."""
    d2 = sqdist(P, q[None])[0]
    R = 0.5 * (P.max(0) - P.min(0)).max() * np.sqrt(k / len(P))
    while (d2 <= R * R).sum() < k:
        R *= 2.0
    return R, int((d2 <= R * R).sum())


def stacked(near, far=0):
    """The origin, then `near` copies of (0.05, 0, 0) and `far` copies of (0.08, 0, 0): within RADIUS of
    the origin lie 1 + near + far points, and near of them tie at its second distance."""
    return np.concatenate([[[0.0, 0.0, 0.0]], np.tile([0.05, 0.0, 0.0], (near, 1)), np.tile([0.08, 0.0, 0.0], (far, 1))])
