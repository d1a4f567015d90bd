"""NumPy/SciPy restatement of the normals contract (include/pyqsm_hip.h, "normals").

Open3D's PointCloud.estimate_normals and orient_normals_consistent_tangent_plane, recollected from
Open3D, parity unpinned: this file is what defines them for the kernels of
pyqsm_amd/csrc/normals.hip.

* Neighbourhoods. Hybrid (radius > 0 and finite): the up to max_nn nearest points with
  d2 < radius^2; KNN: the max_nn nearest. The point itself counts. d2 = ((dx*dx) + dy*dy) + dz*dz
  in fp64; neighbours are ordered by (d2, index), so ties at the cut go to the lower index.
  Candidates come from cKDTree with a slightly widened bound and are then decided on the exact d2.
* Covariance on offsets o_j = p_j - p_i: m = (sum o) / N, C = (sum (o - m)(o - m)^T) / N, every sum
  from 0.0 one add at a time in neighbour order (a loop over the neighbour rank, vectorised over
  the points). Open3D's raw-moment form E[pp^T] - E[p]E[p]^T is NOT used: it cancels about
  eleven digits on georeferenced coordinates.
* Eigenvector: the cyclic Jacobi of pyqsm_amd/csrc/pca.hpp (twelve sweeps of the pairs (0,1),
  (0,2), (1,2)), operation for operation; the column of the smallest diagonal entry, divided by
  its length.
* Degenerate: fewer than 3 neighbours or C == 0 give the previous normal, or (0, 0, 1) without
  one. Sign: flipped when dot(n, previous) < 0, or without previous normals when n_z < 0.
* Orientation: the minimum spanning forest of the undirected kNN graph (k including the point,
  self edges dropped), w = 1 - |dot|, edges ordered by (w, min, max), built by Kruskal with a
  union-find that carries parity; flip bit of an edge = dot(n_i, n_j) < 0 on the input normals;
  every component is rooted at its highest point (lowest index on ties), flipped when n_z < 0.
* filter_by_norm: pyQSM's get_angles + filter_by_norm, transcribed. One quirk of the reference is
  not part of the contract: np.apply_along_axis takes its output dtype from the first row, so a
  first normal with nx = ny = 0 (get_angles returns the int 0) truncates every angle to an
  integer. The contract keeps fp64 angles; callers of this transcription keep row 0 generic.
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree


def sqdist(P, i, j):
    d = P[j] - P[i]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _ragged_select(P, rows, cols, k, r2=None):
    """Neighbour table [n,k] (index, -1 padding) and counts from candidate pairs (rows, cols):
    keep d2 < r2 when given, sort by (row, d2, col) and take the first k of every row."""
    d2 = sqdist(P, rows, cols)
    if r2 is not None:
        keep = d2 < r2
        rows, cols, d2 = rows[keep], cols[keep], d2[keep]
    o = np.lexsort((cols, d2, rows))
    rows, cols = rows[o], cols[o]
    n = len(P)
    cnt_all = np.bincount(rows, minlength=n)
    start = np.concatenate(([0], np.cumsum(cnt_all)[:-1]))
    rank = np.arange(len(rows)) - start[rows]
    sel = rank < k
    table = np.full((n, k), -1, dtype=np.int64)
    table[rows[sel], rank[sel]] = cols[sel]
    return table, np.minimum(cnt_all, k)


def neighbourhoods(P, radius, max_nn):
    """(table [n,max_nn] of indices, -1 padded; counts [n])."""
    P = np.asarray(P, dtype=np.float64)
    n = len(P)
    tree = cKDTree(P)
    if radius is not None and radius > 0 and np.isfinite(radius):
        lists = tree.query_ball_point(P, radius * (1 + 1e-9) + 1e-300, workers=16)
        lens = np.fromiter((len(a) for a in lists), dtype=np.int64, count=n)
        rows = np.repeat(np.arange(n), lens)
        cols = np.concatenate([np.asarray(a, dtype=np.int64) for a in lists]) if n else np.zeros(0, np.int64)
        return _ragged_select(P, rows, cols, max_nn, radius * radius)
    k = min(max_nn, n)
    dk, _ = tree.query(P, k=k, workers=16)
    dk = dk.reshape(n, -1)[:, -1]
    lists = tree.query_ball_point(P, dk * (1 + 1e-9) + 1e-300, workers=16)
    lens = np.fromiter((len(a) for a in lists), dtype=np.int64, count=n)
    rows = np.repeat(np.arange(n), lens)
    cols = np.concatenate([np.asarray(a, dtype=np.int64) for a in lists])
    return _ragged_select(P, rows, cols, k)


def covariances(P, table, cnt):
    """[n,6] (c00, c01, c02, c11, c12, c22) accumulated in neighbour order."""
    P = np.asarray(P, dtype=np.float64)
    n, k = table.shape
    dn = cnt.astype(np.float64)
    O = []
    for t in range(k):
        j = np.where(table[:, t] >= 0, table[:, t], np.arange(n))
        O.append(P[j] - P)
    m = np.zeros((n, 3))
    for t in range(k):
        m = np.where((t < cnt)[:, None], m + O[t], m)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = m / dn[:, None]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    C = np.zeros((n, 6))
    for t in range(k):
        on = (t < cnt)
        for c, (a, b) in enumerate(pairs):
            C[:, c] = np.where(on, C[:, c] + (O[t][:, a] - m[:, a]) * (O[t][:, b] - m[:, b]), C[:, c])
    with np.errstate(invalid="ignore", divide="ignore"):
        return C / dn[:, None]


def jacobi_smallest(C):
    """pca.hpp smallest_eigvec, vectorised: [n,6] -> [n,3]."""
    C = np.asarray(C, dtype=np.float64)
    n = len(C)
    a = np.empty((n, 3, 3))
    a[:, 0, 0], a[:, 0, 1], a[:, 0, 2] = C[:, 0], C[:, 1], C[:, 2]
    a[:, 1, 0], a[:, 1, 1], a[:, 1, 2] = C[:, 1], C[:, 3], C[:, 4]
    a[:, 2, 0], a[:, 2, 1], a[:, 2, 2] = C[:, 2], C[:, 4], C[:, 5]
    v = np.tile(np.eye(3), (n, 1, 1))
    with np.errstate(all="ignore"):
        for _ in range(12):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = a[:, p, q].copy()
                on = apq != 0.0
                theta = (a[:, q, q] - a[:, p, p]) / (2.0 * apq)
                sg = np.where(theta >= 0.0, 1.0, -1.0)
                t = sg / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                cs = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * cs
                for r in range(3):
                    arp, arq = a[:, r, p].copy(), a[:, r, q].copy()
                    a[:, r, p] = np.where(on, cs * arp - sn * arq, arp)
                    a[:, r, q] = np.where(on, sn * arp + cs * arq, arq)
                for r in range(3):
                    apr, aqr = a[:, p, r].copy(), a[:, q, r].copy()
                    a[:, p, r] = np.where(on, cs * apr - sn * aqr, apr)
                    a[:, q, r] = np.where(on, sn * apr + cs * aqr, aqr)
                for r in range(3):
                    vrp, vrq = v[:, r, p].copy(), v[:, r, q].copy()
                    v[:, r, p] = np.where(on, cs * vrp - sn * vrq, vrp)
                    v[:, r, q] = np.where(on, sn * vrp + cs * vrq, vrq)
    m = np.zeros(n, dtype=np.int64)
    m = np.where(a[:, 1, 1] < a[np.arange(n), m, m], 1, m)
    m = np.where(a[:, 2, 2] < a[np.arange(n), m, m], 2, m)
    col = v[np.arange(n), :, m]
    ln = np.sqrt((col[:, 0] * col[:, 0] + col[:, 1] * col[:, 1]) + col[:, 2] * col[:, 2])
    return col / ln[:, None]


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def estimate_normals(P, radius, max_nn, prev=None):
    """float64 [n,3] by the contract."""
    P = np.asarray(P, dtype=np.float64)
    table, cnt = neighbourhoods(P, radius, max_nn)
    C = covariances(P, table, cnt)
    v = jacobi_smallest(C)
    if prev is None:
        flip = v[:, 2] < 0.0
    else:
        flip = dot3(v, prev) < 0.0
    v = np.where(flip[:, None], -v, v)
    bad = (cnt < 3) | np.all(C == 0.0, axis=1)
    fb = np.broadcast_to(np.array([0.0, 0.0, 1.0]), v.shape) if prev is None else prev
    return np.where(bad[:, None], fb, v)


def knn_graph(P, k):
    """[n, min(k,n)] exact kNN by (d2, index), the point itself counted."""
    return neighbourhoods(P, None, k)[0]


def orient_tangent_plane(P, N, k):
    """Kruskal with parity over the kNN graph; returns the oriented normals."""
    P = np.asarray(P, dtype=np.float64)
    N = np.asarray(N, dtype=np.float64)
    n = len(P)
    tab = knn_graph(P, k)
    rows = np.repeat(np.arange(n), tab.shape[1])
    cols = tab.reshape(-1)
    ok = cols != rows
    a, b = np.minimum(rows[ok], cols[ok]), np.maximum(rows[ok], cols[ok])
    key = np.unique(a * n + b)
    a, b = key // n, key % n
    d = dot3(N[a], N[b])
    w = 1.0 - np.abs(d)
    o = np.lexsort((b, a, w))
    a, b, f = a[o], b[o], (d[o] < 0.0)
    parent = np.arange(n)
    par = np.zeros(n, dtype=np.int64)

    def find(x):
        p = 0
        path = []
        while parent[x] != x:
            path.append(x)
            p ^= par[x]
            x = parent[x]
        # compress: every node on the path now points at the root with its own parity
        acc = p
        for y in path:
            py = par[y]
            parent[y] = x
            par[y] = acc
            acc ^= py
        return x, p

    merged = 0
    for ea, eb, ef in zip(a.tolist(), b.tolist(), f.tolist()):
        ra, pa = find(ea)
        rb, pb = find(eb)
        if ra == rb:
            continue
        parent[rb] = ra
        par[rb] = pa ^ pb ^ int(ef)
        merged += 1
        if merged == n - 1:
            break
    root = np.empty(n, dtype=np.int64)
    sgn = np.empty(n, dtype=np.int64)
    for i in range(n):
        root[i], sgn[i] = find(i)
    # highest point of each component, lowest index on ties
    o = np.lexsort((np.arange(n), -P[:, 2], root))
    first = np.ones(n, dtype=bool)
    first[1:] = root[o][1:] != root[o][:-1]
    top_of = np.empty(n, dtype=np.int64)
    top_of[root[o][first]] = o[first]
    top = top_of[root]
    s = (sgn ^ sgn[top]) ^ (N[top, 2] < 0.0).astype(np.int64)
    return np.where(s[:, None] == 1, -N, N)


def get_angles(tup, radians=False, reference='XY'):
    """pyQSM/math_utils/general.py get_angles, transcribed (XY reference)."""
    a = tup[0]
    b = tup[1]
    c = tup[2]
    denom = np.sqrt(a**2 + b**2)
    if denom != 0:
        radians = np.arctan(c / np.sqrt(a**2 + b**2))
        if radians:
            return radians
        else:
            return np.degrees(radians)
    else:
        return 0


def filter_by_norm_idx(normals, angle_thresh=10, rev=False):
    """pyQSM/geometry/point_cloud_processing.py filter_by_norm, transcribed: the kept indices."""
    norms = np.asarray(normals)
    if len(norms) == 0:
        return np.zeros(0, dtype=np.int64)
    angles = np.apply_along_axis(get_angles, 1, norms)
    angles = np.degrees(angles)
    if rev:
        return np.where((angles < -angle_thresh) | (angles > angle_thresh))[0]
    return np.where((angles > -angle_thresh) & (angles < angle_thresh))[0]


def stem_route(P, radius, max_nn, orient_k, angle_cutoff, crop_offset=0.5, prev=None):
    """get_stem_pcd's device part: (kept input indices, their oriented normals)."""
    P = np.asarray(P, dtype=np.float64)
    bound = np.min(P[:, 2]) + crop_offset
    idx = np.arange(len(P))
    if bound:
        idx = idx[P[:, 2] > bound]
    Q = P[idx]
    N = estimate_normals(Q, radius, max_nn, None if prev is None else prev[idx])
    N = orient_tangent_plane(Q, N, orient_k)
    keep = filter_by_norm_idx(N, angle_cutoff)
    return idx[keep], N[keep]
