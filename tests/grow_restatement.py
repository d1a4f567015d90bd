"""Index-based NumPy / SciPy restatement of the region growing rule of ``pyqsm_grow_clusters``
(include/pyqsm_hip.h), and the inputs the growth tests share. No GPU, no library call.

Cycle c: every frontier point of every cluster that is still growing selects its (at most k nearest)
source points with d < radius (``cKDTree.query(k, distance_upper_bound)``: strict). A free point goes
to the smallest cluster index among the clusters that selected it in that cycle. What a cluster
acquired is its next frontier; a cluster that acquired fewer than ``min_new`` points stops.

Ties at the k-th distance are SciPy's here (unspecified); the tests compare against this module only
on inputs without such ties."""
from types import SimpleNamespace

import numpy as np
from scipy.spatial import cKDTree


def grow(src, owner_in, seeds, k, radius, cycles, min_new=5):
    """``seeds``: one float64 [m_i,3] array per cluster (the frontier of cycle 0). Returns a namespace
    with ``owner``, ``cycle`` int32 [n], ``finished`` int32 [n_clusters], ``frontiers`` (queries
    served per cycle) and the counters ``contested`` (points selected as free by more than one cluster
    in a cycle, summed over the cycles), ``over_k`` (frontier queries with more than k sources in
    reach), ``small_end`` / ``empty_end`` (clusters that ended on fewer than ``min_new`` but some new
    points / on none)."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    n, n_cl = len(src), len(seeds)
    owner = np.asarray(owner_in, dtype=np.int32).copy()
    cycle = np.full(n, -1, dtype=np.int32)
    frontier = [np.asarray(s, dtype=np.float64).reshape(-1, 3) for s in seeds]
    active = [len(f) > 0 for f in frontier]
    finished = np.array([-1 if a else 0 for a in active], dtype=np.int32)
    out = SimpleNamespace(contested=0, over_k=0, small_end=0, empty_end=0, frontiers=[])
    tree = cKDTree(src) if n else None
    for c in range(int(cycles)):
        if not any(active):
            break
        out.frontiers.append(sum(len(frontier[i]) for i in range(n_cl) if active[i]))
        selected = {}
        times = np.zeros(n, dtype=np.int64)
        for i in range(n_cl):
            if not active[i]:
                continue
            if n == 0:
                selected[i] = np.zeros(0, dtype=np.int64)
                continue
            _, idx = tree.query(frontier[i], k=int(k) + 1, distance_upper_bound=radius)
            idx = idx.reshape(len(frontier[i]), -1)
            out.over_k += int((idx[:, k] != n).sum()) if idx.shape[1] > k else 0
            nb = np.unique(idx[:, :k])
            nb = nb[nb != n]
            selected[i] = nb[owner[nb] < 0]
            times[selected[i]] += 1
        out.contested += int((times > 1).sum())
        for i in sorted(selected):                       # the lower cluster index wins
            new = selected[i][owner[selected[i]] < 0]
            owner[new] = i
            cycle[new] = c
            frontier[i] = src[new]
            if len(new) < min_new:
                active[i] = False
                finished[i] = c + 1
                if len(new):
                    out.small_end += 1
                else:
                    out.empty_end += 1
    out.owner, out.cycle, out.finished = owner, cycle, finished
    return out


def seed_owner(src, seeds):
    """The ownership ``extend_seed_clusters`` starts from: source points equal to a seed point carry
    that seed's cluster, later seeds overwriting earlier ones."""
    src = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    owner = np.full(len(src), -1, dtype=np.int32)
    where = {}
    for j, p in enumerate(src):
        where.setdefault(tuple(p), []).append(j)
    for i, s in enumerate(seeds):
        for p in np.asarray(s, dtype=np.float64).reshape(-1, 3):
            for j in where.get(tuple(p), ()):
                owner[j] = i
    return owner


def clusters_as_sets(src, seeds, owner, cycle, labels):
    """{label: set of point tuples}: the seed points and the acquired points of every cluster, the
    form in which ``oracle.extend_seed_clusters`` is compared (a seed point that two seeds share
    belongs to the later one, as in the reference's dict)."""
    sets = {}
    assn = {}
    for i, s in enumerate(seeds):
        for p in np.asarray(s, dtype=np.float64).reshape(-1, 3):
            assn[tuple(p)] = i
    for j in np.flatnonzero(np.asarray(cycle) >= 0):
        assn.setdefault(tuple(src[j]), int(owner[j]))
    for p, i in assn.items():
        sets.setdefault(labels[i], set()).add(p)
    return sets


# ---- the inputs of tests/test_grow_host.py and tests/test_gpu_grow.py --------------------------------

def slab():
    """60 000 random points in a 6 x 6 x 0.05 slab, 300 seeds of 9 to 33 points (some points fall in
    two seeds). Random coordinates: no distance ties."""
    rng = np.random.default_rng(7)
    P = np.concatenate([rng.uniform(0, 6, (60000, 2)), rng.uniform(0, 0.05, (60000, 1))], axis=1)
    centres = rng.uniform(0.2, 5.8, (300, 2))
    seeds = [P[np.linalg.norm(P[:, :2] - c, axis=1) < 0.06] for c in centres]
    return P, seeds


def strip(columns):
    gx, gy = np.meshgrid(np.arange(columns) * 0.02, np.arange(6) * 0.02, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size)], 1)


def mixed():
    """A strip (grows for many cycles), a line one point wide (ends on fewer than five new points),
    seven points on their own (end on none) and a cluster without a seed."""
    s = strip(61)
    line = np.stack([np.full(30, -1.0), np.arange(30) * 0.02, np.zeros(30)], 1)
    alone = np.array([5.0, 5.0, 5.0]) + np.random.default_rng(0).normal(0, 0.001, (7, 3))
    src = np.concatenate([s, line, alone])
    seeds = [s[:12], line[:3], alone, np.zeros((0, 3))]
    return src, seeds


def contested_strip(columns):
    s = strip(columns)
    return s, [s[:12], s[-12:]]
