"""Inputs shared by tests/test_knn_cases_host.py (the CPU proof that every input has the property
its GPU test depends on) and tests/test_gpu_knn_f64.py (the kNN engine of knn.hip, bit-exact against
oracle.knn). What the GPU file is after is the storage form that the contraction loop always runs and
the rest of the suite almost never does: clouds whose coordinates are NOT fp32-representable, which
cloud_bbox answers with three fp64 arrays instead of 16-byte fp32 records.

  offgrid(n, seed)      the synthetic forest moved off the fp32 lattice: every row has a coordinate
                        that no float holds.
  few_ties()            the forest on a 5 mm grid: some queries tie at the k-th place, fewer than
                        n // 16 of them (the wave tie pass of launch_knn_reg).
  many_ties()           a 9 x 9 x 9 lattice of 0.1 steps: most queries tie at the k-th place, more
                        than n // 16 (the per-lane exact pass over the tie list).
  spread_ties()         the same steps on a 16 x 16 x 16 lattice, about one point per node.
  contracted()          what the contraction loop hands the search: most points within 1e-9 .. 1e-3 of
                        the nodes of a 0.5 m lattice, exact duplicates, the rest where it was.
  few_strays(...)       40 points 20 to 60 cloud extents away, five of them a 1 mm cluster.
  many_strays(...)      5 % of the points uniform in a box 50 times the cloud's.
  axis_strays(...)      40 points 3 to 8 extents away along x only: a full-box grid that stays small.
  IDENTICAL, THREE, ONE the degenerate clouds, in coordinates no float holds.

Every case is built once per process from fixed seeds and is read-only; expected() keeps the
oracle's answer for a (case, k, exclude_self) so that tests which share an input share it."""
import functools

import numpy as np

import oracle
from pyqsm_amd import synth

LEVEL0_KS = (1, 4, 5, 12, 13, 20, 28, 29, 32,      # k_knn_reg<4 .. 32>, both sides of each list length
             33, 48, 49, 96, 97, 150, 192)         # k_knn<256>, <128>, <64>; 192 is kKnnMaxK
FEW_TIES_KS = (8, 20, 32)
MANY_TIES_KS = (8, 20)
SPREAD_TIES_KS = (20, 32)
N_FEW_STRAYS = 40
SHIFT = np.array([1.0 / 3.0, 1.0 / 7.0, 1.0 / 11.0])


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def f32_representable(P):
    """Per row: every coordinate survives the round trip through float32."""
    return (P.astype(np.float32).astype(np.float64) == P).all(axis=1)


def off_the_f32_lattice(P):
    return P * (1.0 + 2.0 ** -30) + SHIFT


@functools.lru_cache(maxsize=None)
def forest(n, seed=0):
    return frozen(synth.forest(n, seed))


@functools.lru_cache(maxsize=None)
def offgrid(n, seed=0):
    return frozen(off_the_f32_lattice(synth.forest(n, seed)))


@functools.lru_cache(maxsize=None)
def lattice(n=5000, seed=3):
    """The lattice cloud of tests/test_gpu_knn.py: duplicates and equidistant neighbours, in fp32."""
    return frozen(np.random.default_rng(seed).integers(0, 9, (n, 3)) * 0.125)


@functools.lru_cache(maxsize=None)
def few_ties():
    return frozen(np.round(synth.forest(8000, seed=12) * 200.0) / 200.0)


@functools.lru_cache(maxsize=None)
def many_ties():
    return frozen(np.random.default_rng(7).integers(0, 9, (4000, 3)) * 0.1 + 0.3)


@functools.lru_cache(maxsize=None)
def spread_ties():
    """The same 0.1 steps on a 16 x 16 x 16 lattice: about one point per node instead of many_ties'
    five or six. There the cell edge that gives k / 3 points per occupied cell is a fraction of the
    lattice step, three rings of cells reach no neighbouring node, and at k = 20 every query of
    many_ties is answered by a retry level; here the first grid answers, and its strict pass finds
    the ties."""
    return frozen(np.random.default_rng(7).integers(0, 16, (4000, 3)) * 0.1 + 0.3)


def ties_at_kth(P, k):
    """Queries whose k-th and (k+1)-th neighbour are equally far (the query itself left out)."""
    _, d2 = oracle.knn(P, k + 1, True)
    return int((d2[:, k - 1] == d2[:, k]).sum())


N_COPIES = 800
LATTICE_STEP = 0.5
PULLS = (1e-9, 1e-6, 1e-3)


@functools.lru_cache(maxsize=None)
def contracted():
    """(points, copy_dst, copy_src): points[copy_dst] are exact copies of points[copy_src]."""
    rng = np.random.default_rng(41)
    P = synth.forest(8000, seed=4).copy()
    n = len(P)
    pulled = rng.random(n) < 0.7
    node = np.round(P / LATTICE_STEP) * LATTICE_STEP
    reach = rng.choice(PULLS, (n, 1))
    P[pulled] = (node + rng.uniform(-1.0, 1.0, (n, 3)) * reach)[pulled]
    perm = rng.permutation(n)
    dst, src = perm[:N_COPIES], perm[N_COPIES:2 * N_COPIES]
    P[dst] = P[src]
    return frozen(P), frozen(dst), frozen(src)


def _mixed(base, far, rng, representable):
    n = len(base) + len(far)
    perm = rng.permutation(n)
    X = np.concatenate([base, far])[perm]
    stray = (np.arange(n) >= len(base))[perm]
    if representable:
        X = X.astype(np.float32).astype(np.float64)
    return frozen(X), frozen(stray)


def _base(n, representable):
    return forest(n, 5) if representable else offgrid(n, 5)


@functools.lru_cache(maxsize=None)
def few_strays(representable, n_base=6000):
    """(points, stray mask) as test_few_far_outliers_are_searched_one_by_one builds them, on 6 000 points.
    (On 60 000, that test's size, the retry grid of the box without the strays is still too large to be
    the last level at k = 20 and 64, and the strays' queries reach the whole-cloud search.)"""
    rng = np.random.default_rng(23)
    P = _base(n_base, representable)
    ext = P.max(0) - P.min(0)
    far = P.mean(0) + rng.choice([-1.0, 1.0], (N_FEW_STRAYS, 3)) * rng.uniform(20, 60, (N_FEW_STRAYS, 3)) * ext
    far[:5] = far[0] + rng.normal(0, 1e-3, (5, 3))          # a tiny far cluster: neighbours among themselves
    return _mixed(P, far, rng, representable)


@functools.lru_cache(maxsize=None)
def many_strays(representable):
    """(points, stray mask) as test_many_far_outliers_stay_exact builds them, on 8 000 points."""
    rng = np.random.default_rng(17)
    P = _base(8000, representable)
    ext = P.max(0) - P.min(0)
    far = rng.uniform(P.min(0) - 25 * ext, P.max(0) + 25 * ext, (len(P) // 20, 3))
    return _mixed(P, far, rng, representable)


@functools.lru_cache(maxsize=None)
def axis_strays(representable):
    """(points, stray mask): 40 strays 3 to 8 extents beyond the cloud along x, inside its y and z range.
    The full box is a bar: its grid has few cells, however fine they are."""
    rng = np.random.default_rng(29)
    P = _base(6000, representable)
    lo, hi = P.min(0), P.max(0)
    far = rng.uniform(lo, hi, (N_FEW_STRAYS, 3))
    far[:, 0] = hi[0] + rng.uniform(3, 8, N_FEW_STRAYS) * (hi[0] - lo[0])
    return _mixed(P, far, rng, representable)


STRAYS = {"few_strays": few_strays, "many_strays": many_strays, "axis_strays": axis_strays}

IDENTICAL = frozen(np.zeros((40, 3)) + 0.1)                              # extent 0
THREE = frozen(np.array([[0.1, 0.1, 0.1], [1.1, 0.1, 0.1], [0.1, 2.1, 0.1]]))   # fewer points than k = 5
ONE = frozen(np.array([[0.1, 0.2, 0.3]]))


K_REF = 192     # kKnnMaxK: the one k at which the oracle is asked about a cloud


@functools.lru_cache(maxsize=None)
def _reference(key, exclude_self):
    """oracle.knn at K_REF. The result is ascending in the total order (d2, index), so its first k
    columns ARE the oracle's answer at k, ties across the k-th place included (the host test holds
    that against direct calls). The oracle's grid over a box with far strays costs seconds per call,
    whatever k is: once per cloud instead of once per k."""
    idx, d2 = oracle.knn(_CLOUDS[key[0]](*key[1:]), K_REF, exclude_self)
    return frozen(idx), frozen(d2)


@functools.lru_cache(maxsize=None)
def _expected(key, k, exclude_self):
    idx, d2 = _reference(key, exclude_self)
    return frozen(idx[:, :k]), frozen(d2[:, :k])


_CLOUDS = {
    "forest": forest, "offgrid": offgrid, "lattice": lattice, "few_ties": few_ties, "many_ties": many_ties,
    "spread_ties": spread_ties,
    "contracted": lambda: contracted()[0],
    "few_strays": lambda r, n_base=6000: few_strays(r, n_base)[0], "many_strays": lambda r: many_strays(r)[0],
    "axis_strays": lambda r: axis_strays(r)[0],
}


def cloud(name, *args):
    return _CLOUDS[name](*args)


def expected(name, *args, k, exclude_self=True):
    """oracle.knn of cloud(name, *args), computed once per (cloud, k, exclude_self)."""
    return _expected((name,) + args, int(k), bool(exclude_self))


ALTERNATE_CLOUDS = (("few_ties",), ("many_ties",), ("offgrid", 5000))


def check_alternates(device=0):
    """What a child process of test_gpu_knn_f64.py runs under PYQSM_KNN_BUF=0 or PYQSM_KNN_STRICT=0
    (read once per process): the three clouds at k = 20 against the oracle. Returns the exit status."""
    from pyqsm_amd import _lib, hip
    _lib.require_gpu(device)
    bad = 0
    for key in ALTERNATE_CLOUDS:
        idx, d2 = hip.knn(cloud(*key), 20, True, device=device)
        idx0, d20 = expected(*key, k=20)
        ok = np.array_equal(d2, d20) and np.array_equal(idx, idx0)
        print(f"{key[0]}: {'equal to the oracle' if ok else 'MISMATCH'}", flush=True)
        bad += not ok
    return 1 if bad else 0
