"""pyqsm_radius_components on the GPU against the CPU statement of its contract
(tests/density_restatement.py: components() and rank_components(), pinned to SciPy by
tests/test_density_host.py). Every comparison is exact, for `component` and for `sizes`; the counts
stated here were computed on the CPU with the restatement and are asserted of it as well."""
from itertools import chain

import numpy as np
import pytest

from pyqsm_amd import _lib, hip, synth
from pyqsm_amd.geometry import density
from pyqsm_amd.geometry.cloud import PointCloud
from tests import density_restatement as R

pytestmark = pytest.mark.gpu


def check(P, r, count=None, largest=None):
    """The GPU's components of P at r against the restatement's; returns (component, sizes)."""
    ref_comp, ref_sizes = R.components(P, r)
    if count is not None:
        assert len(ref_sizes) == count
    if largest is not None:
        assert ref_sizes[0] == largest
    comp, sizes = hip.radius_components(P, [r])
    assert comp.dtype == np.int32 and comp.shape == (1, len(P))
    assert len(sizes) == 1 and sizes[0].dtype == np.int32
    assert np.array_equal(sizes[0], ref_sizes)
    assert np.array_equal(comp[0], ref_comp)
    return comp[0], sizes[0]


# ---- the smallest clouds ---------------------------------------------------------------------------

def test_one_point(gpu):
    P = np.array([[0.25, -3.0, 7.5]])
    comp, sizes, members = hip.radius_components(P, [0.1, 5.0], members=True)
    assert comp.tolist() == [[0], [0]] and [s.tolist() for s in sizes] == [[1], [1]]
    assert members.tolist() == [[0], [0]]
    check(P, 0.1, 1, 1)


def test_two_points_on_the_bound(gpu):
    r = 5 / 64
    P = np.array([[0, 0, 0], [3, 4, 0]], dtype=np.float64) / 64          # exactly r apart
    comp, sizes = check(P, r, 1, 2)
    assert comp.tolist() == [0, 0] and sizes.tolist() == [2]
    comp, sizes = check(P, np.nextafter(r, 0), 2, 1)
    assert comp.tolist() == [0, 1] and sizes.tolist() == [1, 1]
    comp, sizes = hip.radius_components(P, [np.nextafter(r, 0), r])       # the larger radius' grid serves both
    assert comp.tolist() == [[0, 1], [0, 0]] and [s.tolist() for s in sizes] == [[1, 1], [2]]


# ---- a long diameter: 2 000 one-point cells ------------------------------------------------------------

@pytest.mark.parametrize("shuffled", [False, True])
def test_chain(gpu, shuffled):
    C, h = R.chain(), 2.0 ** -5
    if shuffled:
        C = C[np.random.default_rng(7).permutation(len(C))]
    comp, sizes = check(C, h, 1, 2000)
    assert not comp.any() and sizes.tolist() == [2000]
    comp, sizes = check(C, np.nextafter(h, 0), 2000, 1)
    assert np.array_equal(comp, np.arange(2000)) and sizes.tolist() == [1] * 2000


# ---- ties in the ranking ---------------------------------------------------------------------------------

def test_ranking_ties_by_smallest_member(gpu):
    P, r = R.small_components()
    comp, sizes = check(P, r, 384)
    assert sizes.tolist() == [3] * 128 + [2] * 128 + [1] * 128
    firsts = np.full(384, len(P))
    np.minimum.at(firsts, comp, np.arange(len(P)))
    for s in (0, 128, 256):
        assert np.all(np.diff(firsts[s:s + 128]) > 0)


# ---- the lattice: every edge a tie on the bound ---------------------------------------------------------------

def test_lattice(gpu):
    L = R.lattice()
    comp, sizes = check(L, 1 / 64, 1, 4096)
    comp, sizes = check(L, np.nextafter(1 / 64, 0), 4096, 1)
    assert np.array_equal(comp, np.arange(4096))


# ---- cliques: the light / heavy threshold of the cells and the tiles ---------------------------------------------

@pytest.mark.parametrize("m", [64, 129, 256, 1025, 5000])
def test_clique(gpu, m):
    r = 0.25
    P = R.ball(m, r)
    if m <= 1025:
        check(P, r, 1, m)
    comp, sizes = hip.radius_components(P, [r])                   # a ball of diameter below r: one clique
    assert not comp.any() and sizes[0].tolist() == [m]


# ---- heavy and light cells joined only by edges with d2 == r * r --------------------------------------------------

def test_bridge_on_the_bound(gpu):
    r = 0.125
    A = R.ball(1025, r)
    B = R.ball(300, r) + np.array([1.0, 0.0, 0.0])
    bridge = np.array([[0.5 + 0.125 * k, 0.5, 0.5] for k in range(9)])
    P = np.concatenate([A, B, bridge])
    P = P[np.random.default_rng(9).permutation(len(P))]
    comp, sizes = check(P, r, 1, 1334)
    comp, sizes = check(P, np.nextafter(r, 0), 7, 1027)
    assert sizes.tolist() == [1027, 302, 1, 1, 1, 1, 1]


# ---- coincident points, clamped cells -----------------------------------------------------------------------------

def test_coincident_points(gpu):
    r = 0.1
    P = np.concatenate([np.tile([[0.3, 0.7, 0.2]], (500, 1)), [[0.3, 0.7, 0.2 + 0.09]]])
    comp, sizes = check(P, r, 1, 501)
    comp, sizes = check(P, 0.05, 2, 500)
    assert comp.tolist() == [0] * 500 + [1]


def test_far_points_in_clamped_cells(gpu):
    P = R.uniform(5000, seed=7)
    far = np.array([[1e4, 0.5, 0.5], [1e4 + 0.04, 0.5, 0.5], [0.5, -1e4, 0.5]])   # the first two are neighbours
    P = np.concatenate([P[:1000], far[:1], P[1000:], far[1:]])
    comp, sizes = check(P, 0.05)
    assert comp[1000] == comp[-2] != comp[-1]
    assert sizes[comp[1000]] == 2 and sizes[comp[-1]] == 1


# ---- the percolation sweep: five radii, unsorted, in one call ---------------------------------------------------------

SWEEP = (0.034, 0.026, 0.03, 0.032, 0.028)
SWEEP_COUNTS = (1688, 8607, 4789, 3065, 6633)
SWEEP_LARGEST = (14652, 42, 259, 2652, 102)


@pytest.fixture(scope="module")
def sweep_ref():
    P = R.uniform(20000)
    return P, [R.components(P, r) for r in SWEEP]


def test_sweep_in_one_call(gpu, sweep_ref):
    P, ref = sweep_ref
    assert tuple(len(s) for _, s in ref) == SWEEP_COUNTS and tuple(int(s[0]) for _, s in ref) == SWEEP_LARGEST
    comp, sizes = hip.radius_components(P, SWEEP + (0.03,))              # one radius twice
    for k in range(len(SWEEP)):
        assert np.array_equal(comp[k], ref[k][0]) and np.array_equal(sizes[k], ref[k][1])
    assert np.array_equal(comp[5], comp[2]) and np.array_equal(sizes[5], sizes[2])
    # the partition at a smaller radius refines the one at a larger radius
    by_radius = np.argsort(SWEEP)
    for a, b in zip(by_radius[:-1], by_radius[1:]):
        joint = np.unique(np.stack([comp[a], comp[b]], 1), axis=0)
        assert len(joint) == len(sizes[a])


@pytest.mark.parametrize("k", range(len(SWEEP)))
def test_sweep_rows_equal_single_calls(gpu, sweep_ref, k):
    P, ref = sweep_ref
    comp, sizes = hip.radius_components(P, [SWEEP[k]])
    assert np.array_equal(comp[0], ref[k][0]) and np.array_equal(sizes[0], ref[k][1])


# ---- the grid's storage forms, reached as tests/test_gpu_density.py reaches them ----------------------------------------

@pytest.fixture(scope="module")
def uniform32():
    return R.uniform(20000, seed=8).astype(np.float32).astype(np.float64)


def test_fp32_valued(gpu):
    check(R.fp32_valued(), 0.2)


def test_uniform_fp32_valued(gpu, uniform32):
    check(uniform32, 0.03)


def test_uniform_fp64_records(gpu, uniform32):
    P = uniform32 + 1e-9 * np.random.default_rng(11).standard_normal(uniform32.shape)
    assert not np.array_equal(P.astype(np.float32).astype(np.float64), P)
    check(P, 0.03)


def test_uniform_shifted(gpu, uniform32):
    check(uniform32 + np.array([4e5, 5e6, 100.0]), 0.03)


def test_uniform_tiny_radius(gpu, uniform32):
    comp, sizes = hip.radius_components(uniform32, [1e-6])
    assert np.array_equal(comp[0], np.arange(20000)) and sizes[0].tolist() == [1] * 20000


# ---- a giant component ---------------------------------------------------------------------------------------------------

def test_forest_sweep(gpu):
    P = synth.forest(20000)
    radii = [.06, .07, .08, .09]
    ref = [R.components(P, r) for r in radii]
    assert [len(s) for _, s in ref] == [203, 200, 199, 199]
    assert [int(s[0]) for _, s in ref] == [19796, 19801, 19802, 19802]
    comp, sizes = hip.radius_components(P, radii)
    for k in range(4):
        assert np.array_equal(comp[k], ref[k][0]) and np.array_equal(sizes[k], ref[k][1])


@pytest.fixture(scope="module")
def forest50():
    P = synth.forest(50000)
    return P, R.components(P, 0.1)


def test_forest_giant_component(gpu, forest50):
    P, (ref_comp, ref_sizes) = forest50
    assert len(ref_sizes) == 496 and ref_sizes[0] == 49505
    comp, sizes = hip.radius_components(P, [0.1])
    assert np.array_equal(comp[0], ref_comp) and np.array_equal(sizes[0], ref_sizes)


def test_two_gpu_routes_agree(gpu, forest50, sweep_ref):
    for P, r, ref in ((forest50[0], 0.1, forest50[1]), (sweep_ref[0], 0.03, sweep_ref[1][2])):
        labels, core = hip.dbscan(P, r, 1)
        assert core.all()
        via_dbscan = R.rank_components(labels)
        comp, sizes = hip.radius_components(P, [r])
        assert np.array_equal(via_dbscan[0], comp[0]) and np.array_equal(via_dbscan[1], sizes[0])
        assert np.array_equal(comp[0], ref[0])


# ---- members ----------------------------------------------------------------------------------------------------------------

def test_members(gpu):
    P = synth.forest(6000, seed=3)
    radii = [0.05, 0.12]
    comp, sizes, members = hip.radius_components(P, radii, members=True)
    assert members.dtype == np.int32 and members.shape == comp.shape
    for k in range(2):
        assert np.array_equal(members[k], np.lexsort((np.arange(len(P)), comp[k])))
        assert np.array_equal(comp[k], R.components(P, radii[k])[0])
    # a NULL pointer skips it; the other outputs are the same, and only the valid sizes are written
    n = len(P)
    c2 = np.zeros((2, n), np.int32)
    s2 = np.full((2, n), -7, np.int32)
    cnt = np.zeros(2, np.int64)
    rr = np.array(radii)
    _lib.check(_lib.load().pyqsm_radius_components(hip._p(P), n, hip._p(rr), 2, hip._p(c2), hip._p(s2), None,
                                                   hip._p(cnt), 0))
    assert np.array_equal(c2, comp) and cnt.tolist() == [len(s) for s in sizes]
    for k in range(2):
        assert np.array_equal(s2[k, :cnt[k]], sizes[k]) and np.all(s2[k, cnt[k]:] == -7)


# ---- the same bits twice, and under a permutation ---------------------------------------------------------------------------

def test_reproducible_and_permutation(gpu):
    P = synth.forest(5000, seed=5)
    radii = [0.12, 0.05]
    comp, sizes, members = hip.radius_components(P, radii, members=True)
    comp2, sizes2, members2 = hip.radius_components(P, radii, members=True)
    assert comp.tobytes() == comp2.tobytes() and members.tobytes() == members2.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(sizes, sizes2))
    assert 1 < len(sizes[0]) < len(sizes[1])
    perm = np.random.default_rng(1).permutation(len(P))          # Q[k] = P[perm[k]]
    compq, sizesq = hip.radius_components(P[perm], radii)
    for k in range(2):
        assert np.array_equal(sizesq[k], sizes[k])
        # the same partition: the pairs (rank in Q, rank in P) are a bijection that keeps the sizes
        joint = np.unique(np.stack([compq[k], comp[k][perm]], 1), axis=0)
        assert len(joint) == len(sizes[k])
        assert np.array_equal(sizes[k][joint[:, 0]], sizes[k][joint[:, 1]])


# ---- the wrappers against their host statements -------------------------------------------------------------------------------

def conn_comps(component, sizes):
    return [np.flatnonzero(component == k).tolist() for k in range(len(sizes))]


def test_radius_graph_components(gpu):
    P = synth.forest(6000, seed=3)
    g = density.radius_graph(P, [.06, .09])
    for k, r in enumerate((.06, .09)):
        ref_comp, ref_sizes = R.components(P, r)
        c = g.components(k)
        assert c is g.components(k)
        assert np.array_equal(c.component, ref_comp) and np.array_equal(c.sizes, ref_sizes)
        cc = conn_comps(ref_comp, ref_sizes)
        for s in (0, 1, len(cc) - 1):
            assert c.members(s).tolist() == cc[s]
        want = list(chain.from_iterable(x for x in cc[0:5] if 10 < len(x) < 4000))
        assert c.select(top=5, min_size=10, max_size=4000).tolist() == want


def test_dense_components(gpu):
    P = synth.forest(20000)
    out = density.dense_components(P)                              # [.06 .. .09], top 500, more than 100 points
    assert len(out) == 4
    for c, r in zip(out, (.06, .07, .08, .09)):
        ref_comp, ref_sizes = R.components(P, r)
        assert np.array_equal(c.component, ref_comp) and np.array_equal(c.sizes, ref_sizes)
        cc = conn_comps(ref_comp, ref_sizes)
        assert c.large.tolist() == list(chain.from_iterable(x for x in cc[0:500] if len(x) > 100))
    c = density.dense_components(P, radii=[.07], top=3, min_size=0)[0]
    ref_comp, ref_sizes = R.components(P, .07)
    assert c.large.tolist() == list(chain.from_iterable(conn_comps(ref_comp, ref_sizes)[0:3]))


def test_exclude_dense_areas(gpu, forest50):
    from pyqsm_amd.qsm_generation import exclude_dense_areas
    P, (ref_comp, ref_sizes) = forest50                          # the components at .1, the default radius
    cc = conn_comps(ref_comp, ref_sizes)
    sub, comps = exclude_dense_areas(PointCloud(P))
    assert isinstance(sub, PointCloud)
    assert np.array_equal(comps.component, ref_comp) and np.array_equal(comps.sizes, ref_sizes)
    want = list(chain.from_iterable(x for x in cc[0:500] if len(x) < 100))
    assert len(want) > 0 and np.array_equal(np.asarray(sub.points), P[want])
    sub, _ = exclude_dense_areas(P, radius=.1, top=20, max_size=5)
    want = list(chain.from_iterable(x for x in cc[0:20] if len(x) < 5))
    assert np.array_equal(np.asarray(sub.points), P[want].reshape(-1, 3))
