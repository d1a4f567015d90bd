"""pyqsm_radius_degrees / _pairs on the GPU against the CPU statement of their contract
(tests/density_restatement.py, itself pinned to SciPy's cKDTree by tests/test_density_host.py). Every
comparison is exact: the same degrees, the same pair rows."""
import ctypes

import numpy as np
import pytest

from pyqsm_amd import _lib, hip, synth
from pyqsm_amd.geometry import density
from tests import density_restatement as R

pytestmark = pytest.mark.gpu


def check_degrees(P, radii):
    ref, ref_pairs = R.degrees(P, radii)
    deg, n_pairs = hip.radius_degrees(P, radii)
    assert deg.dtype == np.int32 and deg.shape == ref.shape
    assert np.array_equal(deg, ref)
    assert n_pairs.dtype == np.int64 and np.array_equal(n_pairs, ref_pairs)
    return deg, n_pairs


def check_all(P, r):
    check_degrees(P, [r])
    ref = R.pairs(P, r)
    assert np.array_equal(hip.radius_pairs(P, r), ref)


# ---- the smallest clouds, and what needs no kernel ------------------------------------------------

def test_one_point(gpu):
    P = np.array([[0.25, -3.0, 7.5]])
    deg, n_pairs = hip.radius_degrees(P, [0.1, 5.0])
    assert deg.tolist() == [[0], [0]] and n_pairs.tolist() == [0, 0]
    assert hip.radius_pairs(P, 0.1).shape == (0, 2)


def test_two_points_on_the_bound(gpu):
    r = 5 / 64
    P = np.array([[0, 0, 0], [3, 4, 0]], dtype=np.float64) / 64          # exactly r apart
    deg, n_pairs = hip.radius_degrees(P, [r])
    assert deg.tolist() == [[1, 1]] and n_pairs.tolist() == [1]
    assert hip.radius_pairs(P, r).tolist() == [[0, 1]]
    for Q in (P, np.array([[0, 0, 0], [np.nextafter(3 / 64, 1), 4 / 64, 0]])):   # r, or the gap, one ulp off
        rr = np.nextafter(r, 0) if Q is P else r
        deg, n_pairs = hip.radius_degrees(Q, [rr])
        assert deg.tolist() == [[0, 0]] and n_pairs.tolist() == [0]
        assert hip.radius_pairs(Q, rr).shape == (0, 2)
        check_all(Q, rr)


def test_empty_and_invalid_need_no_kernel(gpu):
    E = np.zeros((0, 3))
    deg, cnt = hip.radius_degrees(E, [0.1, 0.2])
    assert deg.shape == (2, 0) and cnt.tolist() == [0, 0]
    assert hip.radius_pairs(E, 0.1).shape == (0, 2)
    P = np.array([[0.0, 0, 0], [1, 0, np.inf]])
    for call in (lambda: hip.radius_degrees(P, [0.1]), lambda: hip.radius_pairs(P, 0.1),
                 lambda: hip.radius_degrees(P[:1], [0.0]), lambda: hip.radius_pairs(P[:1], -1.0),
                 lambda: hip.radius_pairs(P[:1], np.nan)):
        with pytest.raises(_lib.PyQSMHipError) as e:
            call()
        assert e.value.code == -1
    for radii in ([], [0.1] * 9):
        with pytest.raises(_lib.PyQSMHipError) as e:
            hip.radius_degrees(P[:1], radii)
        assert e.value.code == -4


# ---- the lattice: ties on the bound ---------------------------------------------------------------

@pytest.fixture(scope="module")
def lattice():
    return R.lattice()


@pytest.fixture(scope="module")
def lattice_ref(lattice):
    return R.degrees(lattice, R.LATTICE_RADII)


def test_lattice_radii_in_one_call_and_alone(gpu, lattice, lattice_ref):
    ref, ref_pairs = lattice_ref
    assert tuple(ref_pairs.tolist()) == R.LATTICE_PAIRS and ref[0].max() == 122
    order = (2, 0, 3, 1, 0)                                   # unsorted, one radius twice
    deg, n_pairs = hip.radius_degrees(lattice, [R.LATTICE_RADII[k] for k in order])
    for row, k in enumerate(order):
        assert np.array_equal(deg[row], ref[k]) and n_pairs[row] == ref_pairs[k]
    for k, r in enumerate(R.LATTICE_RADII):
        one, cnt = hip.radius_degrees(lattice, [r])
        assert np.array_equal(one[0], ref[k]) and cnt[0] == ref_pairs[k]
        assert np.array_equal(one[0], deg[order.index(k)])   # the two forms agree


def test_lattice_pairs_and_capacity(gpu, lattice):
    r = 3 / 64
    ref = R.pairs(lattice, r)
    assert len(ref) == 199572
    got = hip.radius_pairs(lattice, r)
    assert got.dtype == np.int32 and np.array_equal(got, ref)
    assert np.array_equal(hip.radius_pairs(lattice, r, n_pairs=len(ref)), ref)
    # one row short: capacity rows are written, the count is reported
    cap = len(ref) - 1
    out = np.full((len(ref), 2), -7, dtype=np.int32)
    found = ctypes.c_int64(0)
    _lib.check(_lib.load().pyqsm_radius_pairs(hip._p(lattice), len(lattice), r, cap, hip._p(out), ctypes.byref(found), 0))
    assert found.value == len(ref)
    assert np.array_equal(out[:cap], ref[:cap]) and out[cap].tolist() == [-7, -7]


# ---- one cell holding everything: wave, block and tile boundaries ------------------------------------

# 63 .. 65: one wave; 127 .. 129: the light / heavy threshold of the cells; 255 .. 257: the block and
# the light tile; 1023 .. 1025: the heavy tile; 5000: many runs and tiles
@pytest.mark.parametrize("m", [63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 5000])
def test_clique_in_one_cell(gpu, m):
    r = 0.25
    P = R.ball(m, r)
    deg, n_pairs = hip.radius_degrees(P, [r, 2 * r])
    assert np.all(deg == m - 1) and n_pairs.tolist() == [m * (m - 1) // 2] * 2
    if m <= 1025:
        i, j = np.triu_indices(m, 1)
        assert np.array_equal(hip.radius_pairs(P, r), np.stack([i, j], 1).astype(np.int32))


@pytest.mark.parametrize("heavy", [195, 196, 197])
def test_light_cell_beside_a_heavy_one(gpu, heavy):
    """60 points in one cell, `heavy` in its x neighbour: the light run's row of the stencil holds
    255, 256, 257 candidates, around its tile of 256."""
    rng = np.random.default_rng(heavy)
    r = 0.25
    A = np.array([0.05, 0.05, 0.05]) + 0.15 * rng.random((60, 3))
    B = np.array([0.30, 0.05, 0.05]) + 0.15 * rng.random((heavy, 3))
    P = np.concatenate([A, B])[rng.permutation(60 + heavy)]
    check_all(P, r)


# ---- coincident points, degenerate extents, clamped cells ------------------------------------------

def test_coincident_points(gpu):
    P = np.tile(R.uniform(300, seed=4), (3, 1))[np.random.default_rng(4).permutation(900)]
    deg, _ = check_degrees(P, [0.1, 1e-7])
    assert np.all(deg[1] == 2)                                # the two copies, at distance zero
    check_all(P, 0.1)


def test_flat_cloud(gpu):
    P = R.uniform(3000, seed=6)
    P[:, 2] = 0.375
    check_all(P, 0.04)


def test_chain_across_hundreds_of_cells(gpu):
    C, h = R.chain(), 2.0 ** -5
    deg, n_pairs = hip.radius_degrees(C, [h, np.nextafter(h, 0)])
    assert n_pairs.tolist() == [1999, 0]
    assert deg[0].tolist() == [1] + [2] * 1998 + [1] and not deg[1].any()
    assert np.array_equal(hip.radius_pairs(C, h), np.stack([np.arange(1999), np.arange(1, 2000)], 1))


def test_far_points_in_clamped_cells(gpu):
    P = R.uniform(3000, seed=7)
    far = np.array([[1e4, 0.5, 0.5], [1e4 + 0.04, 0.5, 0.5], [0.5, -1e4, 0.5]])   # the first two are neighbours
    P = np.concatenate([P[:1000], far[:1], P[1000:], far[1:]])
    r = 0.05
    deg, _ = check_degrees(P, [r])
    assert deg[0, 1000] == 1 and deg[0, -2] == 1 and deg[0, -1] == 0
    check_all(P, r)


# ---- one uniform cloud, four storage and grid situations -------------------------------------------

@pytest.fixture(scope="module")
def uniform32():
    return R.uniform(20000, seed=8).astype(np.float32).astype(np.float64)


def test_uniform_fp32_valued(gpu, uniform32):
    check_all(uniform32, 0.03)


def test_uniform_fp64_records(gpu, uniform32):
    P = uniform32 + 1e-9 * np.random.default_rng(11).standard_normal(uniform32.shape)
    assert not np.array_equal(P.astype(np.float32).astype(np.float64), P)
    check_all(P, 0.03)


def test_uniform_shifted(gpu, uniform32):
    P = uniform32 + np.array([4e5, 5e6, 100.0])
    check_all(P, 0.03)


def test_uniform_tiny_radius(gpu, uniform32):
    deg, n_pairs = hip.radius_degrees(uniform32, [1e-6])
    assert not deg.any() and n_pairs.tolist() == [0]
    assert hip.radius_pairs(uniform32, 1e-6).shape == (0, 2)


def test_uniform_pairs(gpu):
    P = R.uniform(3000)
    ref = R.pairs(P, 0.05)
    assert len(ref) > 1000
    assert np.array_equal(hip.radius_pairs(P, 0.05), ref)


# ---- a forest: heavy cells ---------------------------------------------------------------------------

def test_forest_degrees(gpu):
    P = synth.forest(50_000)
    stats = {}
    ref, ref_pairs = R.degrees(P, [0.1, 0.3])
    deg, n_pairs = hip.radius_degrees(P, [0.3, 0.1], stats=stats)
    assert np.array_equal(deg[0], ref[1]) and np.array_equal(deg[1], ref[0])
    assert n_pairs.tolist() == [ref_pairs[1], ref_pairs[0]]
    # every pair within the radius was tested from both sides, and the point against itself
    assert stats["distance_tests"] >= 2 * ref_pairs[1] + len(P) and stats["candidates_staged"] > 0
    one, cnt = hip.radius_degrees(P, [0.1])
    assert np.array_equal(one[0], ref[0]) and cnt[0] == ref_pairs[0]


# ---- the radius sweep of the call sites, as one call ---------------------------------------------------

def test_radius_sweep_on_a_small_forest(gpu):
    P = synth.forest(6000, seed=3)
    g = density.radius_graph(P, [.06, .07, .08, .09])
    ref_deg, ref_pairs = R.degrees(P, g.radii)
    assert np.array_equal(g.degree, ref_deg) and np.array_equal(g.n_pairs, ref_pairs)
    assert np.array_equal(g.pairs(0), R.pairs(P, .06)) and g.pairs(0) is g.pairs(0)
    assert np.array_equal(g.pairs(3), R.pairs(P, .09))


# ---- the same bits twice, and under a permutation ------------------------------------------------------

def test_reproducible_and_permutation(gpu):
    P = synth.forest(5000, seed=5)
    r = 0.12
    deg, n_pairs = hip.radius_degrees(P, [r, 0.05])
    pairs = hip.radius_pairs(P, r, n_pairs[0])
    deg2, n_pairs2 = hip.radius_degrees(P, [r, 0.05])
    assert deg.tobytes() == deg2.tobytes() and n_pairs.tobytes() == n_pairs2.tobytes()
    assert pairs.tobytes() == hip.radius_pairs(P, r).tobytes()
    perm = np.random.default_rng(1).permutation(len(P))          # Q[k] = P[perm[k]]
    Q = P[perm]
    degq, n_pairsq = hip.radius_degrees(Q, [r, 0.05])
    assert np.array_equal(degq, deg[:, perm]) and np.array_equal(n_pairsq, n_pairs)
    back = np.sort(perm[hip.radius_pairs(Q, r)], 1)
    back = back[np.lexsort((back[:, 1], back[:, 0]))]
    assert np.array_equal(back, pairs)


# ---- the analysis layer against its host statements ------------------------------------------------------

def test_get_pairs(gpu):
    from pyqsm_amd.geometry.skeletonize import LineSet
    from pyqsm_amd.utils.lib_integration import get_pairs
    P = R.uniform(1500, seed=12)
    deg0, cnts0, pairs0 = R.get_pairs(P, 0.1)
    degrees, cnts, line_set = get_pairs(query_pts=P, radius=0.1)
    assert np.array_equal(degrees, deg0) and np.array_equal(cnts, cnts0) and line_set is None
    degrees, cnts, line_set = get_pairs(query_pts=P, radius=0.1, return_line_set=True)
    assert isinstance(line_set, LineSet) and np.array_equal(line_set.lines, pairs0)
    assert np.array_equal(degrees, deg0) and np.array_equal(cnts, cnts0)


def test_degree_split(gpu):
    P = synth.forest(4000, seed=7)
    low0, high0, deg0 = R.degree_split(P, .3, 30)
    low, high, deg = density.degree_split(P)                      # radius .3, the 30th percentile
    assert np.array_equal(deg, deg0) and np.array_equal(low, low0) and np.array_equal(high, high0)
    assert len(low) and len(high) and len(low) + len(high) == len(P)
