"""Geometric features and neighbour smoothing on the GPU against the NumPy/SciPy restatement
(tests/features_restatement.py): ball counts equal, features within the tolerances of DESIGN.md
§11, smoothing min / max / median exact and the mean to fp64 rounding, every call reproducible bit
for bit."""
import numpy as np
import pytest

from pyqsm_amd import exploration, hip, synth
from pyqsm_amd.utils import algo
from tests import features_restatement as R
from tests import wave_select_cases

pytestmark = pytest.mark.gpu

NAMES = R.FEATURE_NAMES
DIMLESS = ("anisotropy", "planarity", "linearity", "PCA1", "PCA2", "surface_variation", "sphericity")


def _check(got, want, lam, names=NAMES):
    """got / want [m, F] (F columns named by names), lam [m, 3] of the restatement. Tolerances about
    50x what was measured on the forest and tree-unit clouds."""
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want[:, 0])
    g, w, l = got[ok], want[ok], lam[ok]
    well = (l[:, 1] - l[:, 2]) > 1e-3 * l[:, 0]
    for j, f in enumerate(names):
        d = np.abs(g[:, j] - w[:, j])
        if f in DIMLESS:
            assert d.max(initial=0) <= 1e-12, f
        elif f == "eigenvalue_sum":
            assert (d <= 1e-12 * np.abs(w[:, j])).all(), f
        elif f == "omnivariance":  # cbrt is unbounded in slope at lambda3 = 0: a floor for lambda3 ~ 0
            floor = np.cbrt(l[:, 0] * l[:, 1] * (1e-13 * l[:, 0]))
            assert (d <= 1e-12 * np.abs(w[:, j]) + floor).all(), f
        elif f == "eigenentropy":
            assert (d <= 1e-12 * np.maximum(1.0, np.abs(w[:, j]))).all(), f
        else:  # nx, ny, nz, verticality: where e3 is well posed, up to sign when e3_z ~ 0
            flat = np.abs(w[:, names.index("nz")] if "nz" in names else 1.0) < 1e-12
            if f in ("nx", "ny"):
                d = np.where(flat, np.minimum(d, np.abs(g[:, j] + w[:, j])), d)
            assert d[well].max(initial=0) <= 1e-10, f


@pytest.fixture(scope="module")
def forest100k():
    return synth.forest(100_000, seed=4)


@pytest.mark.parametrize("radius,stride", [(0.1, 1), (0.3, 5)])
def test_forest_all_features(gpu, forest100k, radius, stride):
    P = forest100k
    got, cnt = hip.geometric_features(P, radius, return_counts=True, device=gpu)
    q = np.arange(0, len(P), stride)
    want, wcnt, lam = R.compute_features(P, radius, qidx=q)
    assert np.array_equal(cnt[q], wcnt)
    _check(got[q], want, lam)


def test_tree_unit_reference_radius(gpu):
    P = synth.tree_unit(7, 50_000)
    names = ["planarity", "linearity", "verticality", "surface_variation"]
    got, cnt = hip.geometric_features(P, 0.6, names, return_counts=True, device=gpu)
    q = np.random.default_rng(0).choice(len(P), 3000, replace=False)
    want, wcnt, lam = R.compute_features(P, 0.6, names, qidx=q)
    assert np.array_equal(cnt[q], wcnt)
    _check(got[q], want, lam, names)


def test_full_size_sampled(gpu):
    P = synth.forest(1_000_000, seed=0)
    got, cnt = hip.geometric_features(P, 0.6, return_counts=True, device=gpu)
    q = np.random.default_rng(1).choice(len(P), 2000, replace=False)
    want, wcnt, lam = R.compute_features(P, 0.6, qidx=q)
    assert np.array_equal(cnt[q], wcnt)
    _check(got[q], want, lam)


def test_lattice_inclusive_and_cap(gpu):
    g = np.arange(12, dtype=np.float64)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    got, cnt = hip.geometric_features(P, 1.0, return_counts=True, device=gpu)
    interior = ((P > 0) & (P < 11)).all(1)
    assert (cnt[interior] == 7).all()
    want, wcnt, lam = R.compute_features(P, 1.0)
    assert np.array_equal(cnt, wcnt)
    _check(got, want, lam)
    # the cap keeps the first by (distance, index): 4 of 7 (the ties at distance 1 by index)
    got4 = hip.geometric_features(P, 1.0, max_k=4, device=gpu)
    want4, _, lam4 = R.compute_features(P, 1.0, max_k=4)
    _check(got4, want4, lam4)
    got2, cnt2 = hip.geometric_features(P, 2.0, max_k=20, return_counts=True, device=gpu)
    want2, wcnt2, lam2 = R.compute_features(P, 2.0, max_k=20)
    assert np.array_equal(cnt2, wcnt2)
    _check(got2, want2, lam2)


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("mk", [4, 64, 100000])
def test_clumps_on_both_sides_of_the_cap_and_the_staging_flush(gpu, jitter, mk):
    """Balls of exactly 1 ... 700 points (tests/wave_select_cases.py): at max_k = 64 the clumps of 63 / 64 /
    65 straddle the cap, those of 127 / 128 / 129 the 64-entry flush of the moment staging."""
    P, size = wave_select_cases.clumps(jitter=jitter)
    got, cnt = hip.geometric_features(P, 0.1, max_k=mk, return_counts=True, device=gpu)
    want, wcnt, lam = R.compute_features(P, 0.1, max_k=mk)
    assert np.array_equal(wcnt, size) and np.array_equal(cnt, wcnt)
    _check(got, want, lam)


def test_lattice_ties_at_the_cap_are_cut_by_index(gpu):
    P = wave_select_cases.lattice_clump(513)
    assert wave_select_cases.tie_at(P, P, 100).any()   # the 100th and 101st distances of some point are equal
    got, cnt = hip.geometric_features(P, 2.0, max_k=100, return_counts=True, device=gpu)
    want, wcnt, lam = R.compute_features(P, 2.0, max_k=100)
    assert (wcnt == 513).all() and np.array_equal(cnt, wcnt)
    _check(got, want, lam)


def test_fp64_negative_coordinates(gpu):
    rng = np.random.default_rng(5)
    P = rng.normal(-3.0, 1.0, (40_000, 3)) * np.array([1.0, 1.0, 0.2]) + 1e-9 * rng.random((40_000, 3))
    assert not np.array_equal(P.astype(np.float32).astype(np.float64), P)
    got, cnt = hip.geometric_features(P, 0.25, return_counts=True, device=gpu)
    want, wcnt, lam = R.compute_features(P, 0.25)
    assert np.array_equal(cnt, wcnt)
    _check(got, want, lam)


def test_georeferenced_cloud(gpu, forest100k):
    shift = np.array([5e5, 4e6, 100.0])
    Q = forest100k + shift
    P = Q - shift
    a, ca = hip.geometric_features(P, 0.1, return_counts=True, device=gpu)
    b, cb = hip.geometric_features(Q, 0.1, return_counts=True, device=gpu)
    assert np.array_equal(ca, cb)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a[:, 0])
    dimless = [NAMES.index(f) for f in DIMLESS]
    assert np.max(np.abs(a[ok][:, dimless] - b[ok][:, dimless])) <= 1e-9


def test_manhattan_ball(gpu, forest100k):
    P = forest100k[::2]
    got, cnt = hip.geometric_features(P, 0.15, metric="manhattan", return_counts=True, device=gpu)
    want, wcnt, lam = R.compute_features(P, 0.15, p=1)
    assert np.array_equal(cnt, wcnt)
    _check(got, want, lam)


def test_reproducible_and_permutation_invariant(gpu, forest100k):
    P = forest100k
    a = hip.geometric_features(P, 0.2, device=gpu)
    b = hip.geometric_features(P, 0.2, device=gpu)
    assert a.tobytes() == b.tobytes()
    perm = np.random.default_rng(9).permutation(len(P))
    c = hip.geometric_features(P[perm], 0.2, device=gpu)
    # the moments are exact integer sums: the same bits whatever the input order
    assert c.tobytes() == a[perm].tobytes()


# ---- smoothing -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(11)
    return rng.uniform(0, 5, (60_000, 3))


@pytest.mark.parametrize("k", [25, 50, 100])
def test_smooth_self_query(gpu, forest100k, k):
    P = forest100k[:60_000]
    rng = np.random.default_rng(k)
    V = rng.normal(size=(len(P), 2))
    V[rng.random(len(P)) < 0.001, 1] = np.nan
    idx = R.knn(P, P, k)
    for red in ("mean", "median", "min", "max"):
        got1 = hip.smooth_values(P, V[:, 0], k, red, device=gpu)
        got2 = hip.smooth_values(P, V, k, red, device=gpu)
        want = R.smooth(V, idx, red)
        assert got1.shape == (len(P),) and got2.shape == (len(P), 2)
        if red == "mean":
            assert np.array_equal(np.isnan(got2), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.all(np.abs(got2[ok] - want[ok]) <= 1e-12 * np.abs(want[ok]) + 1e-300)
        else:
            assert np.array_equal(got2, want, equal_nan=True)
        assert np.array_equal(got1, got2[:, 0], equal_nan=True)


def test_smooth_indices_and_host_callable(gpu, forest100k):
    P = forest100k[:50_000]
    V = np.random.default_rng(2).normal(size=len(P))
    res, idx = hip.smooth_values(P, V, 30, np.std, return_indices=True, device=gpu)
    want_idx = R.knn(P, P, 30)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(res, np.std(V[want_idx], axis=1))


def test_smooth_mean_matches_sklearn(gpu, cloud):
    from sklearn.neighbors import NearestNeighbors
    V = np.random.default_rng(3).normal(size=len(cloud))
    got = algo.smooth_feature(cloud, V, n_nbrs=25)
    ref = np.mean(V[NearestNeighbors(n_neighbors=25).fit(cloud).kneighbors(cloud)[1]], axis=1)
    assert np.allclose(got, ref, rtol=1e-12, atol=1e-15)


def test_smooth_separate_queries_with_far_outliers(gpu, cloud):
    rng = np.random.default_rng(4)
    Q = np.concatenate([rng.uniform(-1, 6, (20_000, 3)),
                        np.array([[1e4, 0, 0], [-3e5, 2e5, 7.5], [2.5, 2.5, 1e6]])])
    V = rng.normal(size=(len(cloud), 3))
    for k in (1, 25, 100):
        want_idx = R.knn(cloud, Q, k)
        res, idx = hip.smooth_values(cloud, V, k, "median", queries=Q, return_indices=True, device=gpu)
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(res, R.smooth(V, want_idx, "median"))
        mean = hip.smooth_values(cloud, V, k, np.mean, queries=Q, device=gpu)
        want = R.smooth(V, want_idx, "mean")
        assert np.all(np.abs(mean - want) <= 1e-12 * np.abs(want) + 1e-300)
    sep = exploration.smooth_feature(cloud, V[:, 0], query_pts=cloud[:5000], n_nbrs=25, smoothing_func=np.max)
    assert np.array_equal(sep, hip.smooth_values(cloud, V[:, 0], 25, "max", device=gpu)[:5000])


@pytest.mark.parametrize("m", [511, 512, 513, 700])
def test_smooth_far_queries_see_the_whole_cloud_on_both_sides_of_the_cap(gpu, m):
    """A query 50 m away is first served at a radius that holds all m sources: k_query_knn sorts 511 or 512
    pairs as they are and bisects (distance, then index among the ties of a lattice) for 513 and 700."""
    src = wave_select_cases.random_cube(m) if m == 700 else wave_select_cases.lattice_clump(m)
    Q = wave_select_cases.far_queries(src)
    V = np.random.default_rng(m).normal(size=len(src))
    for k in wave_select_cases.SMOOTH_KS:
        assert all(wave_select_cases.first_sufficient_radius(src, q, k)[1] == m for q in Q[:6])
        if m == 513:
            assert wave_select_cases.tie_at(src, Q[:6], k).any()
        _, idx = hip.smooth_values(src, V, k, "mean", queries=Q, return_indices=True, device=gpu)
        assert np.array_equal(idx, R.knn(src, Q, k))


def test_end_to_end_reference_defaults(gpu):
    P = synth.tree_unit(3, 50_000)
    names = ["planarity", "linearity", "verticality", "surface_variation"]
    f = exploration.compute_features(P, 0.6, names)
    assert f.dtype == np.float32 and f.shape == (len(P), 4)
    raw = hip.geometric_features(P, 0.6, names, device=gpu).astype(np.float32)
    nan = np.isnan(raw)
    assert not np.isnan(f).any()
    assert np.array_equal(f[~nan], raw[~nan])
    fill = np.broadcast_to(np.nanmean(raw.astype(np.float64), 0).astype(np.float32), raw.shape)
    assert np.allclose(f[nan], fill[nan], rtol=1e-6)
    s = algo.smooth_feature(P, f[:, 0])
    assert s.dtype == np.float32 and s.shape == (len(P),)
    want = R.smooth(f[:, 0].astype(np.float64), R.knn(P, P, 25), "mean").astype(np.float32)
    assert np.allclose(s, want, rtol=1e-6)
