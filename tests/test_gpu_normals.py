"""Normal estimation, tangent-plane orientation and the stem stage on the GPU against the NumPy/SciPy
restatement (tests/normals_restatement.py): normals and orientation signs bit-exact, the stem route's
kept set equal up to fp64 atan ulps at the cutoff, every entry point reproducible bit for bit."""
import numpy as np
import pytest

from pyqsm_amd import _lib, hip, qsm_generation, synth
from pyqsm_amd.geometry.cloud import KDTreeSearchParamHybrid, KDTreeSearchParamKNN, PointCloud
from tests import deep_chain
from tests import normals_restatement as R
from tests import wave_select_cases

pytestmark = pytest.mark.gpu


def _same(a, b):
    assert a.shape == b.shape
    assert np.array_equal(a, b)
    assert np.array_equal(np.signbit(a), np.signbit(b))


@pytest.fixture(scope="module")
def forest():
    return synth.forest(200_000, seed=3)


@pytest.mark.parametrize("radius,nn", [(0.1, 30), (0.05, 30), (None, 30)])
def test_normals_forest_bit_exact(gpu, forest, radius, nn):
    got = hip.estimate_normals(forest, radius, nn, device=gpu)
    _same(got, R.estimate_normals(forest, radius, nn))


def test_normals_fp64_negative_coordinates(gpu):
    rng = np.random.default_rng(5)
    P = rng.normal(-3.0, 1.0, (60_000, 3)) * np.array([1.0, 1.0, 0.2]) + 1e-9 * rng.random((60_000, 3))
    assert not np.array_equal(P.astype(np.float32).astype(np.float64), P)
    for radius, nn in ((0.15, 30), (0.3, 256), (None, 17)):
        _same(hip.estimate_normals(P, radius, nn, device=gpu), R.estimate_normals(P, radius, nn))


def test_normals_lattice_ties_go_to_the_lowest_index(gpu):
    j = np.arange(24, dtype=np.float64)
    g = np.stack(np.meshgrid(j, j, j[:10], indexing="ij"), -1).reshape(-1, 3) * 0.25
    g[:, 2] += 0.01 * (g[:, 0] * 0.25)        # a sheared lattice: neighbourhoods are not symmetric
    perm = np.random.default_rng(0).permutation(len(g))
    P = g[perm]
    for radius, nn in ((0.26, 5), (0.36, 10), (0.51, 40), (None, 9)):
        _same(hip.estimate_normals(P, radius, nn, device=gpu), R.estimate_normals(P, radius, nn))


def test_normals_degenerate_cases(gpu):
    P = np.array([[0, 0, 0]] * 4 + [[5, 5, 5], [5.01, 5, 5], [9, 9, 9]], dtype=np.float64)
    _same(hip.estimate_normals(P, 0.1, 30, device=gpu), np.tile([0.0, 0.0, 1.0], (7, 1)))
    prev = np.tile([0.3, -0.4, -0.5], (7, 1))
    _same(hip.estimate_normals(P, 0.1, 30, normals=prev, device=gpu), prev)


def test_previous_normals_set_the_sign(gpu, forest):
    P = forest[:50_000]
    rng = np.random.default_rng(1)
    prev = rng.normal(size=P.shape)
    got = hip.estimate_normals(P, 0.1, 30, normals=prev, device=gpu)
    _same(got, R.estimate_normals(P, 0.1, 30, prev))
    assert np.all(R.dot3(got, prev) >= 0)


def test_max_nn_out_of_range_raises(gpu):
    P = synth.forest(2000, seed=1)
    lib = _lib.load()
    out = np.empty((len(P), 3))
    for r, nn in ((0.1, 0), (0.1, 257), (0.0, 193), (0.0, -1)):
        rc = lib.pyqsm_estimate_normals(hip._p(P), len(P), r, nn, None, hip._p(out), gpu)
        assert rc == -4  # PYQSM_ERANGE
    with pytest.raises(ValueError):
        hip.estimate_normals(P, 0.1, 257, device=gpu)
    with pytest.raises(ValueError):
        hip.estimate_normals(P, None, 193, device=gpu)
    hip.estimate_normals(P, 0.1, 256, device=gpu)


@pytest.mark.parametrize("jitter", [False, True])
def test_normals_clumps_on_both_sides_of_the_step_the_padding_and_the_cap(gpu, jitter):
    """Balls of exactly 1 ... 700 points (tests/wave_select_cases.py): 63 / 64 / 65 candidates around the
    64-candidate step, 127 / 128 / 129 around a power of two of the sort, 511 / 512 without and 513 / 700
    with the bisection for the max_nn-th distance."""
    P, _ = wave_select_cases.clumps(jitter=jitter)
    for radius, nn in ((0.1, 5), (0.1, 30), (0.1, 256)):
        _same(hip.estimate_normals(P, radius, nn, device=gpu), R.estimate_normals(P, radius, nn))


def test_normals_overflow_of_ties_at_the_max_nn_th_distance(gpu):
    """601 points in the origin's ball, more than a wave sorts: with 600 of them tied at the 30th
    distance the call fails with PYQSM_ERANGE; with 400 tied there (and 200 farther) the ties fit
    and the result is the contract's."""
    lib = _lib.load()
    P = np.ascontiguousarray(wave_select_cases.stacked(600))
    out = np.empty((len(P), 3))
    assert lib.pyqsm_estimate_normals(hip._p(P), len(P), 0.1, 30, None, hip._p(out), gpu) == -4  # PYQSM_ERANGE
    P = wave_select_cases.stacked(400, 200)
    _same(hip.estimate_normals(P, 0.1, 30, device=gpu), R.estimate_normals(P, 0.1, 30))


def test_georeferenced_cloud(gpu, forest):
    shift = np.array([5e5, 4e6, 100.0])
    Q = forest[:100_000] + shift
    # Q - shift is exact (Sterbenz): the same geometry as Q, unshifted. Adding the shift itself rounds
    # the forest by up to 2^-31 m, which alone moves ill-conditioned normals by more than 1e-9.
    P = Q - shift
    assert np.max(np.abs(P - forest[:100_000])) <= 2.0 ** -30
    a = hip.estimate_normals(P, 0.1, 30, device=gpu)
    b = hip.estimate_normals(Q, 0.1, 30, device=gpu)
    assert np.max(np.abs(a - b)) <= 1e-9


def _noisy_normals(P, seed):
    N = R.estimate_normals(P, None, 15)
    s = np.where(np.random.default_rng(seed).random(len(P)) < 0.5, -1.0, 1.0)
    return N * s[:, None]


@pytest.mark.parametrize("k", [30, 100])
def test_orientation_bit_exact(gpu, forest, k):
    P = forest[::7][:30_000]
    N = _noisy_normals(P, 2)
    got, rounds = hip.orient_normals_tangent_plane(P, N, k, return_rounds=True, device=gpu)
    _same(got, R.orient_tangent_plane(P, N, k))
    assert rounds > 0


def _sphere(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def test_orientation_two_clusters_each_rooted_at_its_top(gpu):
    S = _sphere(3000, 7)
    P = np.r_[S, S * 0.5 + [50.0, 0, 0]]
    N = np.r_[S, S] * np.where(np.random.default_rng(8).random(6000) < 0.5, -1.0, 1.0)[:, None]
    got = hip.orient_normals_tangent_plane(P, N, 12, device=gpu)
    _same(got, R.orient_tangent_plane(P, N, 12))
    assert np.all(np.sum(got * np.r_[S, S], axis=1) > 0)


def test_orientation_plane_meets_cylinder_with_orthogonal_normals(gpu):
    rng = np.random.default_rng(9)
    m = 4000
    plane = np.c_[rng.uniform(-1, 1, (m, 2)), np.zeros(m)]
    ang = rng.uniform(0, 2 * np.pi, m)
    cyl = np.c_[0.3 * np.cos(ang), 0.3 * np.sin(ang), rng.uniform(0, 1, m)]
    P = np.r_[plane, cyl]
    N = np.r_[np.tile([0.0, 0.0, -1.0], (m, 1)), np.c_[np.cos(ang), np.sin(ang), np.zeros(m)]]
    N[m::2] *= -1
    got = hip.orient_normals_tangent_plane(P, N, 20, device=gpu)
    _same(got, R.orient_tangent_plane(P, N, 20))


def test_orientation_sphere_outward(gpu):
    S = _sphere(20_000, 11)
    P = 3.0 * S + [10.0, -4.0, 2.0]
    N = S * np.where(np.random.default_rng(12).random(len(S)) < 0.5, -1.0, 1.0)[:, None]
    got = hip.orient_normals_tangent_plane(P, N, 30, device=gpu)
    _same(got, R.orient_tangent_plane(P, N, 30))
    assert np.all(np.sum(got * S, axis=1) > 0)


@pytest.mark.parametrize("permuted", [False, True])
def test_orientation_single_deep_chain(gpu, permuted):
    """Points on the y axis whose normals turn by strictly decreasing angles: the first round hooks
    all m points into one tree of depth m - 2 (tests/deep_chain.py), and every parity is the XOR of
    the flips along a path that the bounded pointer jumping has composed."""
    m = 4096
    theta = 0.1 + np.r_[0.0, np.cumsum((1.0 + (m - np.arange(m - 1)) / m) / (2.0 * m))]
    assert theta[-1] < 0.85
    sign = np.where(np.random.default_rng(3).random(m) < 0.5, -1.0, 1.0)
    chain_n = np.c_[np.sin(theta), np.zeros(m), np.cos(theta)] * sign[:, None]
    y = 0.25 * np.arange(m)
    label = deep_chain.relabel(m, permuted, 22)
    a, b = deep_chain.line_graph(y, 2)                      # k = 3 counts the point itself
    deep_chain.assert_one_chain(a, b, 1.0 - np.abs(R.dot3(chain_n[a], chain_n[b])), label)
    P, N = np.zeros((m, 3)), np.empty((m, 3))
    P[label, 1] = y
    N[label] = chain_n
    got, rounds = hip.orient_normals_tangent_plane(P, N, 3, return_rounds=True, device=gpu)
    assert rounds == 1
    _same(got, R.orient_tangent_plane(P, N, 3))
    assert np.all(got[:, 2] > 0)                            # rooted at the top point: index 0 on the all-equal z


def _tree(seed, flat=False):
    rng = np.random.default_rng(seed)
    n = 12_000
    ang = rng.uniform(0, 2 * np.pi, n)
    stem = np.c_[0.2 * np.cos(ang), 0.2 * np.sin(ang), rng.uniform(0, 4, n)]
    m = 8000
    r = 1.5 * np.sqrt(rng.random(m))
    t = rng.uniform(0, 2 * np.pi, m)
    dz = np.zeros(m) if flat else 0.01 * rng.normal(size=m)
    disc = np.c_[r * np.cos(t) + 2.0, r * np.sin(t), 3.0 + dz]
    noise = rng.uniform([-3, -3, 0], [3, 3, 5], (800, 3))
    return np.r_[stem, disc, noise]


def _angle(nrm):
    return np.degrees(np.arctan(nrm[:, 2] / np.sqrt(nrm[:, 0] ** 2 + nrm[:, 1] ** 2)))


def _same_stem(idx, nrm, want_idx, want_nrm, t):
    """Kept sets equal except where the angle sits at the cutoff within fp64 atan ulps; the normals
    of the points both keep bit-exact."""
    only_gpu = ~np.isin(idx, want_idx)
    only_ref = ~np.isin(want_idx, idx)
    for a in (_angle(nrm[only_gpu]), _angle(want_nrm[only_ref])):
        assert np.all(np.abs(np.abs(a) - t) <= 1e-12 * t)
    _same(nrm[~only_gpu], want_nrm[~only_ref])
    assert np.array_equal(idx[~only_gpu], want_idx[~only_ref])


def test_stem_route_matches_restatement(gpu):
    P = _tree(13)
    idx, nrm = hip.stem_cloud(P, 0.1, 30, 100, 10, device=gpu)
    want_idx, want_nrm = R.stem_route(P, 0.1, 30, 100, 10)
    _same_stem(idx, nrm, want_idx, want_nrm, 10)
    z = P[idx, 2]
    assert np.all(z > P[:, 2].min() + 0.5)
    assert len(idx) > 5000


def test_stem_exactly_flat_disc_is_kept(gpu):
    P = _tree(14, flat=True)
    idx, nrm = hip.stem_cloud(P, 0.1, 30, 100, 10, device=gpu)
    want_idx, want_nrm = R.stem_route(P, 0.1, 30, 100, 10)
    _same_stem(idx, nrm, want_idx, want_nrm, 10)
    disc = np.arange(12_000, 20_000)
    inner = disc[np.hypot(P[disc, 0] - 2.0, P[disc, 1]) < 1.3]
    assert np.isin(inner, idx).mean() > 0.9   # n = (0, 0, 1): angle 0, kept (the pinned quirk)


def test_stem_crop_skipped_when_bound_is_zero(gpu):
    P = _tree(15)
    P[:, 2] -= P[:, 2].min() + 0.5          # min z + 0.5 == 0 exactly: pyQSM's crop does nothing
    assert P[:, 2].min() + 0.5 == 0.0
    idx, nrm = hip.stem_cloud(P, 0.1, 30, 50, 10, device=gpu)
    want_idx, want_nrm = R.stem_route(P, 0.1, 30, 50, 10)
    _same_stem(idx, nrm, want_idx, want_nrm, 10)
    assert np.any(P[idx, 2] <= 0.0)


def test_get_stem_pcd_with_config_defaults(gpu):
    P = _tree(16)
    out = qsm_generation.get_stem_pcd(PointCloud(P))
    idx, nrm = hip.stem_cloud(P, 0.1, 30, 100, 10, device=gpu)
    want_idx, want_nrm = R.stem_route(P, 0.1, 30, 100, 10)
    _same_stem(idx, nrm, want_idx, want_nrm, 10)
    assert isinstance(out, PointCloud) and out.has_normals()
    _same(out.points, P[idx])
    _same(out.normals, nrm)
    vox = qsm_generation.get_stem_pcd(PointCloud(P), voxel_size=0.05, post_id_stat_down=True)
    assert 0 < len(vox) < len(out) and vox.has_normals()
    ln = np.linalg.norm(vox.normals, axis=1)
    assert np.all((np.abs(ln - 1) < 1e-12) | (ln == 0))
    with pytest.raises(NotImplementedError):
        qsm_generation.get_stem_pcd(source_file="x.pcd")


def test_pointcloud_methods(gpu, forest):
    pcd = PointCloud(forest[:40_000])
    pcd.estimate_normals(KDTreeSearchParamHybrid(radius=0.1, max_nn=30))
    _same(pcd.normals, R.estimate_normals(pcd.points, 0.1, 30))
    first = pcd.normals.copy()
    pcd.orient_normals_consistent_tangent_plane(50)
    _same(pcd.normals, R.orient_tangent_plane(pcd.points, first, 50))
    knn = PointCloud(forest[:40_000])
    knn.estimate_normals(KDTreeSearchParamKNN(20))
    _same(knn.normals, R.estimate_normals(knn.points, None, 20))


def test_new_entry_points_reproducible(gpu, forest):
    P = forest[:100_000]
    a = hip.estimate_normals(P, 0.1, 30, device=gpu)
    _same(a, hip.estimate_normals(P, 0.1, 30, device=gpu))
    _same(hip.estimate_normals(P, None, 30, device=gpu), hip.estimate_normals(P, None, 30, device=gpu))
    o1 = hip.orient_normals_tangent_plane(P, a, 100, device=gpu)
    _same(o1, hip.orient_normals_tangent_plane(P, a, 100, device=gpu))
    s1 = hip.stem_cloud(P, 0.1, 30, 100, 10, device=gpu)
    s2 = hip.stem_cloud(P, 0.1, 30, 100, 10, device=gpu)
    assert np.array_equal(s1[0], s2[0])
    _same(s1[1], s2[1])
