"""Voxel down-sampling, statistical outlier removal and the fused clean_cloud on the GPU against
the NumPy/SciPy restatement (tests/clean_restatement.py): voxel means bit-exact, outlier
averages bit-exact, kept sets identical, every entry point reproducible bit for bit."""
import numpy as np
import pytest

from pyqsm_amd import _lib, hip, synth
from pyqsm_amd.geometry import cleaning
from pyqsm_amd.geometry.cloud import PointCloud
from tests import clean_restatement as R

pytestmark = pytest.mark.gpu
WORKERS = 16


def _same_voxels(P, v, C=None, device=0):
    means, cm, inv, off, mem = R.voxel_down_sample(P, v, C)
    xyz, rgb, (inv_g, off_g, mem_g) = hip.voxel_down_sample(P, v, colors=C, return_trace=True,
                                                            device=device)
    assert xyz.shape == means.shape
    assert np.array_equal(xyz, means)                  # bit-exact, also the signs of zeros
    assert np.array_equal(np.signbit(xyz), np.signbit(means))
    if C is not None:
        assert np.array_equal(rgb, cm)
    assert np.array_equal(inv_g, inv)
    assert np.array_equal(off_g, off)
    assert np.array_equal(mem_g, mem)
    return len(means)


@pytest.mark.parametrize("v", [0.04, 0.1, 1.0])
def test_voxel_forest_bit_exact(gpu, v):
    P = synth.forest(200_000, seed=3)
    m = _same_voxels(P, v, device=gpu)
    assert 1 < m < len(P)


def test_voxel_fp64_cloud_with_negative_coordinates(gpu):
    rng = np.random.default_rng(5)
    P = rng.normal(-3.0, 7.0, (150_000, 3)) * np.array([1.0, 0.3, 2.0]) + 1e-9 * rng.random((150_000, 3))
    assert not np.array_equal(P.astype(np.float32).astype(np.float64), P)
    for v in (0.07, 0.5, 3.3):
        _same_voxels(P, v, device=gpu)


def _keys(P, v):
    """Per-axis key indices by the contract (true division) and by a reciprocal multiply."""
    vmin = P.min(axis=0) - v * 0.5
    return np.floor((P - vmin) / v), np.floor((P - vmin) * (1.0 / v))


def test_voxel_points_on_faces(gpu):
    # exact binary steps: faces at vmin + j * 0.25, where both rules agree
    j = np.arange(-40, 41, dtype=np.float64)
    g = np.stack(np.meshgrid(j, j, j[:9], indexing="ij"), -1).reshape(-1, 3)
    _same_voxels(g * 0.25 - 0.125, 0.25, device=gpu)
    _same_voxels(np.round(g * 0.3, 12), 0.3, device=gpu)


def test_voxel_keys_use_division_not_a_reciprocal(gpu):
    # voxel 0.1 with the minimum at 0.05 per axis: vmin = 0 exactly, and the decimal points
    # x = k / 10 sit on faces. (p - vmin) / 0.1 and (p - vmin) * (1 / 0.1) round to different sides
    # of an integer for many of them (0.3 / 0.1 = 2.9999999999999996, 0.3 * 10 = 3.0000000000000004)
    x = np.array([[0.05, 0.05, 0.05], [0.3, 0.05, 0.05], [0.25, 0.05, 0.05], [0.7, 0.05, 0.05],
                  [0.65, 0.05, 0.05]])
    div, rcp = _keys(x, 0.1)
    assert div[:, 0].tolist() == [0, 2, 2, 6, 6] and rcp[:, 0].tolist() == [0, 3, 2, 7, 6]
    inv = hip.voxel_down_sample(x, 0.1, return_trace=True, device=gpu)[2][0]
    assert inv.tolist() == [0, 1, 1, 2, 2]                 # a reciprocal would give [0, 1, 2, 3, 4]
    _same_voxels(x, 0.1, device=gpu)
    v = np.concatenate([[0.05], np.arange(1, 120) / 10])
    g = np.stack(np.meshgrid(v, v, v[:12], indexing="ij"), -1).reshape(-1, 3)
    div, rcp = _keys(g, 0.1)
    assert (div != rcp).any(axis=1).sum() > 100_000        # the two rules disagree on most points
    _same_voxels(g, 0.1, device=gpu)
    _same_voxels(g[::-1].copy(), 0.1, device=gpu)


def test_voxel_one_voxel_holds_300k_points(gpu):
    rng = np.random.default_rng(7)
    big = rng.random((300_000, 3)) * 0.9 + 0.05            # all in voxel (0, 0, 0) of edge 1
    rest = rng.random((5000, 3)) * 40.0
    P = np.concatenate([rest[:2000], big, rest[2000:]])
    C = rng.random(P.shape)
    m = _same_voxels(P, 1.0, C, device=gpu)
    assert m < 5002


def test_voxel_duplicates_and_tiny_clouds(gpu):
    rng = np.random.default_rng(11)
    P = rng.random((2000, 3))
    P = np.concatenate([P, P[::3], P[:5]])
    _same_voxels(P, 0.05, device=gpu)
    for n in (1, 2):
        _same_voxels(P[:n], 0.05, device=gpu)
    _same_voxels(np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]]), 0.05, device=gpu)
    xyz, rgb = hip.voxel_down_sample(np.zeros((0, 3)), 0.1, device=gpu)
    assert xyz.shape == (0, 3) and rgb is None


def test_voxel_colors_and_point_cloud_method(gpu):
    P = synth.forest(50_000, seed=4)
    C = np.random.default_rng(1).random(P.shape)
    means, cm, *_ = R.voxel_down_sample(P, 0.04, C)
    down = PointCloud(P, C).voxel_down_sample(0.04, device=gpu)
    assert isinstance(down, PointCloud)
    assert np.array_equal(down.points, means) and np.array_equal(down.colors, cm)
    assert PointCloud(P).voxel_down_sample(0.04, device=gpu).colors is None


def test_voxel_keys_wider_than_32_bits(gpu):
    rng = np.random.default_rng(13)
    a = rng.random((20_000, 3)) * np.array([3.0, 3.0, 20.0])
    b = rng.random((20_000, 3)) * np.array([3.0, 3.0, 20.0]) + np.array([5000.0, 5000.0, 0.0])
    P = np.concatenate([a, b])[rng.permutation(40_000)]
    top = np.floor((P.max(0) - (P.min(0) - 0.02)) / 0.04) + 1
    assert np.prod(top) > 2.0 ** 40                      # keys need more than 32 bits
    _same_voxels(P, 0.04, device=gpu)


def test_voxel_keys_whose_low_halves_collide(gpu):
    # voxel 1.0 with nx = ny = 2^16 occupied index ranges: nx * ny = 2^32, so the voxels of one
    # (x, y) column stacked in z have keys exactly 2^32 apart and the same low 32 bits. Their members
    # are interleaved in input order: a sort by the low half alone leaves them mixed, only the
    # second (high-half) pass makes every voxel contiguous.
    rng = np.random.default_rng(17)
    cols = rng.integers(0, 65536, (300, 2))
    c = np.repeat(np.arange(300), 40)
    iz = rng.integers(0, 12, len(c))
    P = np.stack([cols[c, 0], cols[c, 1], iz], 1).astype(np.float64) + 0.5 + rng.random((len(c), 3)) * 0.4 - 0.2
    P[:2] = [[0.5, 0.5, 0.5], [65535.5, 65535.5, 0.5]]
    P = P[rng.permutation(len(P))]
    div, _ = _keys(P, 1.0)
    k3 = div.astype(np.int64)
    dims = k3.max(axis=0) + 1
    assert dims[0] * dims[1] == 2 ** 32 and dims[2] > 1
    key = np.unique(k3[:, 0] + dims[0] * (k3[:, 1] + dims[1] * k3[:, 2]))
    assert len(np.unique(key & 0xFFFFFFFF)) < len(key) // 5          # low halves collide
    m = _same_voxels(P, 1.0, device=gpu)
    assert m == len(key)
    _same_voxels(P, 1.0, C=rng.random(P.shape), device=gpu)


def test_voxel_too_small_is_erange(gpu):
    P = np.random.default_rng(0).random((1000, 3)) * 1000.0
    with pytest.raises(R.VoxelRangeError):
        R.voxel_down_sample(P, 1e-12)
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.voxel_down_sample(P, 1e-12, device=gpu)
    assert e.value.code == -4


def test_voxel_non_finite_is_einval(gpu):
    P = np.zeros((10, 3))
    P[3, 1] = np.nan
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.voxel_down_sample(P, 0.1, device=gpu)
    assert e.value.code == -1


# ---- statistical outlier removal ------------------------------------------------------------

@pytest.fixture(scope="module")
def noisy_forest():
    P = synth.forest(100_000, seed=6)
    noise = synth.ring_cluster(4000, radius=2.0, seed=2, noise=0.3, outliers=0.5)
    return np.concatenate([P, noise])


@pytest.mark.parametrize("nb", [2, 4, 8, 20, 50])
def test_outlier_avg_bit_exact_and_kept_sets(gpu, noisy_forest, nb):
    P = noisy_forest
    avg = R.stat_avg(P, nb, WORKERS)
    mean, std = R.stat_threshold(avg)
    for ratio in (4.0, 4.0 / 1.5, 0.15):
        keep, avg_g, (mean_g, std_g, thr_g) = hip.stat_outlier(P, nb, ratio, return_stats=True,
                                                               device=gpu)
        assert np.array_equal(avg_g, avg)
        assert abs(mean_g - mean) <= 1e-11 * mean
        assert abs(std_g - std) <= 1e-11 * std
        thr = mean + ratio * std
        band = np.abs(avg - thr) <= 1e-9 * thr
        assert band.sum() == 0
        ref = np.nonzero((avg > 0) & (avg < thr))[0]
        assert np.array_equal(keep, ref)


def test_outlier_duplicates_small_and_single(gpu):
    rng = np.random.default_rng(9)
    P = rng.random((3000, 3))
    P = np.concatenate([P, P[:500]])                       # 500 exact pairs: avg == 0 at k = 2
    keep, avg_g, _ = hip.stat_outlier(P, 2, 4.0, return_stats=True, device=gpu)
    keep_r, avg_r, *_ = R.stat_outlier(P, 2, 4.0)
    assert np.array_equal(avg_g, avg_r) and np.array_equal(keep, keep_r)
    assert (avg_g[:500] == 0).all() and not np.isin(np.arange(500), keep).any()
    Q = rng.random((5, 3))
    keep, avg_g, _ = hip.stat_outlier(Q, 50, 1.0, return_stats=True, device=gpu)   # k = min(50, n)
    keep_r, avg_r, *_ = R.stat_outlier(Q, 50, 1.0)
    assert np.array_equal(avg_g, avg_r) and np.array_equal(keep, keep_r)
    assert hip.stat_outlier(Q[:1], 2, 4.0, device=gpu).size == 0
    assert hip.stat_outlier(np.zeros((0, 3)), 2, 4.0, device=gpu).size == 0


def test_outlier_k_above_kmax_is_erange(gpu):
    P = np.random.default_rng(0).random((500, 3))
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.stat_outlier(P, 193, 1.0, device=gpu)
    assert e.value.code == -4


def test_remove_statistical_outlier_method(gpu, noisy_forest):
    pcd = PointCloud(noisy_forest)
    out, ind = pcd.remove_statistical_outlier(nb_neighbors=4, std_ratio=2.0, device=gpu)
    assert ind.dtype == np.int64
    assert np.array_equal(ind, R.stat_outlier(noisy_forest, 4, 2.0, WORKERS)[0])
    assert np.array_equal(out.points, noisy_forest[ind])
    assert np.array_equal(pcd.select_by_index(ind).points, out.points)


# ---- reproducibility ------------------------------------------------------------------------

def test_every_entry_point_is_reproducible_on_1m_points(gpu):
    P = synth.forest(1_000_000, seed=8)
    C = np.random.default_rng(3).random(P.shape)
    a = hip.voxel_down_sample(P, 0.04, colors=C, return_trace=True, device=gpu)
    b = hip.voxel_down_sample(P, 0.04, colors=C, return_trace=True, device=gpu)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    a = hip.stat_outlier(P, 8, 2.0, return_stats=True, device=gpu)
    b = hip.stat_outlier(P, 8, 2.0, return_stats=True, device=gpu)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    a = hip.clean_cloud(P, 0.04, 2, 4, 3, device=gpu)
    b = hip.clean_cloud(P, 0.04, 2, 4, 3, device=gpu)
    assert np.array_equal(a, b)


# ---- clean_cloud ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def forest_1m_noisy():
    P = synth.forest(1_000_000, seed=10)
    rng = np.random.default_rng(12)
    noise = np.concatenate([synth.ring_cluster(20_000, radius=3.0, seed=s, noise=0.5, outliers=0.6)
                            + np.array([10.0 * s, 0.0, 0.0]) for s in range(3)])
    P = np.concatenate([P, noise])
    return P[rng.permutation(len(P))]


def test_clean_cloud_fused_equals_chain_and_restatement(gpu, forest_1m_noisy):
    P = forest_1m_noisy
    fused = cleaning.clean_cloud(P, device=gpu)          # config defaults 0.04, 2, 4, 3
    assert isinstance(fused, PointCloud)
    # the same loop by hand on the PointCloud methods (what pyQSM's own clean_cloud does)
    pcd = PointCloud(P).voxel_down_sample(voxel_size=0.04, device=gpu)
    neighbors, ratio = 2, 4
    for _ in range(3):
        _, ind = pcd.remove_statistical_outlier(nb_neighbors=int(neighbors), std_ratio=ratio, device=gpu)
        pcd = pcd.select_by_index(ind)
        neighbors, ratio = neighbors * 2, ratio / 1.5
    assert np.array_equal(fused.points, pcd.points)
    ref = R.clean_cloud(P, 0.04, 2, 4, 3, WORKERS)
    assert np.array_equal(fused.points, ref)
    assert 0 < len(ref) < len(P)


def test_clean_cloud_stat_step_off_returns_the_input(gpu):
    P = synth.forest(50_000, seed=1)
    pcd = PointCloud(P)
    assert cleaning.clean_cloud(pcd, voxels=0.04, neighbors=2, ratio=4, iters=0) is pcd
    assert np.array_equal(cleaning.clean_cloud(P, voxels=0.04, neighbors=0, ratio=4, iters=3).points, P)
    # the library's own iters = 0 is the voxel step alone
    assert np.array_equal(hip.clean_cloud(P, 0.04, 2, 4, 0, device=gpu), R.voxel_down_sample(P, 0.04)[0])
    # no voxel step: the statistical rounds on the input itself
    assert np.array_equal(cleaning.clean_cloud(P, voxels=0, neighbors=2, ratio=4, iters=2, device=gpu).points,
                          R.clean_cloud(P, 0, 2, 4, 2, WORKERS))
