"""The host side of the stem-width measurement (pyqsm_amd/geometry/stem_width.py) against NumPy and
SciPy themselves, and the restatement the GPU tests compare with (tests/width_restatement.py) against
the same: the rank rule and the lerp equal np.percentile bit for bit, the square root of the sorted
squared keys is the sorted pdist, and the conventions without a pair need no device."""
import numpy as np
import pytest
from scipy.spatial.distance import pdist

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry import stem_width as sw
from pyqsm_amd.geometry.cloud import PointCloud
from tests import width_restatement as R

QS = [0, 37.5, 50, 90, 95, 99.9, 100]
SIZES = [2, 3, 24, 65, 257]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_rank_rule_and_lerp_are_numpys(kind, dim):
    for n in SIZES:
        d = R.sorted_pdist(R.make_points(kind, n, dim, seed=n))
        want = np.percentile(d, QS)
        lo, hi, t = sw.percentile_ranks(len(d), QS)
        assert (hi == np.minimum(lo + 1, len(d) - 1)).all() and (lo >= 0).all()
        np.testing.assert_array_equal(sw.lerp(d[lo], d[hi], t), want)
        np.testing.assert_array_equal([R.percentile(d, q) for q in QS], want)
        a, b = sw.middle_ranks(len(d))
        assert sw.median_of(d[a], d[b]) == np.median(d)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("dim", [2, 3])
def test_sqrt_of_sorted_keys_is_sorted_pdist(kind, dim):
    for n in SIZES:
        P = R.make_points(kind, n, dim, seed=100 + n)
        d2, i, j = R.squared_keys(P)
        np.testing.assert_array_equal(np.sqrt(d2), pdist(P))         # the key is pdist's own arithmetic
        np.testing.assert_array_equal(np.sqrt(np.sort(d2)), R.sorted_pdist(P))
        far = R.farthest_pair(P)
        assert far[0] < far[1] and d2[(i == far[0]) & (j == far[1])][0] == d2.max()


def test_farthest_pair_takes_the_smallest_of_equal_ones():
    P = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 0.0], [3.0, 4.0], [1.0, 1.0]])
    assert R.farthest_pair(P) == (0, 1)
    assert R.farthest_pair(P[::-1]) == (1, 2)
    assert R.farthest_pair(P[:1]) == (-1, -1)


def test_slab_is_closed_and_follows_the_axis():
    pts = np.array([[0.0, 5.0, 0.0], [1.0, 6.0, 1.25], [2.0, 7.0, 1.5], [3.0, 8.0, 1.75], [4.0, 9.0, 1.76]])
    np.testing.assert_array_equal(sw.slab_indices(pts, 1.5, 0.25, 2), [1, 2, 3])
    np.testing.assert_array_equal(R.slab(pts, 1.5, 0.25, 2), [1, 2, 3])
    np.testing.assert_array_equal(sw.slab_indices(pts, 2.0, 1.0, 0), [1, 2, 3])     # ground = 0 along x
    np.testing.assert_array_equal(sw.slab_indices(pts, 2.0, 1.0, 1), [1, 2, 3])     # ground = 5 along y
    assert sw.plane_axes(2) == [0, 1] and sw.plane_axes(0) == [1, 2] and sw.plane_axes(1) == [0, 2]
    with pytest.raises(ValueError):
        sw.plane_axes(3)
    rng = np.random.default_rng(2)
    cloud = rng.uniform(0, 3, size=(500, 3))
    for axis in range(3):
        np.testing.assert_array_equal(sw.slab_indices(cloud, 1.37, 0.1, axis), R.slab(cloud, 1.37, 0.1, axis))


def test_without_a_pair_everything_is_zero_and_no_device_is_needed():
    for n in (0, 1):
        P = np.ones((n, 2))
        assert sw.pairwise_distance_quantiles(P, 95) == 0.0
        np.testing.assert_array_equal(sw.pairwise_distance_quantiles(P, [5, 50]), [0.0, 0.0])
    out = sw.pairwise_distance_quantiles(np.ones((2, 3)), [50, 95], seg_start=[0, 1, 1, 2])
    np.testing.assert_array_equal(out, np.zeros((3, 2)))
    res = hip.pdist_select(np.ones((2, 2)), [0, 1, 2], [[-1, -1], [-1, -1]])
    np.testing.assert_array_equal(res.values, np.zeros((2, 2)))
    np.testing.assert_array_equal(res.n_pairs, [0, 0])
    np.testing.assert_array_equal(res.max_pair, [[-1, -1], [-1, -1]])
    assert res.stats == {"pairs": 0, "pair_evaluations": 0, "passes": 0}

    pts = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 1.4], [0.0, 0.2, 3.0]])
    w = sw.width_at_height(pts, nb_neighbors=None)
    assert w["n_points"] == 1 and w["n_pairs"] == 0 and w["max_pair"] == (-1, -1) and w["seed"] is None
    assert w["width"] == w["p90"] == w["p95"] == w["median"] == w["max_width"] == 0.0
    np.testing.assert_array_equal(w["bounds"], np.zeros(3))
    prof = sw.width_profile(pts, [1.37, 2.0, 9.0], nb_neighbors=None)
    np.testing.assert_array_equal(prof["n_points"], [1, 0, 0])
    np.testing.assert_array_equal(prof["width"], np.zeros(3))
    np.testing.assert_array_equal(prof["max_pair"], np.full((3, 2), -1))
    np.testing.assert_array_equal(prof["bounds"], np.zeros((3, 3)))


def test_file_content_dict_form():
    pts = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 1.4], [0.0, 0.2, 3.0]])
    content = {"seed": "tree_7", "src": None, "clean_pcd": PointCloud(pts), "shift_one": None}
    w = sw.width_at_height(content, nb_neighbors=None)
    assert w["seed"] == "tree_7" and w["n_points"] == 1
    assert sw.width_at_height(content, nb_neighbors=None, seed=3)["seed"] == 3
    assert sw.width_at_height(content, height=3.0, nb_neighbors=None)["n_points"] == 1     # the argument counts


def test_bad_arguments_are_refused_before_any_device():
    P = np.arange(12.0).reshape(6, 2)                                 # 15 pairs
    for pts, seg, ranks in [(P, [0, 6], [[15]]), (np.zeros((3, 4)), [0, 3], [[0]]),
                            (P, [0, 6], [list(range(15)) * 2 + [0, 1, 2]]), (P, [0, 5], [[0]]), (P, [1, 6], [[0]]),
                            (P, [0, 1, 6], [[0], [0]])]:
        with pytest.raises(_lib.PyQSMHipError) as e:
            hip.pdist_select(pts, seg, ranks)
        assert e.value.code == -1
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.pdist_select(P, [0, 6], [[0]], max_pairs=14)
    assert e.value.code == -4
    with pytest.raises(ValueError):
        sw.pairwise_distance_quantiles(P, 101)


@pytest.mark.skipif(_lib.device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_gpu_means_an_error_not_a_fallback():
    with pytest.raises(_lib.PyQSMHipError) as e:
        sw.pairwise_distance_quantiles(np.arange(12.0).reshape(6, 2), 95)
    assert e.value.code == -3
