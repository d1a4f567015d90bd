"""pyqsm_radius_reduce against tests/voxelgrid_restatement.py on an MI355X: the values of a
12 500-point cloud reduced over the neighbours of the 50 000 points of its tree, bit for bit."""
import numpy as np
import pytest

from pyqsm_amd import hip
from pyqsm_amd.geometry.cloud import PointCloud
from tests import voxelgrid_restatement as R
from tests import wave_select_cases

pytestmark = pytest.mark.gpu

REDUCERS = ["mean", "min", "max", "first"]
CASES = [(0.05, 500), (0.05, 8), (0.3, 64)]


def _values(F, seed=0):
    _, _, comp = R.detail_inputs()
    return np.random.default_rng(seed).normal(0.0, 3.0, (len(comp), F))


def _neighbours(radius, k):
    """The restated neighbour lists, with the branches the case is there for populated."""
    idx, cnt, in_range = R.detail_neighbours(radius, k)
    assert (cnt == 0).mean() >= 0.005
    if (radius, k) == (0.05, 500):
        assert not (in_range > k).any()
    else:
        assert (in_range > k).mean() >= 0.10
    return idx, cnt


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("radius,k", CASES)
@pytest.mark.parametrize("F", [1, 5])
def test_reductions_equal_restatement_bit_for_bit(gpu, radius, k, F):
    _, tree, comp = R.detail_inputs()
    idx, cnt = _neighbours(radius, k)
    vals = _values(F)
    for reducer in REDUCERS:
        out, got_cnt = hip.radius_reduce(comp, tree, vals, radius, k=k, reducer=reducer, empty_row=0,
                                         return_counts=True)
        assert np.array_equal(got_cnt, cnt), reducer
        assert _same_bits(out, R.reduce_values(idx, cnt, vals, reducer, 0)), reducer


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("k", [64, 512])
def test_clumps_on_both_sides_of_k_the_step_and_the_padding(gpu, jitter, k):
    """Queries with exactly 1 ... 700 sources in range (tests/wave_select_cases.py): k - 1, k and k + 1 of
    them at k = 64 and 512; one query finds nothing. No row has a tie at the k-th place
    (tests/test_wave_select_host.py), so the restatement's (d2, index) order settles every row."""
    src, size = wave_select_cases.clumps(jitter=jitter)
    qry = wave_select_cases.clump_queries(src)
    idx, cnt, _ = R.neighbours(src, qry, wave_select_cases.RADIUS, k)
    assert np.array_equal(cnt, np.r_[np.minimum(size, k), 0])
    vals = np.random.default_rng(k).normal(0.0, 3.0, (len(src), 3))
    for reducer in ("mean", "first"):
        out, got_cnt = hip.radius_reduce(src, qry, vals, wave_select_cases.RADIUS, k=k, reducer=reducer, empty_row=0,
                                         return_counts=True)
        assert np.array_equal(got_cnt, cnt), reducer
        assert _same_bits(out, R.reduce_values(idx, cnt, vals, reducer, 0)), reducer


def test_sixty_four_columns(gpu):
    _, tree, comp = R.detail_inputs()
    idx, cnt = _neighbours(0.3, 64)
    vals = _values(64, seed=1)
    for reducer in ("mean", "max"):
        out = hip.radius_reduce(comp, tree, vals, 0.3, k=64, reducer=reducer)
        assert _same_bits(out, R.reduce_values(idx, cnt, vals, reducer, 0)), reducer


def test_empty_row_and_one_dimensional_values(gpu):
    _, tree, comp = R.detail_inputs()
    idx, cnt = _neighbours(0.05, 500)
    vals = _values(1)[:, 0]
    a = hip.radius_reduce(comp, tree, vals, 0.05, empty_row=0)
    b = hip.radius_reduce(comp, tree, vals, 0.05, empty_row=-1)
    c = hip.radius_reduce(comp, tree, vals, 0.05, empty_row=77, reducer="first")
    assert a.shape == (len(tree),)
    empty = cnt == 0
    assert (a[empty] == vals[0]).all() and np.isnan(b[empty]).all() and (c[empty] == vals[77]).all()
    assert _same_bits(a[~empty], b[~empty])
    assert _same_bits(b[:, None], R.reduce_values(idx, cnt, vals, "mean", -1))


def test_nan_in_values_propagates(gpu):
    _, tree, comp = R.detail_inputs()
    idx, cnt = _neighbours(0.05, 8)
    vals = _values(2, seed=2)
    vals[::7, 0] = np.nan
    for reducer in REDUCERS:
        out = hip.radius_reduce(comp, tree, vals, 0.05, k=8, reducer=reducer, empty_row=-1)
        want = R.reduce_values(idx, cnt, vals, reducer, -1)
        assert np.array_equal(np.isnan(out), np.isnan(want)), reducer
        assert np.array_equal(out[~np.isnan(want)], want[~np.isnan(want)]), reducer
    touched = np.isnan(vals[:, 0])[np.where(idx < len(comp), idx, 0)] & (idx < len(comp))
    assert np.array_equal(np.isnan(hip.radius_reduce(comp, tree, vals, 0.05, k=8, reducer="min")[:, 0])[cnt > 0],
                          touched.any(axis=1)[cnt > 0])


@pytest.mark.parametrize("k", [1, 2048])
def test_smallest_and_largest_k(gpu, k):
    _, tree, comp = R.detail_inputs()
    qry = tree[:2000]
    radius = 0.05 if k == 1 else 1.0   # 1 m around a trunk point: more than 2048 of the 12 500 in range
    idx, cnt, in_range = R.neighbours(comp, qry, radius, k)
    assert (in_range > k).mean() >= 0.10
    vals = _values(3, seed=3)
    for reducer in ("mean", "first"):
        out, got = hip.radius_reduce(comp, qry, vals, radius, k=k, reducer=reducer, return_counts=True)
        assert np.array_equal(got, cnt)
        assert _same_bits(out, R.reduce_values(idx, cnt, vals, reducer, 0)), reducer


@pytest.mark.parametrize("radius,k", [(0.05, 8), (0.3, 64)])
def test_counts_and_nearest_equal_radius_knn(gpu, radius, k):
    _, tree, comp = R.detail_inputs()
    qry = tree[::5]
    dist, idx = hip.radius_knn(comp, qry, radius, k=k)
    out, cnt = hip.radius_reduce(comp, qry, np.arange(len(comp), dtype=np.float64), radius, k=k, reducer="first",
                                 empty_row=-1, return_counts=True)
    assert np.array_equal(cnt, np.isfinite(dist).sum(axis=1))
    has = cnt > 0
    assert np.array_equal(out[has], idx[has, 0].astype(np.float64)) and np.isnan(out[~has]).all()
    far = hip.radius_reduce(comp, qry, np.arange(len(comp), dtype=np.float64), radius, k=k, reducer="max", empty_row=-1)
    assert np.array_equal(far[has], np.where(np.isfinite(dist), idx, -1).max(axis=1)[has].astype(np.float64))


def test_two_runs_are_identical(gpu):
    _, tree, comp = R.detail_inputs()
    vals = _values(5, seed=4)
    a = hip.radius_reduce(comp, tree, vals, 0.3, k=64)
    b = hip.radius_reduce(comp, tree, vals, 0.3, k=64)
    assert _same_bits(a, b)


def test_transfer_wrappers(gpu):
    from pyqsm_amd.geometry.reconstruction import expand_features_to_orig, transfer_features
    _, tree, comp = R.detail_inputs()
    idx, cnt = _neighbours(0.05, 500)
    vals = _values(2, seed=5)
    data = {"points": comp, "colors": comp, "labels": np.zeros(len(comp)), "linearity": vals[:, 0], "pca1": vals[:, 1]}
    res = expand_features_to_orig(PointCloud(comp), PointCloud(tree), data)
    want = R.reduce_values(idx, cnt, vals, "mean", 0)
    assert sorted(res) == ["features", "points"] and res["points"] is not None
    assert _same_bits(res["features"], want)
    assert _same_bits(transfer_features(comp, vals, tree), want)
    assert _same_bits(transfer_features(comp, vals[:, 0], tree, reducer="first", empty_row=-1)[:, None],
                      R.reduce_values(idx, cnt, vals[:, :1], "first", -1))
