"""The epiphyte split on the GPU (pyqsm_select_values, pyqsm_split_above_dev, pyqsm_shift_components,
pyqsm_kmeans_pp and the wrappers of geometry/epiphytes.py) against the CPU statement of its contract
(tests/epiphyte_restatement.py, itself held to NumPy and scikit-learn by tests/test_epiphyte_host.py).
Every comparison with the restatement is exact."""
import functools
import operator

import numpy as np
import pytest

from pyqsm_amd import hip, synth
from pyqsm_amd.geometry import epiphytes as E
from pyqsm_amd.geometry import stem_width as sw
from pyqsm_amd.geometry.cloud import PointCloud
from pyqsm_amd.math_utils import clustering
from pyqsm_amd.viz.projection import project_by_label
from tests import epiphyte_restatement as R
from tests.test_epiphyte_host import CENTRE_BOUND, GOLDEN_NAMES, golden_case

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 255, 256, 257, 70_001]      # a block is 256 rows; 70 001 rows take more than one round of the grid


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def some_ranks(n, rng, count=8):
    return np.unique(np.concatenate([[0, n - 1, (n - 1) // 2, n // 2], rng.integers(0, n, count)]))


def percentile_gpu(v, q, key=0):
    n = len(v)
    lo, hi, t = sw.percentile_ranks(n, q)
    a, b = hip.select_values(v, [int(lo), int(hi)], key=key)
    return np.float64(sw.lerp(a, b, t))


# ---------------------------------------------------------------- selection

@pytest.mark.parametrize("n", SIZES)
def test_select_sizes(gpu, n):
    rng = np.random.default_rng(n)
    rows = rng.normal(0, 1, (n, 3)) * np.array([1.0, 1e-3, 50.0])
    ranks = some_ranks(n, rng)
    for key in (0, 2, "norm"):
        assert bits(hip.select_values(rows, ranks, key=key)) == bits(R.select(rows, ranks, key))
    z = np.ascontiguousarray(rows[:, 2])                         # [n] values, mixed sign
    assert bits(hip.select_values(z, ranks)) == bits(np.sort(z)[ranks])
    for q in (0, 60, 65, 100):
        assert bits(percentile_gpu(z, q)) == bits(np.percentile(z, q)) == bits(R.percentile(z, q))
        mag = R.keys_of(rows, "norm")
        assert bits(percentile_gpu(rows, q, key="norm")) == bits(np.percentile(mag, q))


def test_select_special_keys(gpu):
    rng = np.random.default_rng(5)
    n = 1000
    ranks = some_ranks(n, rng)
    equal = np.full(n, -7.125)
    assert bits(hip.select_values(equal, ranks)) == bits(equal[ranks])
    negative = -np.abs(rng.normal(0, 3, n)) - 1e-3
    assert bits(hip.select_values(negative, ranks)) == bits(np.sort(negative)[ranks])
    denormal = rng.integers(-2000, 2000, n) * 5e-324
    denormal[denormal == 0] = 5e-324
    assert bits(hip.select_values(denormal, ranks)) == bits(np.sort(denormal)[ranks])
    zeros = rng.normal(0, 1, n)
    zeros[::3] = -0.0
    zeros[1::7] = 0.0
    got = hip.select_values(zeros, np.arange(0, n, 40))
    assert np.array_equal(got, np.sort(zeros)[::40])             # by value: -0.0 is keyed as +0.0
    assert not np.signbit(got[got == 0]).any()
    wide = np.concatenate([rng.normal(0, 1, n), [np.inf, -np.inf, 1e308, -1e308]])
    assert bits(hip.select_values(wide, [0, 1, 2, n + 1, n + 2, n + 3])) == bits(np.sort(wide)[[0, 1, 2, -3, -2, -1]])


def test_select_32_ranks_unused_slots_and_errors(gpu):
    rng = np.random.default_rng(6)
    v = rng.normal(0, 1, (5000, 3))
    ranks = rng.integers(0, 5000, 32)
    ranks[[3, 17]] = -1
    ranks[9] = ranks[8]
    assert bits(hip.select_values(v, ranks, key="norm")) == bits(R.select(v, ranks, "norm"))
    buf = hip.DeviceBuffer.from_array(v)
    assert bits(hip.select_values_dev(buf.ptr, 5000, 3, ranks, key=1)) == bits(R.select(v, ranks, 1))
    buf.free()
    with pytest.raises(ValueError):
        hip.select_values(v, np.arange(33))
    with pytest.raises(ValueError):
        hip.select_values(v, [5000])
    assert hip.select_values(np.zeros((0, 3)), [-1, -1]).tolist() == [0.0, 0.0]
    bad = v.copy()
    bad[4321, 1] = np.nan                                        # not in the key column: "a NaN anywhere"
    with pytest.raises(ValueError):
        hip.select_values(bad, [0], key=0)
    with pytest.raises(ValueError):
        hip.shift_components(bad)


# ---------------------------------------------------------------- the three-way labels

@functools.lru_cache(maxsize=None)
def shift_case():
    shift = R.shift_field(20_000, seed=4)
    shift.setflags(write=False)
    return shift, R.shift_components(shift, 65, 60)


def test_shift_components_equal_the_restatement(gpu):
    shift, (labels, thr, counts) = shift_case()
    got = hip.shift_components(shift, 65, 60)
    assert np.array_equal(got.labels, labels)
    assert bits(got.thresholds) == bits(thr)
    assert got.counts.tolist() == counts.tolist() == np.bincount(labels, minlength=3).tolist()
    assert got.counts.sum() == len(shift)
    d_shift = hip.DeviceBuffer.from_array(shift)
    d_lab = hip.DeviceBuffer(len(shift))
    thr_d, counts_d = hip.shift_components_dev(d_shift.ptr, len(shift), d_lab.ptr, 65, 60)
    assert bits(thr_d) == bits(thr) and counts_d.tolist() == counts.tolist()
    assert np.array_equal(d_lab.download((len(shift),), np.uint8), labels)
    d_shift.free()
    d_lab.free()
    for small in (shift[:1], shift[:2], shift[:257], np.ones((9, 3))):
        got, want = hip.shift_components(small, 65, 60), R.shift_components(small, 65, 60)
        assert np.array_equal(got.labels, want[0]) and got.counts.tolist() == want[2].tolist()
        assert np.array_equal(got.thresholds, want[1], equal_nan=True)
    empty = hip.shift_components(np.zeros((0, 3)))
    assert empty.counts.tolist() == [0, 0, 0] and np.isnan(empty.thresholds).all()


def test_chained_splits_equal_the_one_call_form(gpu):
    shift, (labels, thr, _) = shift_case()
    pts = np.random.default_rng(1).uniform(0, 10, shift.shape)
    c_mag = R.keys_of(shift, "norm")
    high_idx, high, low = E.split_on_percentile(PointCloud(pts), c_mag, 65)
    assert np.array_equal(high_idx, np.nonzero(labels > 0)[0])
    assert np.array_equal(high.points, pts[labels > 0]) and np.array_equal(low.points, pts[labels == 0])
    z_mag = shift[high_idx][:, 2]
    leaf_idx, leaves, epis = E.split_on_percentile(high, z_mag, 60)
    assert np.array_equal(high_idx[leaf_idx], np.nonzero(labels == 1)[0])
    assert np.array_equal(leaves.points, pts[labels == 1]) and np.array_equal(epis.points, pts[labels == 2])
    # a comparison the device does not know runs on the host with the device's percentile
    host_idx = E.split_on_percentile(pts, c_mag, 65, comp=lambda x, y: x > y)[0]
    assert np.array_equal(host_idx, high_idx)
    for comp in (operator.ge, operator.lt, operator.le):
        assert np.array_equal(E.split_on_percentile(pts, c_mag, 65, comp=comp)[0],
                              np.where(comp(c_mag, np.percentile(c_mag, 65)))[0])
    low2, high2 = E.split_on_pct(pts, 65, shift=shift)
    assert np.array_equal(high2.points, high.points) and np.array_equal(low2.points, low.points)
    low3, high3 = E.split_on_pct(pts, 65, cmag=c_mag)
    assert np.array_equal(high3.points, high.points) and np.array_equal(low3.points, low.points)
    with pytest.raises(ValueError):
        E.split_on_percentile(pts, c_mag[:-1], 65)


# ---------------------------------------------------------------- k-means

def same_fit(got, want):
    assert np.array_equal(got.seeds, want.seeds)
    assert got.n_iter == want.n_iter
    assert np.array_equal(got.labels, want.labels)
    assert bits(got.centres) == bits(want.centres)
    assert bits(got.inertia) == bits(want.inertia)
    assert got.n_empty == want.n_empty


KMEANS_SHAPES = [(1, 1, 3), (20, 20, 3), (255, 20, 3), (256, 20, 3), (257, 20, 3), (513, 64, 3), (3000, 20, 3),
                 (2000, 2, 1), (3000, 5, 2)]


@pytest.mark.parametrize("n,k,d", KMEANS_SHAPES)
def test_kmeans_shapes(gpu, n, k, d):
    x = R.cloud("tree", n, d, seed=n + k)
    first, u = clustering.kmeanspp_draws(n, k, seed=k)
    got = hip.kmeans_pp(x, k, first, u)
    same_fit(got, R.kmeans_pp(x, k, first, u))
    assert got.labels.dtype == np.int32 and got.centres.shape == (k, d)


def test_kmeans_zero_potential_and_empty_centres(gpu):
    x = R.cloud("few", 300, seed=3)
    first, u = clustering.kmeanspp_draws(300, 8, 0)
    got, want = hip.kmeans_pp(x, 8, first, u), R.kmeans_pp(x, 8, first, u)
    same_fit(got, want)
    assert got.n_empty >= 3 and got.n_empty == 8 - len(np.unique(got.labels))
    assert 0 in got.seeds[5:]                                    # pot == 0 selects point 0
    fit = clustering.kmeans_pp(x, 8, seed=0)
    assert fit.n_empty_ == got.n_empty and np.array_equal(fit.labels_, got.labels)


def test_kmeans_lattice_ties(gpu):
    x = R.cloud("lattice", 1000, seed=9)
    first, u = clustering.kmeanspp_draws(1000, 20, 1)
    same_fit(hip.kmeans_pp(x, 20, first, u), R.kmeans_pp(x, 20, first, u))


def test_kmeans_max_iter_tol_and_errors(gpu):
    x = R.cloud("box", 1500, seed=2)
    first, u = clustering.kmeanspp_draws(1500, 20, 0)
    for kw in ({"max_iter": 1}, {"max_iter": 3}, {"tol": 0.0}, {"tol": 0.05}, {"max_iter": 40, "tol": 0.0}):
        got, want = hip.kmeans_pp(x, 20, first, u, **kw), R.kmeans_pp(x, 20, first, u, **kw)
        same_fit(got, want)
    assert hip.kmeans_pp(x, 20, first, u, max_iter=1).n_iter == 1
    with pytest.raises(ValueError):
        clustering.kmeans_pp(x[:5], 8)                            # n < k
    with pytest.raises(ValueError):
        hip.kmeans_pp(x, 65, 0, np.zeros(64 * 6))
    with pytest.raises(ValueError):
        hip.kmeans_pp(x, 20, first, u[:-1])


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_kmeans_against_sklearn_goldens(gpu, name):
    x, k, seed, g = golden_case(name)
    fit = clustering.kmeans_pp(x, k, seed=seed)
    assert np.array_equal(fit.labels_, g[f"{name}_labels"])
    assert np.array_equal(fit.seed_indices_, g[f"{name}_seeds"])
    assert fit.n_iter_ == int(g[f"{name}_n_iter"])
    assert np.abs(fit.cluster_centers_ - g[f"{name}_centres"]).max() <= CENTRE_BOUND
    assert fit.n_empty_ == 0


def test_kmeans_dev_form_and_repeat(gpu):
    x = R.cloud("tree", 3000, 3, seed=21)
    first, u = clustering.kmeanspp_draws(3000, 20, 5)
    a = hip.kmeans_pp(x, 20, first, u)
    b = hip.kmeans_pp(x, 20, first, u)
    buf = hip.DeviceBuffer.from_array(x)
    c = hip.kmeans_pp_dev(buf.ptr, 3000, 3, 20, first, u)
    buf.free()
    for other in (b, c):
        same_fit(other, a)


def test_kmeans_feature(gpu):
    x, k, seed, g = golden_case("feature")
    idxs, feats = clustering.kmeans_feature(x[:, 0], seed=seed)
    assert len(idxs) == 2
    for v in (0, 1):
        assert np.array_equal(idxs[v], np.where(g["feature_labels"] == v)[0])
        assert np.array_equal(feats[v], x[idxs[v], 0])


# ---------------------------------------------------------------- the driver

def test_project_components_is_the_composition_of_its_parts(gpu):
    pts = synth.tree_unit(seed=3, n=30_000)
    labels = R.shift_components(R.shift_field(len(pts), seed=8))[0]
    wood, leaves, epis = (PointCloud(pts[labels == v]) for v in (0, 1, 2))
    kw = dict(voxel_size=0.1, n_clusters=20, every=4, alpha=0.4)
    got = E.project_components_in_clusters(None, None, epis, leaves, wood, "t3", include_epis=True, **kw)
    assert list(got) == ["t3"] and set(got["t3"]) == {"epi_clusters", "leaf_clusters", "wood_clusters"}
    for cloud, name in ((epis, "epi_clusters"), (leaves, "leaf_clusters"), (wood, "wood_clusters")):
        vox = hip.voxel_down_sample(cloud.points, 0.1)[0]
        first, u = clustering.kmeanspp_draws(len(vox), 20, 0)
        want = project_by_label(vox, R.kmeans_pp(vox, 20, first, u).labels, 0.4, every=4)["total_area"]
        assert bits(got["t3"][name]) == bits(want)
        assert want > 0
    plain = E.project_components_in_clusters(None, None, epis, leaves, wood, "t3", **kw)["t3"]
    assert set(plain) == {"leaf_clusters", "wood_clusters"}
    idx = E.area_indices(got, pca=20.0)
    m = got["t3"]
    assert idx["EAI"] == m["epi_clusters"] / 20.0
    assert idx["LAI_proposed"] == (m["wood_clusters"] + m["leaf_clusters"]) / 20.0
    assert idx["LAI"] == ((m["wood_clusters"] + m["leaf_clusters"]) + m["epi_clusters"]) / 20.0


def test_identify_epiphytes_on_a_contraction_shift(gpu):
    from pyqsm_amd.geometry.skeletonize import extract_skeleton
    pts = synth.tree_unit(seed=1, n=5000)
    _, _, steps = extract_skeleton(PointCloud(pts), max_iter=1, debug=True)
    content = {"seed": 7, "src": PointCloud(pts), "clean_pcd": PointCloud(pts), "shift_one": steps[0]}
    out = E.identify_epiphytes(content, voxel_size=0.1, alpha=0.4)
    labels = out["labels"]
    want = R.shift_components(steps[0], 65, 60)
    assert np.array_equal(labels, want[0]) and out["counts"].tolist() == want[2].tolist()
    assert out["counts"].sum() == len(pts) and (out["counts"] > 0).all()
    for v, name in enumerate(("wood", "leaves", "epis")):          # disjoint, and together the input
        assert np.array_equal(out[name].points, pts[labels == v])
    assert set(out["metrics"][7]) == {"epi_clusters", "leaf_clusters", "wood_clusters"}
    assert all(a > 0 for a in out["metrics"][7].values())
    with pytest.raises(ValueError):
        E.identify_epiphytes({**content, "shift_one": None})
