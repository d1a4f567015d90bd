"""The branch-tracing restatement (tests/sphere_restatement.py) against the libraries it stands for,
no GPU: Lloyd against scipy's kmeans2, the silhouette against sklearn's silhouette_score, the
initial centroids against scipy's _krandinit, pyQSM's kmeans selection with its fixes, and the
restated sphere_step on a synthetic tree (RANSAC through the CPU oracle)."""
import warnings

import numpy as np
import pytest
from scipy.cluster.vq import _krandinit, kmeans2
from sklearn.metrics import silhouette_score as sk_silhouette

import oracle
from pyqsm_amd import hip, synth
from pyqsm_amd.math_utils import clustering
from tests import sphere_restatement as R


def _blobs(seed, k, per, spread=0.05, dim=2):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-3, 3, (k, dim))
    centers[:, 0] += 2.0 * np.arange(k)          # far apart: no point near a Voronoi boundary
    pts = np.concatenate([c + rng.normal(0, spread, (n, dim)) for c, n in zip(centers, per)])
    return pts, centers


@pytest.mark.parametrize("seed,k,per", [(0, 1, [7]), (1, 2, [300, 41]), (2, 3, [1000, 3, 517]),
                                        (3, 5, [4000, 2000, 10, 333, 1200]), (4, 8, [600] * 8)])
def test_lloyd_matches_kmeans2(seed, k, per):
    xy, centers = _blobs(seed, k, per)
    init = centers + np.random.default_rng(seed + 100).normal(0, 0.2, centers.shape)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_c, want_l = kmeans2(xy, init.copy(), iter=10, minit="matrix")
    got_c, got_l = R.lloyd(xy, init, 10)
    assert np.array_equal(got_l, want_l)
    np.testing.assert_allclose(got_c, want_c, rtol=1e-12, atol=0)


def test_lloyd_empty_centroid_keeps_its_place():
    xy, centers = _blobs(5, 2, [200, 300])
    init = np.vstack([centers, [[100.0, 100.0]]])   # nobody is near the third centroid
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_c, want_l = kmeans2(xy, init.copy(), iter=10, minit="matrix")
    got_c, got_l = R.lloyd(xy, init, 10)
    assert np.array_equal(got_l, want_l) and 2 not in got_l
    assert np.array_equal(got_c[2], [100.0, 100.0])
    np.testing.assert_allclose(got_c, want_c, rtol=1e-12, atol=0)


def test_lloyd_returns_the_last_assignment_before_the_last_update():
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [10.0, 0.0], [11.0, 0.0]])
    init = np.array([[0.0, 0.0], [0.9, 0.0]])
    c1, l1 = R.lloyd(xy, init, 1)
    assert np.array_equal(l1, [0, 1, 1, 1]) and np.allclose(c1, [[0.0, 0.0], [22 / 3, 0.0]])
    assert np.array_equal(R.lloyd(xy, init, 1)[1], kmeans2(xy, init.copy(), iter=1, minit="matrix")[1])
    # a tie goes to the lowest centroid
    assert R.vq(np.array([[1.0, 0.0]]), np.array([[0.5, 0.0], [1.5, 0.0]]))[0] == 0


def _sil_case(seed, m, k):
    rng = np.random.default_rng(seed)
    pts = rng.normal(0, 1, (m, 3))
    labels = rng.integers(0, k, m)
    pts += labels[:, None] * 0.7
    return pts, labels


@pytest.mark.parametrize("seed,m,k", [(0, 3, 2), (1, 50, 2), (2, 400, 3), (3, 1500, 4), (4, 700, 8)])
def test_silhouette_matches_sklearn(seed, m, k):
    pts, labels = _sil_case(seed, m, k)
    score, present = R.silhouette(pts, labels, k)
    assert present == len(np.unique(labels))
    assert abs(score - sk_silhouette(pts, labels)) < 1e-10


def test_silhouette_singletons_and_empty_labels():
    pts, labels = _sil_case(7, 300, 3)
    labels[5] = 3                          # a singleton
    labels[labels == 1] = 4                # label 1 empty: the labelling has a gap
    labels[17] = 6                         # another singleton past another gap
    score, present = R.silhouette(pts, labels, 7)
    assert present == 5                     # 0, 2, 3, 4, 6
    assert abs(score - sk_silhouette(pts, labels)) < 1e-10
    s, _ = R.silhouette_samples(pts, labels, 7)
    assert s[5] == 0.0 and s[17] == 0.0


def test_silhouette_invalid_counts():
    pts, _ = _sil_case(8, 10, 2)
    for labels in (np.zeros(10, int), np.arange(10)):   # one label; m labels
        score, present = R.silhouette(pts, labels, int(labels.max()) + 1)
        assert score == 0.0 and not 2 <= present <= 9
        with pytest.raises(ValueError):
            sk_silhouette(pts, labels)
        with pytest.raises(ValueError):
            clustering.silhouette_score(pts, labels)
    labels = np.r_[np.zeros(9, int), 1]                 # m - 1 = 9 is not reached: 2 labels, valid
    assert abs(R.silhouette(pts, labels, 2)[0] - sk_silhouette(pts, labels)) < 1e-10


def test_silhouette_duplicate_points():
    pts = np.repeat(np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]), 5, axis=0)
    labels = np.repeat([0, 1], 5)
    assert abs(R.silhouette(pts, labels, 2)[0] - sk_silhouette(pts, labels)) < 1e-10
    labels = np.r_[0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert abs(R.silhouette(pts, labels, 2)[0] - sk_silhouette(pts, labels)) < 1e-10


@pytest.mark.parametrize("m", [1, 2, 5, 400])
def test_init_draws_match_krandinit(m):
    data = np.random.default_rng(m).normal(0, 1, (m, 2)) * [2.0, 0.5] + [3.0, -1.0]
    for k in (1, 2, 3, 4):
        if m >= 2:
            want = _krandinit(data, k, np.random.default_rng(9), np)
            np.testing.assert_array_equal(clustering.krandinit(data, k, np.random.default_rng(9)), want)
        got = clustering.krandinit(data, k, np.random.default_rng(9))
        np.testing.assert_array_equal(R.krandinit(data, k, np.random.default_rng(9)), got)
        assert got.shape == (k, 2) and np.all(np.isfinite(got))


def test_init_singular_data_takes_the_svd_form():
    data = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [3.0, 3.0]])     # collinear: cov singular
    with pytest.raises(np.linalg.LinAlgError):
        _krandinit(data, 2, np.random.default_rng(0), np)
    got = clustering.krandinit(data, 2, np.random.default_rng(0))
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got[:, 0], got[:, 1])                 # drawn along the line
    np.testing.assert_array_equal(R.krandinit(data, 2, np.random.default_rng(0)), got)
    assert np.array_equal(clustering.krandinit(np.ones((3, 2)), 3, np.random.default_rng(0)), np.ones((3, 2)))


def test_selection_rule():
    m = 6
    lab = np.array([[0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 2, 2], [0, 1, 2, 3, 3, 3]], np.int32)
    ks = [1, 2, 3, 4]
    # the last k above 0.4 wins, and its last label comes back (the reference drops it)
    labels, idxs = clustering.select(ks, lab, [0, 0.9, 0.5, 0.3], [1, 2, 3, 4], m)
    assert labels == [0, 1, 2] and [list(i) for i in idxs] == [[0, 1], [2, 3], [4, 5]]
    # 0.4 itself does not pass; nothing passes: the k = 1 labelling, one cluster
    labels, idxs = clustering.select(ks, lab, [0, 0.4, 0.1, 0.2], [1, 2, 3, 4], m)
    assert labels == [0] and [list(i) for i in idxs] == [list(range(6))]
    # an invalid labelling counts as 0 whatever its score
    labels, _ = clustering.select(ks, lab, [0, 0.9, 0.5, 0.95], [1, 2, 3, m], m)
    assert labels == [0, 1, 2]
    # labels without members are skipped
    labels, idxs = clustering.select([2], np.array([[0, 0, 2, 2, 2, 2]], np.int32), [0.8], [2], m)
    assert labels == [0, 2] and [list(i) for i in idxs] == [[0, 1], [2, 3, 4, 5]]
    # min_clusters > 1 and no score above 0.4: no clusters
    assert clustering.select([2, 3], lab[1:3], [0.1, 0.2], [2, 3], m) == ([], [])
    assert clustering.candidate_ks(1) == [1, 2, 3, 4] and clustering.candidate_ks(-1) == [1, 2]
    with pytest.raises(ValueError):
        clustering.candidate_ks(6)


def test_restated_kmeans_finds_separated_branches():
    pts, _ = _blobs(11, 3, [400, 300, 350], spread=0.05, dim=3)
    labels, idxs = R.kmeans(pts, 1, np.random.default_rng(3))
    assert len(labels) >= 2
    assert sorted(np.concatenate(idxs).tolist()) == list(range(len(pts)))


def _cpu_ransac(points, triples, shape="circle", thresh=0.2, device=0):
    c, a, r, inl, best = oracle.ransac_fit(points, triples, shape, thresh)
    return np.asarray(c), np.asarray(a), float(r), inl, int(best)


def trunk_seed(P):
    r = np.hypot(P[:, 0], P[:, 1])
    return np.flatnonzero((P[:, 2] < 0.3) & (r < 0.5))


def test_restated_sphere_step_on_a_tree(monkeypatch):
    monkeypatch.setattr(hip, "ransac", _cpu_ransac)
    P = synth.tree_unit(0, 20_000)
    seed = trunk_seed(P)
    out = R.sphere_step(P[seed].copy(), 0.3, P, seed, total_found=list(seed), seed=1)
    assert out != []
    branches, id_to_num, cyls, cyl_details = out
    found = np.asarray(branches[0][0])
    assert len(found) == len(np.unique(found)) > len(P) // 2     # no point assigned twice
    assert set(id_to_num) <= set(found.tolist())
    assert len(branches) > 1 and len(cyls) == len(cyl_details)
    # the trace climbs the trunk first (DFS): its first fits are the trunk's, bottom to top
    trunk = cyl_details[:15]
    assert all(np.hypot(*d["center"][:2]) < 0.2 for d in trunk)
    assert np.all(np.diff([d["center"][2] for d in trunk]) > 0)
    radii = np.array([d["radius"] for d in trunk])
    assert np.all(np.abs(radii - 0.30) < 0.03) and abs(np.median(radii) - 0.30) < 0.01
