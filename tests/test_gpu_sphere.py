"""Branch tracing on the GPU against the restatement (tests/sphere_restatement.py): Lloyd, the
silhouette and the fused k-means selection bit-exact, the excluded ball query, the k-means branch
of choose_and_cluster, and branch_tracing.sphere_step on a synthetic tree: the same branches,
id_to_num and cylinders, the same bits on every run, one upload of the cloud per call."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from pyqsm_amd import branch_tracing, hip, synth
from pyqsm_amd.math_utils import clustering, fit
from tests import sphere_restatement as R

pytestmark = pytest.mark.gpu


def _cloud(seed, m, k):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-1, 1, (k, 3))
    lab = rng.integers(0, k, m)
    return centers[lab] + rng.normal(0, 0.25, (m, 3))


@pytest.mark.parametrize("m", [3, 100, 1000, 10_007, 50_000])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_lloyd_bit_exact(gpu, m, k):
    P = _cloud(m + k, m, k)
    init = clustering.krandinit(P[:, :2], k, np.random.default_rng(k))
    cent, labels = hip.kmeans(P, init, 10, device=gpu)
    want_c, want_l = R.lloyd(P[:, :2], init, 10)
    assert np.array_equal(labels, want_l)
    assert np.array_equal(cent, want_c)
    c2, l2 = clustering.kmeans2(P[:, :2], k, seed=k, device=gpu)
    assert np.array_equal(c2, cent) and np.array_equal(l2, labels)


@pytest.mark.parametrize("m,k", [(3, 2), (500, 3), (5000, 4), (4099, 8)])
def test_silhouette_bit_exact(gpu, m, k):
    P = _cloud(m, m, k)
    labels = np.random.default_rng(m).integers(0, k, m)
    score, present, samples = hip.silhouette(P, labels, k, return_samples=True, device=gpu)
    want, want_present = R.silhouette_samples(P, labels, k)
    assert present == want_present
    assert np.array_equal(samples, want)
    assert score == R.chunk_sum(want) / m
    if 2 <= present <= m - 1:
        assert score == clustering.silhouette_score(P, labels, device=gpu)


def test_silhouette_large_and_gaps(gpu):
    m, k = 50_000, 6
    P = _cloud(1, m, 4)
    labels = np.random.default_rng(2).integers(0, 4, m)
    labels[labels == 2] = 5            # label 2 and 4 empty
    labels[123] = 4                    # then 4 a singleton
    score, present, samples = hip.silhouette(P, labels, k, return_samples=True, device=gpu)
    assert present == 5
    rows = np.r_[0, 123, np.random.default_rng(3).choice(m, 200, replace=False), m - 1]
    want, _ = R.silhouette_samples(P, labels, k, rows=rows)
    assert np.array_equal(samples[rows], want)
    assert samples[123] == 0.0
    assert score == R.chunk_sum(samples) / m


def test_silhouette_invalid_labellings(gpu):
    P = _cloud(4, 10, 2)
    for labels in (np.zeros(10, int), np.arange(10)):
        score, present, samples = hip.silhouette(P, labels, int(labels.max()) + 1, return_samples=True,
                                                 device=gpu)
        assert score == 0.0 and not np.any(samples) and not 2 <= present <= 9


@pytest.mark.parametrize("m", [3, 40, 2000, 12_345, 50_000])
@pytest.mark.parametrize("k0", [1, 2, 5])
def test_kmeans_select_bit_exact(gpu, m, k0):
    P = _cloud(m, m, 3)
    rng = np.random.default_rng(m + k0)
    inits = [clustering.krandinit(P[:, :2], k0 + q, rng) for q in range(4)]
    labels, scores, present = hip.kmeans_select(P, k0, inits, device=gpu)
    for q in range(4):
        _, want_l = R.lloyd(P[:, :2], inits[q], 10)
        assert np.array_equal(labels[q], want_l)
        if m <= 2000:
            want_s, want_p = R.silhouette(P, want_l, k0 + q)
            assert scores[q] == want_s and present[q] == want_p
        else:
            s, p = hip.silhouette(P, want_l, k0 + q, device=gpu)
            assert scores[q] == s and present[q] == p
    got = clustering.kmeans(P, k0, seed=7, device=gpu)
    want = R.kmeans(P, k0, np.random.default_rng(7))
    assert got[0] == want[0]
    assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1])) and len(got[1]) == len(want[1])


def test_excluded_ball_query(gpu):
    P = synth.tree_unit(3, 30_000)
    rng = np.random.default_rng(0)
    found0 = rng.choice(len(P), 9000, replace=False)
    tracer = branch_tracing.SphereTracer(P, found0, device=gpu)
    tree = cKDTree(P)
    mask = np.zeros(len(P), bool)
    mask[found0] = True
    try:
        for center, r in [((0.0, 0.0, 1.0), 0.5), ((0.3, 0.0, 3.0), 1.5), ((9.0, 9.0, 9.0), 0.1),
                          (tuple(P[5]), 0.0)]:
            got = tracer.ball(center, r)
            want = np.array(sorted(tree.query_ball_point(center, r)), dtype=np.int64)
            want = want[~mask[want]] if len(want) else want
            assert np.array_equal(got, want)
            assert np.array_equal(tracer.nn_xyz.download((len(got), 3), np.float64), P[got])
            tracer.mark(got[::2])
            mask[got[::2]] = True
    finally:
        tracer.free()


def test_choose_and_cluster_kmeans_returns_main_cloud_indices(gpu):
    rng = np.random.default_rng(5)
    blobs = np.concatenate([c + rng.normal(0, 0.03, (400, 3)) for c in ([0, 0, 0], [1, 0, 0], [0, 1, 0])])
    P = np.concatenate([rng.uniform(-5, 5, (3000, 3)), blobs])
    new_neighbors = np.sort(np.r_[rng.choice(3000, 50, replace=False), 3000 + np.arange(1200)])
    labels, clusters = fit.choose_and_cluster(new_neighbors, P, "kmeans", seed=11, device=gpu)
    want_labels, want_local = R.kmeans(P[new_neighbors], 1, np.random.default_rng(11))
    assert len(clusters) >= 2 and labels == want_labels
    for c, w in zip(clusters, want_local):
        assert np.array_equal(c, new_neighbors[w])
        assert np.isin(c, new_neighbors).all()
    assert sorted(np.concatenate(clusters).tolist()) == new_neighbors.tolist()


def _trace(P, seed_idx, seed, last_radius=0.3, **kw):
    return branch_tracing.sphere_step(P[seed_idx].copy(), last_radius, P, seed_idx, total_found=list(seed_idx),
                                      seed=seed, **kw)


def _same_trace(a, b):
    br_a, id_a, cyl_a, det_a = a
    br_b, id_b, cyl_b, det_b = b
    assert len(br_a) == len(br_b)
    assert list(br_a[0][0]) == list(br_b[0][0])
    assert list(br_a[0][1:]) == list(br_b[0][1:])
    for x, y in zip(br_a[1:], br_b[1:]):
        assert list(x) == list(y)
    assert dict(id_a) == dict(id_b)
    assert len(det_a) == len(det_b) and len(cyl_a) == len(cyl_b)
    for x, y in zip(det_a, det_b):
        for key in ("center", "axis", "height", "radius"):
            assert np.array_equal(np.asarray(x[key]), np.asarray(y[key])), key


@pytest.fixture(scope="module")
def tree():
    P = synth.tree_unit(0, 20_000)
    r = np.hypot(P[:, 0], P[:, 1])
    return P, np.flatnonzero((P[:, 2] < 0.3) & (r < 0.5))


# 0.3: the trunk's radius, the fits are good and the steps cluster with DBSCAN; 0.05: the first fits
# are wider than the radius bound allows, so those steps cluster with k-means
@pytest.mark.parametrize("last_radius", [0.3, 0.05])
def test_sphere_step_equals_restatement(gpu, tree, monkeypatch, last_radius):
    P, seed_idx = tree
    calls = {"kmeans": 0}
    real = hip.kmeans_select_dev

    def counted(*a, **k):
        calls["kmeans"] += 1
        return real(*a, **k)
    monkeypatch.setattr(hip, "kmeans_select_dev", counted)
    got = _trace(P, seed_idx, 1, last_radius, device=gpu)
    want = R.sphere_step(P[seed_idx].copy(), last_radius, P, seed_idx, total_found=list(seed_idx), seed=1)
    assert got != []
    assert calls["kmeans"] > 0 or last_radius > 0.1
    _same_trace(got, want)
    found = np.asarray(got[0][0][0])
    assert len(found) == len(np.unique(found))


def test_sphere_step_reproducible_and_one_upload(gpu, tree, monkeypatch):
    P, seed_idx = tree
    uploads = []
    real = hip.DeviceBuffer.upload

    def counted(self, a):
        uploads.append(np.asarray(a).nbytes)
        return real(self, a)
    monkeypatch.setattr(hip.DeviceBuffer, "upload", counted)
    hip.prof_enable(1, gpu)
    hip.prof_reset(gpu)
    spheres = []
    try:
        a = _trace(P, seed_idx, 2, spheres=spheres, device=gpu)
        steps = hip.prof_get("ball_excl", gpu)[1]
    finally:
        hip.prof_enable(0, gpu)
    b = _trace(P, seed_idx, 2, device=gpu)
    _same_trace(a, b)
    assert uploads.count(P.nbytes) == 2              # once per call
    assert steps == len(spheres) > 10                # one ball per step, no re-upload
