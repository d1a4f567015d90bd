"""Plane segmentation on the GPU against tests/plane_restatement.py.

Shapes: n in {1, 63, 1024, 1025, 2500} straddles the 64-lane wave and the 1024-point tile of the count,
H in {1, 257, 300} the 256-lane block; m = 3 and m = 10 take the two constructions. Tolerances:
unit normals within 1e-12 and d within 1e-9 * extent (those of test_gpu_ransac.py for axes and
centres); counts, selections, inlier sets, labels and the order-free refit are compared exactly.
"""
import math

import numpy as np
import pytest

from pyqsm_amd import hip
from pyqsm_amd.geometry import cleaning
from pyqsm_amd.geometry.cloud import PointCloud
from pyqsm_amd.geometry import point_cloud_processing as pcp
from pyqsm_amd.geometry.point_cloud_processing import cluster_plus
from pyqsm_amd.math_utils import fit
from tests import plane_restatement as R

pytestmark = pytest.mark.gpu

THRESH = 0.04
DEFAULT_P = 0.99999999


def _patch(n, seed=1):
    """n points of a 2 x 2 patch of the plane z = 0.1 x + 0.2 y, sigma 0.01 along z."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, 2, n), rng.uniform(0, 2, n)
    return np.ascontiguousarray(np.stack([x, y, 0.1 * x + 0.2 * y + rng.normal(0, 0.01, n)], axis=1))


def _same_planes(got, want, extent):
    got, want = np.asarray(got).reshape(-1, 4), np.asarray(want).reshape(-1, 4)
    assert got.shape == want.shape
    np.testing.assert_array_equal((got == 0).all(axis=1), (want == 0).all(axis=1))  # the same rows are invalid
    assert np.abs(got[:, :3] - want[:, :3]).max(initial=0.0) <= 1e-12
    assert np.abs(got[:, 3] - want[:, 3]).max(initial=0.0) <= 1e-9 * extent


@pytest.fixture(scope="module")
def scene():
    return R.scene(0)


@pytest.fixture(scope="module")
def patch():
    return _patch(2500)


@pytest.fixture(scope="module")
def patch_planes(gpu, patch):
    """300 device hypotheses on the patch; row 7 invalid (a repeated point)."""
    smp = fit.draw_plane_samples(len(patch), 300, 3, seed=2)
    smp[7] = [5, 5, 9]
    planes = hip.plane_models(patch, smp, device=gpu)
    assert (planes[7] == 0).all() and (planes[:7] != 0).any(axis=1).all()
    return planes


@pytest.mark.parametrize("m", [3, 10])
@pytest.mark.parametrize("n,H", [(63, 1), (63, 257), (1025, 300), (2500, 257)])
def test_models_match_the_restatement(gpu, patch, n, H, m):
    P = patch[:n]
    smp = fit.draw_plane_samples(n, H, m, seed=n + H + m)
    got = hip.plane_models(P, smp, device=gpu)
    _same_planes(got, R.models(P, smp), 2.0)
    assert np.abs(np.linalg.norm(got[:, :3], axis=1) - 1).max() <= 1e-12
    assert ((got[:, 2] > 0) | ((got[:, 2] == 0) & (got[:, 1] > 0))).all()


def test_models_of_one_point(gpu):
    P = np.array([[0.5, -1.0, 2.0]])
    for m in (3, 10):
        smp = np.zeros((2, m), dtype=np.int64)
        _same_planes(hip.plane_models(P, smp, device=gpu), R.models(P, smp), 2.0)
    assert (hip.plane_models(P, np.zeros((2, 3), dtype=np.int64), device=gpu) == 0).all()


def test_invalid_hypotheses_give_zero_rows(gpu):
    P = np.array([[0.0, 0, 0], [1.0, 1, 1], [2.0, 2, 2], [0.0, 1, 0], [1.0, 0, 0]])
    smp = np.array([[0, 1, 2], [0, 0, 3], [3, 3, 3], [0, 1, 5], [-1, 1, 3], [0, 4, 3], [2**40, 1, 3]], dtype=np.int64)
    got = hip.plane_models(P, smp, device=gpu)
    np.testing.assert_array_equal(got[[0, 1, 2, 3, 4, 6]], np.zeros((6, 4)))  # collinear, repeated, out of range
    np.testing.assert_array_equal(got[5], [0.0, 0.0, 1.0, 0.0])
    wide = np.tile(np.arange(5, dtype=np.int64), (3, 2))
    wide[1, 9] = 5
    wide[2, 0] = -3
    got = hip.plane_models(P, wide, device=gpu)
    assert (got[0] != 0).any() and (got[1:] == 0).all()
    np.testing.assert_array_equal(hip.plane_count(P, np.zeros((3, 4)), 10.0, device=gpu), [0, 0, 0])


@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 2500])
@pytest.mark.parametrize("H", [1, 257, 300])
def test_counts_are_bit_exact(gpu, patch, patch_planes, n, H):
    planes = patch_planes[:H]  # row 7 is invalid
    for thresh in (0.01, 0.05):
        got = hip.plane_count(patch[:n], planes, thresh, device=gpu)
        np.testing.assert_array_equal(got, R.count(patch[:n], planes, thresh))
    assert H == 1 or got[7] == 0
    assert n < 63 or got.max() > 0


def test_threshold_is_strict(gpu):
    t = 0.125
    below = math.nextafter(t, 0.0)
    P = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 1, 0],
                  [3.0, 1, t], [2.0, 5, -t], [1.0, 1, below], [4.0, 2, -below], [0.0, 0, math.nextafter(t, 1.0)]])
    smp = np.array([[0, 1, 2]], dtype=np.int64)
    planes = hip.plane_models(P, smp, device=gpu)
    np.testing.assert_array_equal(planes, [[0.0, 0.0, 1.0, 0.0]])
    assert hip.plane_count(P, planes, t, device=gpu)[0] == 5
    _, hyp, inl, best, used = hip.segment_plane(P, smp, t, device=gpu)
    np.testing.assert_array_equal(inl, [0, 1, 2, 5, 6])
    np.testing.assert_array_equal(hyp, [0.0, 0.0, 1.0, 0.0])
    assert (best, used) == (0, 1)


@pytest.mark.parametrize("m", [3, 10])
@pytest.mark.parametrize("probability", [0.5, DEFAULT_P, 1.0])
def test_single_plane_end_to_end_and_early_stop(gpu, scene, m, probability):
    P, kind = scene
    H = 300
    smp = fit.draw_plane_samples(len(P), H, m, seed=40 + m)
    planes = hip.plane_models(P, smp, device=gpu)
    got_fit, got_hyp, inl, best, used = hip.segment_plane(P, smp, THRESH, probability, device=gpu)
    w_best, w_used, w_inl, w_hyp = R.segment(P, planes, THRESH, probability, m)
    assert (best, used) == (w_best, w_used) and best >= 0
    np.testing.assert_array_equal(inl, w_inl)
    np.testing.assert_array_equal(got_hyp, planes[best])
    extent = float((P.max(axis=0) - P.min(axis=0)).max())
    _same_planes(got_fit, R.refit(P, inl), extent)
    if probability == 1.0:
        assert used == H
    if m == 3 and probability == 0.5:
        assert used < H  # the ground holds 60 % of the cloud: a handful of rows are enough


def test_nothing_found(gpu, patch):
    P = patch[:100]
    dead = np.tile(np.array([[4, 4, 9]], dtype=np.int64), (20, 1))
    fitp, hyp, inl, best, used = hip.segment_plane(P, dead, THRESH, device=gpu)
    assert best == -1 and used == 20 and len(inl) == 0 and (fitp == 0).all() and (hyp == 0).all()
    fitp, hyp, inl, best, used = hip.segment_plane(P, np.zeros((0, 3), dtype=np.int64), THRESH, device=gpu)
    assert best == -1 and used == 0 and len(inl) == 0 and (fitp == 0).all() and (hyp == 0).all()
    seg = hip.segment_planes(P, np.zeros((3, 0, 3), dtype=np.uint64), THRESH, device=gpu)
    assert len(seg) == 0 and (seg.labels == -1).all() and len(seg.rest()) == 100


def test_peeling_stops_when_fewer_points_than_samples_are_left(gpu):
    # four points on z = 0 and one far above: whatever is drawn, round 0 takes the four or nothing
    P = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 1, 0], [1.0, 1, 0], [0.5, 0.5, 50.0]])
    draws = fit.draw_u64((4, 64, 3), seed=1)
    seg = hip.segment_planes(P, draws, 0.01, probability=1.0, min_inliers=4, device=gpu)
    assert len(seg) == 1 and seg.counts[0] == 4
    np.testing.assert_array_equal(seg.labels, [0, 0, 0, 0, -1])
    np.testing.assert_array_equal(seg.planes[0], [0.0, 0.0, 1.0, 0.0])


def test_refit_does_not_depend_on_the_order_of_the_points(gpu, scene):
    P, _ = scene
    smp = fit.draw_plane_samples(len(P), 300, 3, seed=8)
    base = hip.segment_plane(P, smp, THRESH, device=gpu)
    again = hip.segment_plane(P, smp, THRESH, device=gpu)
    for a, b in zip(base, again):
        np.testing.assert_array_equal(a, b)
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(P))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(P))
        got = hip.segment_plane(np.ascontiguousarray(P[perm]), inv[smp], THRESH, device=gpu)
        assert got[0].tobytes() == base[0].tobytes()  # plane_fit: the same bits
        assert got[1].tobytes() == base[1].tobytes()
        np.testing.assert_array_equal(got[2], np.sort(inv[base[2]]))
        assert got[3:] == base[3:]


def _compose(P, draws, thresh, probability, min_inliers, m, gpu, axis=None, cos_limit=0.0):
    """Round by round on the host: pyqsm_segment_plane on the compacted alive cloud."""
    n, rounds = len(P), len(draws)
    labels = np.full(n, -1, dtype=np.int32)
    out = {"fit": [], "hyp": [], "counts": [], "best": [], "used": []}
    for r in range(rounds):
        alive = np.flatnonzero(labels < 0)
        if len(alive) < m:
            break
        smp = R.local_samples(draws[r], len(alive))
        fitp, hyp, inl, best, used = hip.segment_plane(np.ascontiguousarray(P[alive]), smp, thresh, probability,
                                                       axis=axis, cos_limit=cos_limit, device=gpu)
        if best < 0 or len(inl) < min_inliers:
            out["last"] = len(inl)
            break
        labels[alive[inl]] = r
        for key, v in zip(("fit", "hyp", "counts", "best", "used"), (fitp, hyp, len(inl), best, used)):
            out[key].append(v)
    return labels, out


@pytest.mark.parametrize("seed", [0, 1])
def test_peeling_on_the_scene(gpu, scene, seed):
    P, kind = scene
    draws = fit.draw_u64((4, 256, 3), seed=seed)
    seg = hip.segment_planes(P, draws, THRESH, min_inliers=200, device=gpu)
    assert len(seg) == 2  # stops in the third round
    g, w = seg.indices(0), seg.indices(1)
    assert (kind[g] == 0).sum() >= 1490
    assert len(w) >= 650 and (kind[w] == 1).all()
    np.testing.assert_array_equal(np.bincount(seg.labels[seg.labels >= 0], minlength=2), seg.counts)
    assert len(seg.rest()) == len(P) - seg.counts.sum()
    assert seg.planes[0, 2] > 0.99 and abs(seg.planes[1, 0]) > 0.99
    labels, want = _compose(P, draws, THRESH, DEFAULT_P, 200, 3, gpu)
    assert want["last"] < 200
    np.testing.assert_array_equal(seg.labels, labels)
    assert seg.planes.tobytes() == np.array(want["fit"]).tobytes()
    assert seg.hypothesis_planes.tobytes() == np.array(want["hyp"]).tobytes()
    np.testing.assert_array_equal(seg.counts, want["counts"])
    np.testing.assert_array_equal(seg.best, want["best"])
    np.testing.assert_array_equal(seg.used, want["used"])


def test_peeling_with_ten_samples_equals_the_composition(gpu, scene):
    P, _ = scene
    draws = fit.draw_u64((3, 257, 10), seed=4)
    seg = hip.segment_planes(P, draws, THRESH, probability=1.0, min_inliers=50, device=gpu)
    labels, want = _compose(P, draws, THRESH, 1.0, 50, 10, gpu)
    np.testing.assert_array_equal(seg.labels, labels)
    assert len(seg) == len(want["fit"]) >= 1
    assert seg.planes.tobytes() == np.array(want["fit"]).tobytes()
    np.testing.assert_array_equal(seg.used, want["used"])


def test_cone(gpu):
    rng = np.random.default_rng(6)
    wall = np.stack([10.5 + rng.normal(0, 0.01, 700), rng.uniform(0, 10, 700), rng.uniform(0, 4, 700)], axis=1)
    ground = np.stack([rng.uniform(0, 10, 300), rng.uniform(0, 10, 300), rng.normal(0, 0.01, 300)], axis=1)
    perm = rng.permutation(1000)
    P = np.ascontiguousarray(np.concatenate([wall, ground])[perm])
    on_ground = np.flatnonzero(perm >= 700)
    draws = fit.draw_u64((1, 256, 3), seed=2)
    free = hip.segment_planes(P, draws, THRESH, device=gpu)
    assert len(free) == 1 and abs(free.planes[0, 0]) > 0.99 and free.counts[0] >= 650
    axis = np.array([0.0, 0.0, 1.0])
    cos_limit = math.cos(math.radians(20))
    coned = PointCloud(P).segment_planes(THRESH, max_planes=1, min_inliers=1, num_iterations=256, axis=(0, 0, 2.0),
                                         max_angle_deg=20, draws=draws, device=gpu)
    assert len(coned) == 1 and coned.planes[0, 2] > 0.99 and coned.counts[0] >= 290
    assert abs(coned.hypothesis_planes[0] @ np.append(axis, 0.0)) >= cos_limit
    labels, want = _compose(P, draws, THRESH, DEFAULT_P, 1, 3, gpu, axis=axis, cos_limit=cos_limit)
    np.testing.assert_array_equal(coned.labels, labels)
    smp = fit.draw_plane_samples(len(P), 300, 3, seed=3)
    smp[:50] = on_ground[fit.draw_plane_samples(len(on_ground), 50, 3, seed=4)]  # some inside the cone for sure
    got = hip.plane_models(P, smp, axis=axis, cos_limit=cos_limit, device=gpu)
    _same_planes(got, R.models(P, smp, axis, cos_limit), 10.5)
    valid = (got != 0).any(axis=1)
    assert 50 <= valid.sum() < 300 and (np.abs(got[valid, 2]) >= cos_limit).all()


def test_wrappers(gpu, scene, monkeypatch):
    P, kind = scene
    pcd = PointCloud(P)
    plane, inl = pcd.segment_plane(THRESH, 3, 100, seed=5, device=gpu)
    want = hip.segment_plane(P, fit.draw_plane_samples(len(P), 100, 3, seed=5), THRESH, device=gpu)
    np.testing.assert_array_equal(plane, want[0])
    np.testing.assert_array_equal(inl, want[2])
    assert inl.dtype == np.int64 and len(pcd.select_by_index(inl)) == len(inl)
    seg = pcd.segment_planes(THRESH, max_planes=4, min_inliers=200, num_iterations=256, seed=7, device=gpu)
    ref = hip.segment_planes(P, fit.draw_u64((4, 256, 3), seed=7), THRESH, min_inliers=200, device=gpu)
    np.testing.assert_array_equal(seg.labels, ref.labels)
    np.testing.assert_array_equal(seg.planes, ref.planes)
    np.testing.assert_array_equal(seg.hypothesis_planes, ref.hypothesis_planes)
    np.testing.assert_array_equal(seg.counts, ref.counts)
    monkeypatch.setattr(pcp, "PLANE_SEED", 3)
    got = cluster_plus(P, THRESH, ransac=True, return_pcds=False, device=gpu)
    _, inl10 = pcd.segment_plane(THRESH, 10, 1000, seed=3, device=gpu)
    assert sorted(got) == [-1, 0]
    np.testing.assert_array_equal(got[0], inl10)
    np.testing.assert_array_equal(got[-1], np.setdiff1d(np.arange(len(P)), inl10))
    clouds = cluster_plus(P, THRESH, ransac=True, device=gpu)
    assert [len(c) for c in clouds] == [len(P) - len(inl10), len(inl10)]
    ground, rest, gp = cleaning.split_ground(pcd, distance_threshold=THRESH, max_slope_deg=30, num_iterations=256,
                                             seed=1, device=gpu)
    assert len(ground) + len(rest) == len(P) and len(ground) >= 1490
    assert (R.distance(ground.points, gp) < 2 * THRESH).all() and gp[2] > 0.99
    resid = np.abs(ground.points[:, 2] - (0.05 * ground.points[:, 0] - 0.02 * ground.points[:, 1]))
    assert (resid < 2 * THRESH).mean() > 0.99  # the slab of the slope, not a wedge


def test_many_blocks(gpu):
    n, H = 200_000, 1000
    rng = np.random.default_rng(12)
    x, y = rng.uniform(0, 50, n), rng.uniform(0, 50, n)
    z = np.where(rng.random(n) < 0.5, 0.03 * x + rng.normal(0, 0.02, n), rng.uniform(0, 20, n))
    P = np.ascontiguousarray(np.stack([x, y, z], axis=1))
    smp = fit.draw_plane_samples(n, H, 3, seed=13)
    planes = hip.plane_models(P, smp, device=gpu)
    counts = hip.plane_count(P, planes, 0.1, device=gpu)
    rows = np.concatenate([[0, 255, 256, 999, int(np.argmax(counts))], rng.integers(0, H, 11)])
    np.testing.assert_array_equal(counts[rows], R.count(P, planes[rows], 0.1))
    fitp, hyp, inl, best, used = hip.segment_plane(P, smp, 0.1, 1.0, device=gpu)
    assert best == int(np.argmax(counts)) and used == H
    np.testing.assert_array_equal(inl, np.flatnonzero(R.distance(P, planes[best]) < 0.1))
    _same_planes(fitp, R.refit(P, inl), 50.0)
