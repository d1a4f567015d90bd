"""Region growing without a GPU: the restatement the GPU tests compare against is itself pinned to
the reference's loop (oracle.extend_seed_clusters); the (owner, cycle) -> indices / clouds
reconstruction; the argument errors; the cases pyqsm_grow_clusters answers on the host."""
import numpy as np
import pytest

import oracle
from pyqsm_amd import hip
from pyqsm_amd._lib import PyQSMHipError
from pyqsm_amd.tree_isolation import (extend_seed_clusters, growth_clouds, growth_indices,
                                      labeled_pts_to_lists)
from tests import grow_restatement as R


def _oracle_sets(seeds, src, **kw):
    got = oracle.extend_seed_clusters(list(enumerate(seeds)), src, **kw)
    return {label: {tuple(p) for p in pts} for label, pts in got.items()}


def test_restatement_matches_reference_loop_on_the_slab():
    P, seeds = R.slab()
    r = R.grow(P, R.seed_owner(P, seeds), seeds, 30, 0.1, 12)
    # conditions on the input: every rule of the loop is exercised
    assert r.contested > 0 and r.over_k > 0 and r.small_end > 0 and r.empty_end > 0
    assert (r.finished > 0).all() and (r.owner >= 0).all()
    assert min(r.frontiers) < 1024 < max(r.frontiers)
    want = _oracle_sets(seeds, P, k=30, max_distance=0.1, cycles=12)
    assert R.clusters_as_sets(P, seeds, r.owner, r.cycle, list(range(len(seeds)))) == want


@pytest.mark.parametrize("cycles,finished,counts", [(200, [31, 1, 1, 0], [366, 5, 7, 0]),
                                                    (10, [-1, 1, 1, 0], [132, 5, 7, 0])])
def test_restatement_matches_reference_loop_on_mixed_endings(cycles, finished, counts):
    src, seeds = R.mixed()
    r = R.grow(src, R.seed_owner(src, seeds), seeds, 40, 0.05, cycles)
    assert r.finished.tolist() == finished
    assert [int((r.owner == i).sum()) for i in range(4)] == counts
    want = _oracle_sets(seeds, src, k=40, max_distance=0.05, cycles=cycles)
    assert R.clusters_as_sets(src, seeds, r.owner, r.cycle, list(range(len(seeds)))) == want


def _dict_clouds(seeds, src, owner, cycle):
    """The reference's ownership dict, entry by entry."""
    assigned = {}
    for idc, (_, pts) in enumerate(seeds):
        for p in pts:
            assigned[tuple(p)] = idc
    for c in range(int(cycle.max()) + 1 if len(cycle) else 0):
        for idc in range(len(seeds)):
            for j in np.flatnonzero((cycle == c) & (owner == idc)):
                assigned.setdefault(tuple(src[j]), idc)
    _, pcds = labeled_pts_to_lists(assigned, {i: label for i, (label, _) in enumerate(seeds)}, draw_cycle=True)
    return pcds


def test_indices_and_clouds_from_owner_and_cycle():
    src = np.arange(30, dtype=np.float64).reshape(10, 3)
    #                0   1   2   3   4   5   6   7   8   9
    owner = np.array([1, 0, 0, -1, 1, 0, 1, 1, 0, -1], dtype=np.int32)
    cycle = np.array([1, 0, 2, -1, 0, 0, -1, 1, 2, -1], dtype=np.int32)
    # seed "a" lies outside the source; seed "b" holds source row 6 (owned from the start: cycle -1)
    # and shares the point [100, 100, 100] with "a" (the later seed owns it, at a's place)
    seeds = [("a", np.array([[100.0, 100, 100], [101, 101, 101]])),
             ("b", np.array([src[6], [100.0, 100, 100]]))]
    idx = growth_indices(owner, cycle, 2)
    assert [a.tolist() for a in idx] == [[1, 5, 2, 8], [4, 0, 7]]
    clouds = growth_clouds(seeds, src, owner, cycle)
    assert len(clouds) == 2
    # the shared point is the dict's first key and belongs to "b": b's cloud comes first
    assert clouds[0].points.tolist() == [[100, 100, 100]] + src[[6, 4, 0, 7]].tolist()
    assert clouds[1].points.tolist() == [[101, 101, 101]] + src[[1, 5, 2, 8]].tolist()
    want = _dict_clouds(seeds, src, owner, cycle)
    assert all(np.array_equal(a.points, b.points) for a, b in zip(clouds, want))


def test_clouds_match_the_reference_dict_on_random_growth():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 6, (400, 3)).astype(np.float64)      # many duplicate coordinates
    owner = rng.integers(-1, 5, 400).astype(np.int32)
    cycle = np.where(owner >= 0, rng.integers(-1, 4, 400), -1).astype(np.int32)
    seeds = [(label, rng.integers(0, 7, (m, 3)).astype(np.float64))
             for label, m in (("x", 9), ("y", 0), ("x", 4), ("z", 6), ("w", 5))]   # a label used twice
    got = growth_clouds(seeds, src, owner, cycle)
    want = _dict_clouds(seeds, src, owner, cycle)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.array_equal(a.points, b.points)
    assert growth_clouds([], src, np.full(400, -1, np.int32), np.full(400, -1, np.int32)) == []


def test_engine_argument_errors_come_before_any_device_work():
    P = np.zeros((10, 3))
    with pytest.raises(ValueError, match="order_cutoff"):
        extend_seed_clusters([("a", P[:2])], P, engine="device", order_cutoff=3)
    with pytest.raises(ValueError, match="engine"):
        extend_seed_clusters([("a", P[:2])], P, engine="gpu")


def test_cases_answered_on_the_host():
    src = np.random.default_rng(0).uniform(0, 1, (50, 3))
    owner = np.full(50, -1, dtype=np.int32)
    owner[:3] = 1
    seeds, labels = src[:3], np.array([1, 1, 1], dtype=np.int32)
    own, cyc, fin, stats = hip.grow_clusters(src, owner, seeds, labels, 3, 0.1, cycles=0)       # no cycles
    assert np.array_equal(own, owner) and (cyc == -1).all() and fin.tolist() == [0, -1, 0] and not stats.any()
    own, cyc, fin, stats = hip.grow_clusters(src, owner, np.zeros((0, 3)), [], 3, 0.1)            # no seeds
    assert np.array_equal(own, owner) and (cyc == -1).all() and fin.tolist() == [0, 0, 0] and not stats.any()
    own, cyc, fin, stats = hip.grow_clusters(np.zeros((0, 3)), [], seeds, labels, 3, 0.1)         # empty source
    assert len(own) == 0 and len(cyc) == 0 and fin.tolist() == [0, 1, 0] and stats.tolist() == [1, 3, 0, 3]
    r = R.grow(np.zeros((0, 3)), [], [np.zeros((0, 3)), seeds, np.zeros((0, 3))], 200, 0.1, 150)
    assert r.finished.tolist() == [0, 1, 0]
    for bad in (dict(seed_labels=[1, 3, 1]), dict(seed_labels=[1, -1, 1]), dict(owner=np.full(50, 3)),
                dict(owner=np.full(50, -2)), dict(radius=0.0), dict(radius=np.inf), dict(k=0), dict(min_new=0),
                dict(cycles=-1)):
        kw = dict(src=src, owner=owner, seed_points=seeds, seed_labels=labels, n_clusters=3, radius=0.1)
        kw.update(bad)
        with pytest.raises(PyQSMHipError) as e:                # validation: no device is touched
            hip.grow_clusters(**kw)
        assert e.value.code != -3, bad
