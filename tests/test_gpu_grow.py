"""The device-resident region growing (pyqsm_grow_clusters, grow_seed_clusters, engine="device")
against the index-based restatement (tests/grow_restatement.py, itself pinned to the reference's loop
in tests/test_grow_host.py), against oracle.extend_seed_clusters, and against the host engine."""
import numpy as np
import pytest

import oracle
from pyqsm_amd import hip, synth
from pyqsm_amd._lib import PyQSMHipError
from pyqsm_amd.tree_isolation import extend_seed_clusters, grow_seed_clusters
from tests import grow_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def slab():
    P, seeds = R.slab()
    P.setflags(write=False)
    return P, seeds, R.seed_owner(P, seeds)


@pytest.fixture(scope="module")
def slab_k30(slab):
    P, seeds, owner = slab
    return R.grow(P, owner, seeds, 30, 0.1, 12)


def _labelled(seeds):
    return list(enumerate(seeds))


def _same_as_restatement(res, r):
    assert np.array_equal(res.owner, r.owner)
    assert np.array_equal(res.cycle, r.cycle)
    assert np.array_equal(res.finished, r.finished)
    assert res.stats.tolist() == [len(r.frontiers), sum(r.frontiers), int((r.cycle >= 0).sum()),
                                  max(r.frontiers, default=0)]


def test_slab_matches_restatement_and_reference_loop(gpu, slab, slab_k30):
    P, seeds, _ = slab
    r = slab_k30
    # conditions on the input, not measurements: contested points, queries cut at k, both endings,
    # frontiers on both sides of the query sort's threshold, everything owned within the cycles
    assert r.contested > 0 and r.over_k > 0 and r.small_end > 0 and r.empty_end > 0
    assert min(r.frontiers) < 1024 < max(r.frontiers)
    assert (r.owner >= 0).all() and (r.finished > 0).all()
    res = grow_seed_clusters(_labelled(seeds), P, k=30, max_distance=0.1, cycles=12, device=gpu)
    _same_as_restatement(res, r)
    want = oracle.extend_seed_clusters(_labelled(seeds), P, k=30, max_distance=0.1, cycles=12)
    want = {label: {tuple(p) for p in pts} for label, pts in want.items()}
    assert R.clusters_as_sets(P, seeds, res.owner, res.cycle, res.labels) == want


def test_slab_without_a_cut_at_k(gpu, slab):
    P, seeds, owner = slab
    r = R.grow(P, owner, seeds, 200, 0.1, 12)
    assert r.over_k == 0 and r.contested > 0
    res = grow_seed_clusters(_labelled(seeds), P, k=200, max_distance=0.1, cycles=12, device=gpu)
    _same_as_restatement(res, r)


@pytest.mark.parametrize("cycles,finished,counts", [(200, [31, 1, 1, 0], [366, 5, 7, 0]),
                                                    (10, [-1, 1, 1, 0], [132, 5, 7, 0])])
def test_mixed_endings(gpu, cycles, finished, counts):
    src, seeds = R.mixed()
    res = grow_seed_clusters(_labelled(seeds), src, k=40, max_distance=0.05, cycles=cycles, device=gpu)
    assert res.finished.tolist() == finished
    assert [int((res.owner == i).sum()) for i in range(4)] == counts
    _same_as_restatement(res, R.grow(src, R.seed_owner(src, seeds), seeds, 40, 0.05, cycles))


@pytest.mark.parametrize("columns,counts,finished", [(199, [600, 594], [50, 50]), (61, [186, 180], [16, 15])])
def test_contested_column_goes_to_the_lower_cluster(gpu, columns, counts, finished):
    src, seeds = R.contested_strip(columns)
    res = grow_seed_clusters(_labelled(seeds), src, k=40, max_distance=0.05, cycles=200, device=gpu)
    assert [int((res.owner == i).sum()) for i in range(2)] == counts
    assert res.finished.tolist() == finished
    middle = np.flatnonzero(src[:, 0] == (columns // 2) * 0.02)
    assert len(middle) == 6 and (res.owner[middle] == 0).all()
    assert len(set(res.cycle[middle].tolist())) == 1            # reached by both in the same cycle
    r = R.grow(src, R.seed_owner(src, seeds), seeds, 40, 0.05, 200)
    assert r.contested == 6
    _same_as_restatement(res, r)


def _engines_agree(seeds, src, gpu, **kw):
    host_pcds, host_nbrs = extend_seed_clusters(seeds, src, "t", device=gpu, engine="host", **kw)
    dev_pcds, dev_nbrs = extend_seed_clusters(seeds, src, "t", device=gpu, engine="device", **kw)
    assert len(dev_pcds) == len(host_pcds)
    for a, b in zip(dev_pcds, host_pcds):
        assert np.array_equal(a.points, b.points)               # row order included
    assert dev_nbrs == host_nbrs
    return host_nbrs


def test_engines_agree_on_the_slab(gpu, slab):
    P, seeds, _ = slab
    _engines_agree(_labelled(seeds), P, gpu, k=30, max_distance=0.1, cycles=12)


def test_engines_agree_on_the_strips(gpu):
    src, seeds = R.mixed()
    for cycles in (200, 10):
        _engines_agree([("wide", seeds[0]), ("thin", seeds[1]), ("alone", seeds[2]), ("none", seeds[3])], src, gpu,
                       k=40, max_distance=0.05, cycles=cycles)
    for columns in (199, 61, 200):
        src, seeds = R.contested_strip(columns)
        named = [("a", seeds[0]), ("b", seeds[1])]
        _engines_agree(named, src, gpu, k=40, max_distance=0.05, cycles=200)
    nbrs = _engines_agree(named, src, gpu, k=40, max_distance=0.05, cycles=200,
                          exclude_pts=np.array([[2.0, 0.05, 0]]))           # an exclusion zone
    assert sum(len(a) for a in nbrs) < len(src) - 24


@pytest.mark.parametrize("columns", [199, 61, 200])
def test_engines_agree_under_ties_at_the_kth_distance(gpu, columns):
    """Grid points, k = 8: a query has itself, four points at 0.02 and FOUR at 0.02 * sqrt(2) in reach
    for the three places left, so walk order decides (compared between the engines only: SciPy's
    choice is unspecified)."""
    src, seeds = R.contested_strip(columns)
    _engines_agree([("a", seeds[0]), ("b", seeds[1])], src, gpu, k=8, max_distance=0.05, cycles=200)


@pytest.mark.parametrize("k,cycles,include_seeds", [(50, 25, True), (8, 40, False)])
def test_engines_agree_on_the_forest(gpu, k, cycles, include_seeds):
    P = synth.forest(100_000, seed=1)
    low = P[P[:, 2] < 0.3]
    lab, _ = hip.dbscan(low, 0.1, 10, device=gpu)
    seeds = [(f"tree{c}", low[lab == c]) for c in range(lab.max() + 1)]
    src = P if include_seeds else P[P[:, 2] >= 0.3]
    nbrs = _engines_agree(seeds, src, gpu, k=k, max_distance=0.1, cycles=cycles)
    assert sum(len(a) for a in nbrs) > 5000
    res = grow_seed_clusters(seeds, src, k=k, max_distance=0.1, cycles=cycles, device=gpu)
    assert res.finished.tolist() == [-1, -1] and res.stats[0] == cycles     # the cycle cap ended it


def test_same_bits_twice_and_for_any_seed_order(gpu, slab, slab_k30):
    P, seeds, _ = slab
    first = grow_seed_clusters(_labelled(seeds), P, k=30, max_distance=0.1, cycles=12, device=gpu)
    again = grow_seed_clusters(_labelled(seeds), P, k=30, max_distance=0.1, cycles=12, device=gpu)
    rng = np.random.default_rng(5)
    shuffled = [s[rng.permutation(len(s))] for s in seeds]
    other = grow_seed_clusters(_labelled(shuffled), P, k=30, max_distance=0.1, cycles=12, device=gpu)
    for res in (first, again, other):
        assert np.array_equal(res.owner, slab_k30.owner)
        assert np.array_equal(res.cycle, slab_k30.cycle)
        assert np.array_equal(res.finished, slab_k30.finished)


def test_edges(gpu):
    src, seeds = R.mixed()
    owner = R.seed_owner(src, seeds)
    q = np.concatenate(seeds)
    ql = np.concatenate([np.full(len(s), i, dtype=np.int32) for i, s in enumerate(seeds)])
    own, cyc, fin, stats = hip.grow_clusters(src, owner, q, ql, 4, 0.05, k=40, cycles=0, device=gpu)
    assert np.array_equal(own, owner) and (cyc == -1).all() and fin.tolist() == [-1, -1, -1, 0] and not stats.any()
    own, cyc, fin, stats = hip.grow_clusters(src, owner, q[:0], ql[:0], 4, 0.05, k=40, device=gpu)
    assert np.array_equal(own, owner) and (cyc == -1).all() and fin.tolist() == [0, 0, 0, 0]
    own, cyc, fin, stats = hip.grow_clusters(src[:0], owner[:0], q, ql, 4, 0.05, k=40, device=gpu)
    assert len(own) == 0 and fin.tolist() == [1, 1, 1, 0]
    with pytest.raises(PyQSMHipError):
        hip.grow_clusters(src, owner, q, np.where(ql == 2, 4, ql), 4, 0.05, k=40, device=gpu)
    # k larger than the source: nothing is ever cut
    r = R.grow(src, owner, seeds, 1000, 0.05, 200)
    own, cyc, fin, stats = hip.grow_clusters(src, owner, q, ql, 4, 0.05, k=1000, cycles=200, device=gpu)
    assert np.array_equal(own, r.owner) and np.array_equal(cyc, r.cycle) and np.array_equal(fin, r.finished)
    # one cluster
    s = R.strip(61)
    res = grow_seed_clusters([("only", s[:12])], s, k=40, max_distance=0.05, cycles=200, device=gpu)
    r = R.grow(s, R.seed_owner(s, [s[:12]]), [s[:12]], 40, 0.05, 200)
    assert (res.owner == 0).all() and res.finished.tolist() == r.finished.tolist()
    assert np.array_equal(res.cycle, r.cycle)
    assert res.indices(0).tolist() == sorted(np.flatnonzero(r.cycle >= 0), key=lambda j: (r.cycle[j], j))
