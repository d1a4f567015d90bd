"""The shared grid (pyqsm_amd/csrc/grid.hip) through every size class of its cell directory, through
the public wrappers and against the references the suite already trusts.

The number of cells decides which binning kernels run (tests/grid_restatement.py states the rule):
the fused class (every other test), a separate scan of the bucket totals from 2^24 cells, buckets of
8192 cells from 2^26, one atomic per point from 2^27 up to the 2^28 the dense grid may have; axis
compression and a doubled edge beyond that. Directory size does not depend on the point count, so
clumps of a few ten thousand points in a wide box at eps (or a query radius of) 0.02 reach every
class. Each test asserts from the restatement that its cloud is in the class it claims, with the
bucket and cell populations it claims (tests/test_grid_restatement_host.py does the same without a
GPU). Labels and core flags are oracle.dbscan's; the fixed-radius results are cKDTree's; adjacency,
features and normals are their restatements'. No tolerance beyond those of the tests they copy.
"""
import functools
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

import oracle
from pyqsm_amd import hip, synth
from pyqsm_amd.geometry.reconstruction import get_neighbors_kdtree
from tests import adjacency_restatement as RA
from tests import features_restatement as RF
from tests import grid_restatement as G
from tests import normals_restatement as RN
from tests.test_gpu_adjacency import assert_same as assert_same_adjacency
from tests.test_gpu_dbscan_buckets import slab as one_bucket_slab_of_dbscan
from tests.test_gpu_features import _check as check_features
from tests.test_gpu_normals import _same as same_bits

pytestmark = pytest.mark.gpu

LARGE = ("scan", "bucket13", "atomic")
ENV = ("PYQSM_DBSCAN_PLAN", "PYQSM_COORD_F32", "PYQSM_DBSCAN_BIN", "PYQSM_GRID_BIN")


class _env:
    """Sets the library's switches for one call and puts back what was there."""

    def __init__(self, **kv):
        self.kv = {"PYQSM_" + k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        self.keep = {k: os.environ.pop(k, None) for k in ENV}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _dbscan(P, eps, min_pts, gpu, host=False, f64=False, bin=None):
    """(labels, core, 'hit' | 'miss') of one call."""
    with _env(DBSCAN_PLAN="host" if host else None, COORD_F32="0" if f64 else None, DBSCAN_BIN=bin):
        hip.prof_enable(True, gpu)
        hip.prof_reset(gpu)
        lab, core = hip.dbscan(P, eps, min_pts, device=gpu)
        hit = hip.prof_get("dbscan_plan_hit", gpu)[1]
        miss = hip.prof_get("dbscan_plan_miss", gpu)[1]
        hip.prof_enable(False, gpu)
    assert hit + miss == 1
    return lab, core, "hit" if hit else "miss"


def _prime_fused_hint(gpu):
    """A host-planned call on a tiny fp32 cloud: the context's hint is then a small fused directory."""
    P = np.array([[0.0, 0.0, 0.0], [0.0625, 0.0, 0.0], [0.0, 0.0625, 0.0]])
    assert _dbscan(P, 0.1, 2, gpu, host=True)[2] == "miss"


@functools.lru_cache(maxsize=None)
def _cloud(kind, key, nudge=False):
    """(points, oracle labels, oracle core flags, eps, min_pts), computed once and shared."""
    if kind == "class":
        P, eps, mp = G.class_cloud(key, nudge=nudge), G.EPS, G.MIN_PTS
    elif kind == "threshold":
        P, eps, mp = G.threshold_cloud(key), G.EPS, G.MIN_PTS
    elif kind == "dashed":
        P, eps, mp = G.dashed_diagonal(key, nudge=nudge), G.EPS, G.MIN_PTS
    elif kind == "forest":
        P, eps, mp = synth.forest(key), 0.1, 10
    elif kind == "bigcell":
        P, eps, mp = G.big_cell_cloud(), 0.1, 10
    else:
        assert kind == "mapped"
        P, eps, mp = G.axis_mapped_cloud(), 0.03, 4
    lab, core = oracle.dbscan(P, eps, mp)
    for a in (P, lab, core):
        a.setflags(write=False)
    return P, lab, core, eps, mp


def _expect(cloud, gpu, runs):
    """runs: (name, keyword arguments of _dbscan, expected planning or None) in a row on one cloud."""
    P, lab0, core0, eps, mp = cloud
    for name, kw, path in runs:
        lab, core, got = _dbscan(P, eps, mp, gpu, **kw)
        assert np.array_equal(core, core0), name
        assert np.array_equal(lab, lab0), name
        if path is not None:
            assert got == path, name


# ---- DBSCAN: one cloud per class -------------------------------------------------------------------

@pytest.mark.parametrize("cls", LARGE)
def test_dbscan_one_cloud_per_class(gpu, cls):
    """Host-planned, planned by default twice in a row after a fused hint, and with fp64 records.
    The separate-scan class misses (the hint's `fused` differs) and then hits: the device writes a
    plan with hint.fused == 0. Buckets of 8192 cells and the atomic fallback are left to the host."""
    cloud = _cloud("class", cls)
    G.claim_class_cloud(cloud[0], cls)
    lab0 = cloud[1]
    assert lab0.max() + 1 > 1000 and 0.02 < (lab0 < 0).mean() < 0.5 and 0.3 < cloud[2].mean() < 0.95
    _expect(cloud, gpu, [("host", dict(host=True), "miss")])
    _prime_fused_hint(gpu)
    second = "hit" if cls == "scan" else "miss"
    _expect(cloud, gpu, [("default", {}, "miss"), ("default again", {}, second),
                         ("fp64 records", dict(f64=True), "miss")])


@pytest.mark.parametrize("cls", LARGE)
def test_dbscan_class_cloud_not_representable_in_fp32(gpu, cls):
    """One coordinate moved by 1e-9: the whole cloud keeps fp64 records (k_bk_sort<., false>)."""
    cloud = _cloud("class", cls, True)
    G.claim_class_cloud(cloud[0], cls)
    _expect(cloud, gpu, [("host", dict(host=True), "miss"), ("default", {}, "miss")])


@pytest.mark.parametrize("cls", LARGE)
def test_dbscan_state_left_behind(gpu, cls):
    """After a call in a large class the hint, the arena and the zeroed counters are in order: a
    forest on the same context gets the oracle's labels."""
    _expect(_cloud("class", cls), gpu, [("large", {}, None)])
    _expect(_cloud("forest", 20_000), gpu, [("forest", {}, None), ("forest again", {}, None)])


# ---- DBSCAN: either side of every threshold ----------------------------------------------------------

@pytest.mark.parametrize("dims", list(G.THRESHOLD_DIMS), ids=lambda d: "x".join(map(str, d)))
def test_dbscan_grid_on_either_side_of_every_threshold(gpu, dims):
    """Two corner points pin the directory's dimensions; clumps inside, 24 points in the last y row
    of the last z slab. A host-planned grid of 4096-cell buckets leaves a hint that fits itself."""
    cloud = _cloud("threshold", dims)
    pl = G.claim_threshold_cloud(cloud[0], dims)
    assert cloud[1][0] == -1 and cloud[1][-1] == -1, "the corner points are noise"
    _expect(cloud, gpu, [("host", dict(host=True), "miss"),
                         ("default", {}, "hit" if pl.bits == 12 else "miss")])


# ---- DBSCAN: compression into a large directory --------------------------------------------------------

@pytest.mark.parametrize("cls", LARGE)
def test_dbscan_compressed_axes_with_a_large_directory(gpu, cls):
    """A dashed diagonal: the dense grid would exceed 2^28 cells, the compressed one lands in `cls`
    (k_bk_hist<1>, k_cell_count_oct<true>). Compressed grids are always planned on the host."""
    cloud = _cloud("dashed", cls)
    G.claim_dashed(cloud[0], cls)
    assert cloud[1].max() + 1 >= 80
    _expect(cloud, gpu, [("host", dict(host=True), "miss"), ("default", {}, "miss"),
                         ("host, fp64 records", dict(host=True, f64=True), "miss"),
                         ("default, fp64 records", dict(f64=True), "miss")])
    nudged = _cloud("dashed", cls, True)
    G.claim_dashed(nudged[0], cls)
    _expect(nudged, gpu, [("not representable", {}, "miss")])


# ---- DBSCAN: the binning switches, at small size -------------------------------------------------------

@pytest.mark.parametrize("bin", ["atomic"])
@pytest.mark.parametrize("kind,key", [("forest", 30_000), ("bigcell", None), ("mapped", None)])
def test_dbscan_binning_switches(gpu, kind, key, bin):
    """PYQSM_DBSCAN_BIN=atomic (one atomic per point) on a forest, on cells of more than 255 points
    and on a compressed grid."""
    cloud = _cloud(kind, key)
    _expect(cloud, gpu, [(bin, dict(bin=bin), "miss"), (bin + ", fp64 records", dict(bin=bin, f64=True), "miss")])


# ---- build_grid's classes through its consumers --------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tree(cls):
    P = _cloud("class", cls)[0]
    return P, cKDTree(P), G.radius_plan(P, G.EPS)


def _kdtree_union(tree, n, qry, dist, k):
    d, i = tree.query(qry, k=k, distance_upper_bound=dist)
    i = np.atleast_2d(i.reshape(len(qry), -1))
    return np.unique(i[i < n]), (i < n).sum(axis=1)


@pytest.mark.parametrize("f64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("cls", LARGE)
def test_radius_queries_in_every_class(gpu, cls, f64):
    """radius_mark, the padded tables and ball_query over a source grid of each large class, as
    tests/test_gpu_radius.py compares them with cKDTree; 3000 queries are served in cell order
    (keys of up to 28 bits), 500 in the caller's."""
    P, tree, rp = _tree(cls)
    n = len(P)
    assert (rp.cls, rp.doubled) == (cls, False) and not G.robust_box_cuts(P)
    assert G.populations(rp)[1] > 500                       # more neighbours than the cap somewhere
    with _env(COORD_F32="0" if f64 else None):
        for m in (3000, 500):
            qry = G.query_set(P, rp, m, seed=m)
            G.claim_queries(qry, P, rp)
            for k in (500, 7):
                mask, counts = hip.radius_mark(P, qry, G.EPS, k=k, device=gpu)
                want_idx, want_counts = _kdtree_union(tree, n, qry, G.EPS, k)
                assert np.array_equal(counts, want_counts), (m, k)
                assert np.array_equal(np.flatnonzero(mask), want_idx), (m, k)
                assert counts.max() == k and (counts == 0).sum() >= 6
            k = 8
            d0, i0 = tree.query(qry, k=k, distance_upper_bound=G.EPS)
            d, i = get_neighbors_kdtree(P, query_pts=qry, dist=G.EPS, k=k, return_pcd=False, device=gpu)
            assert d.shape == d0.shape and i.dtype == np.int64
            assert np.array_equal(d, d0)                       # includes the inf padding
            assert np.array_equal(np.isinf(d), i == n)
            for r in np.flatnonzero(~(i == i0).all(1)):        # ties in distance may be ordered differently
                assert sorted(zip(d[r], i[r])) == sorted(zip(d0[r], i0[r]))
        mn, mx = P.min(0), P.max(0)
        blob = P[np.argmax(tree.query_ball_point(P[::50], G.EPS, return_length=True)) * 50]
        for center in (mx - 0.004, mn + 0.004, blob, mx + [0.01, 0.0, 0.0], mx + 50.0):
            got = hip.ball_query(P, center, G.EPS, device=gpu)
            assert np.array_equal(got, np.sort(tree.query_ball_point(center, G.EPS)))
        assert len(hip.ball_query(P, mx - 0.004, G.EPS, device=gpu)) >= 8


@pytest.mark.parametrize("cls", ["bucket13", "atomic"])
def test_cluster_adjacency_in_the_large_classes(gpu, cls):
    P = _cloud("class", cls)[0]
    lab = np.unique(np.floor(P).astype(np.int64), axis=0, return_inverse=True)[1].reshape(-1).astype(np.int64)
    src = np.random.default_rng(5).random(len(P)) < 1.0 / 3.0
    s, sl, t, tl = P[src], lab[src], P[~src], lab[~src]
    rp = G.radius_plan(t, G.EPS)                            # the grid is built over the targets
    assert (rp.cls, rp.doubled) == (cls, False) and not G.robust_box_cuts(t)
    ref = RA.adjacency(s, sl, t, tl, G.EPS, witness=True)
    assert len(ref) > 500 and sum(v[1] for v in ref.values()) > 500_000
    assert_same_adjacency(hip.cluster_adjacency(s, sl, G.EPS, t, tl, return_pairs=True), ref, witness=True)


@pytest.mark.parametrize("cls", ["bucket13", "atomic"])
def test_features_in_the_large_classes(gpu, cls):
    P, _, rp = _tree(cls)
    assert (rp.cls, rp.doubled) == (cls, False) and not G.robust_box_cuts(P)
    got, cnt = hip.geometric_features(P, G.EPS, return_counts=True, device=gpu)
    last = rp.ncell - 1 - (rp.dims[0] * rp.dims[1] + rp.dims[0] + 1)
    q = np.union1d(np.arange(0, len(P), 10), np.flatnonzero(rp.cells == last))
    want, wcnt, lam = RF.compute_features(P, G.EPS, qidx=q)
    assert wcnt.max() > 1000
    assert np.array_equal(cnt[q], wcnt)
    check_features(got[q], want, lam)


@pytest.mark.parametrize("cls", ["bucket13", "atomic"])
def test_normals_in_the_large_classes(gpu, cls):
    P = G.class_cloud(cls, light=True)                      # (the restatement takes 0.5 s on it)
    rp = G.radius_plan(P, G.EPS)
    assert (rp.cls, rp.doubled) == (cls, False) and not G.robust_box_cuts(P)
    assert G.populations(rp)[1] > 128
    same_bits(hip.estimate_normals(P, G.EPS, 30, device=gpu), RN.estimate_normals(P, G.EPS, 30))


# ---- PYQSM_GRID_BIN=atomic, at small size ----------------------------------------------------------------

def test_knn_on_the_atomic_grid(gpu, monkeypatch):
    """tests/test_gpu_knn.py::test_against_oracle[20000-8-False] with build_grid's atomic path."""
    monkeypatch.setenv("PYQSM_GRID_BIN", "atomic")
    P = synth.forest(20_000, seed=2)
    idx, d2 = hip.knn(P, 8, False, device=gpu)
    idx0, d20 = oracle.knn(P, 8, False)
    assert np.array_equal(d2, d20)
    assert np.array_equal(idx, idx0)


def test_knn_ties_on_the_atomic_grid(gpu, monkeypatch):
    """tests/test_gpu_knn.py::test_quantised_coordinates_have_ties_at_the_kth_place at k = 20: the
    fine grid keeps fp64 arrays, and kNN's coarse retry grid is gathered from it (coarsen_grid with
    fine.p4 == nullptr)."""
    monkeypatch.setenv("PYQSM_GRID_BIN", "atomic")
    P = np.round(synth.forest(40_000, seed=12) * 200.0) / 200.0          # 5 mm grid
    idx, d2 = hip.knn(P, 20, True, device=gpu)
    idx0, d20 = oracle.knn(P, 20, True)
    assert float((d20[:, 1:] == d20[:, :-1]).any(axis=1).mean()) > 0.01
    assert np.array_equal(d2, d20) and np.array_equal(idx, idx0)


def test_radius_mark_on_the_atomic_grid(gpu, monkeypatch):
    """tests/test_gpu_radius.py::test_radius_mark_matches_ckdtree[0.3-40]."""
    monkeypatch.setenv("PYQSM_GRID_BIN", "atomic")
    src = synth.forest(30_000, seed=1)
    qry = synth.forest(30_000, seed=1)[::37] + [0.01, -0.02, 0.005]
    mask, counts = hip.radius_mark(src, qry, 0.3, k=40, device=gpu)
    want_idx, want_counts = _kdtree_union(cKDTree(src), len(src), qry, 0.3, 40)
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(np.flatnonzero(mask), want_idx)
    assert counts.max() == 40


# ---- build_grid's second level across the register tile's capacity -------------------------------------

@pytest.mark.parametrize("f64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("m", G.ONE_BUCKET_SIZES)
def test_radius_queries_on_one_bucket_of_m_points(gpu, m, f64):
    """tests/test_gpu_dbscan_buckets.py::test_one_bucket_of_m_points for k_bk_sort_plain, which shares
    the two sweeps with DBSCAN's k_bk_sort: the same slab, all of it in one bucket of build_grid's
    directory, on either side of the 6144 points a block keeps in registers."""
    P = G.one_bucket_slab(m)
    assert np.array_equal(P, one_bucket_slab_of_dbscan(m))
    G.claim_one_bucket_slab(P, m)
    tree, r = cKDTree(P), G.ONE_BUCKET_RADIUS
    qry = P[::7]
    with _env(COORD_F32="0" if f64 else None):
        mask, counts = hip.radius_mark(P, qry, r, k=40, device=gpu)
        want_idx, want_counts = _kdtree_union(tree, m, qry, r, 40)
        assert np.array_equal(counts, want_counts)
        assert np.array_equal(np.flatnonzero(mask), want_idx)
        for center in (0.5 * (P.min(0) + P.max(0)), P.max(0) - 0.004):
            got = hip.ball_query(P, center, r, device=gpu)
            assert np.array_equal(got, np.sort(tree.query_ball_point(center, r)))
