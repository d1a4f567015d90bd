"""The clouds of tests/test_gpu_grid_classes.py, checked without a GPU: every size class of the
grid's directory, both modifiers and either side of every threshold is populated as the GPU tests
claim (tests/grid_restatement.py restates the plan of grid.hip on the CPU)."""
import numpy as np
import pytest

from pyqsm_amd import synth
from tests import grid_restatement as G


def test_size_classes_at_their_bounds():
    assert G.size_class((1 << 24) - 1) == ("fused", 12, 4096)
    assert G.size_class(1 << 24) == ("scan", 12, 4097)
    assert G.size_class((1 << 26) - 1) == ("scan", 12, 16384)
    assert G.size_class(1 << 26) == ("bucket13", 13, 8193)
    assert G.size_class((1 << 27) - 1) == ("bucket13", 13, 16384)
    assert G.size_class(1 << 27) == ("atomic", 13, 16385)
    assert G.tile(12) == 6144 and G.tile(13) == 12288


def test_agrees_with_the_bucket_populations_of_the_buckets_test():
    """The same cells as tests/test_gpu_dbscan_buckets.py::bucket_populations restates them."""
    P = synth.forest(30_000, seed=3)
    pl = G.dbscan_plan(P, 0.1)
    cell = 0.1 * (1.0 + 2.0 ** -20)
    mn, mx = P.min(0), P.max(0)
    raw = (np.floor((mx - mn) / cell) + 1.0).astype(np.int64)
    c = np.clip(np.floor((P - mn) * (1.0 / cell)).astype(np.int64), 0, raw - 1) + 1
    dims = raw + 2
    assert pl.dims == tuple(dims) and (pl.cls, pl.mapped, pl.doubled) == ("fused", False, False)
    assert np.array_equal(pl.cells, (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0])


@pytest.mark.parametrize("cls", ["scan", "bucket13", "atomic"])
def test_class_clouds(cls):
    P = G.class_cloud(cls)
    assert np.array_equal(P.astype(np.float32).astype(np.float64), P)
    pl, rp = G.claim_class_cloud(P, cls)
    Q = G.class_cloud(cls, nudge=True)
    assert (Q != P).sum() == 1 and not np.array_equal(Q.astype(np.float32).astype(np.float64), Q)
    G.claim_class_cloud(Q, cls)
    for m in (3000, 500):
        q = G.query_set(P, rp, m, seed=m)
        assert len(q) == m
        G.claim_queries(q, P, rp)


@pytest.mark.parametrize("dims", list(G.THRESHOLD_DIMS))
def test_threshold_clouds(dims):
    G.claim_threshold_cloud(G.threshold_cloud(dims), dims)


def test_threshold_table_covers_both_sides_of_every_bound():
    got = [G.THRESHOLD_DIMS[d][0] for d in G.THRESHOLD_DIMS]
    assert got == ["fused", "scan", "scan", "bucket13", "bucket13", "atomic", "atomic"]
    assert G.THRESHOLD_NCELL[(645, 645, 645)] <= G.MAX_CELLS < 646 ** 3
    for d, n in G.THRESHOLD_NCELL.items():
        assert d[0] * d[1] * d[2] == n


@pytest.mark.parametrize("cls", ["atomic", "scan", "bucket13"])
def test_dashed_diagonals_compress_into_a_large_directory(cls):
    P = G.dashed_diagonal(cls)
    G.claim_dashed(P, cls)
    G.claim_dashed(G.dashed_diagonal(cls, nudge=True), cls)
    # without the compression the edge would be doubled
    cell = G.EPS * (1.0 + 2.0 ** -20)
    assert np.prod(np.floor((P.max(0) - P.min(0)) / cell) + 3.0) > G.MAX_CELLS


def test_doubled_edge():
    """Points in every slab of a box too large for cells of eps: nothing to compress, the edge doubles."""
    rng = np.random.default_rng(0)
    P = rng.uniform(0, 20.0, (20_000, 3))
    pl = G.dbscan_plan(P, 0.02)
    assert pl.doubled and pl.cell == 2.0 * 0.02 * (1.0 + 2.0 ** -20)
    rp = G.radius_plan(P, 0.02)
    assert rp.doubled and rp.cell == pl.cell


def test_small_clouds_of_the_switch_tests():
    pl = G.dbscan_plan(synth.forest(30_000), 0.1)
    assert (pl.cls, pl.mapped, pl.doubled) == ("fused", False, False)
    pl = G.dbscan_plan(G.big_cell_cloud(), 0.1)
    assert pl.cls == "fused" and G.populations(pl)[1] > G.BK_BIG
    pl = G.dbscan_plan(G.axis_mapped_cloud(), 0.03)
    assert (pl.cls, pl.mapped, pl.doubled) == ("fused", True, False)


@pytest.mark.parametrize("m", G.ONE_BUCKET_SIZES)
def test_one_bucket_slabs_of_the_radius_grid(m):
    """tests/test_gpu_grid_classes.py::test_radius_queries_on_one_bucket_of_m_points: the sizes lie on
    either side of a bucket's 4096 cells and of the register tile of k_bk_sort_plain<12, .>."""
    rp = G.claim_one_bucket_slab(G.one_bucket_slab(m), m)
    assert rp.dims == (402, 5, 3)
    assert {G.tile(12) - 1, G.tile(12), G.tile(12) + 1} <= set(G.ONE_BUCKET_SIZES)


def test_robust_box_restatement_sees_a_cut():
    rng = np.random.default_rng(1)
    P = np.concatenate([rng.uniform(0, 1, (20_000, 3)), [[40.0, 0.5, 0.5]]])
    assert G.robust_box_cuts(P)
    assert not G.robust_box_cuts(P[:-1])
