"""Every input of tests/laplacian_cases.py reaches the kernel class its table entry names, shown on the CPU
with the oracle's own counts (oracle.point_cloud_laplacian_counts: the oracle builds the same fans, the
same cover and the same flips as laplacian.hip, so its bucket and row lengths are the kernel's). Without
this a GPU test could pass on a path it never took: one ring point more or fewer moves a row across a
limit of k_sort_rows.

The last test guards the inputs themselves: a cloud whose sparsity pattern changes under coordinate noise
of 1e-13 sits on a near-tie, where kernel and oracle may legitimately decide differently; such a case is
to be replaced, not excused.

Measured with the oracle: under that noise the values move by about 1e-11 of the largest entry on most
cases and by 1.4e-10 on the hub of 180 (the thinnest wedges)."""
import numpy as np
import pytest
from scipy.sparse import diags

import oracle

from tests import laplacian_cases as lc


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_case_reaches_the_class_its_entry_names(case):
    bucket, rows = lc.counts(case)
    n = len(case.points)
    assert bucket.shape == rows.shape == (n,)
    print(f"{case.name}: n {n}, longest bucket {bucket.max()} ({(bucket > 64).sum()} beyond 64), "
          f"longest row {rows.max()} ({(rows > 512).sum()} beyond 512)")
    assert rows.max() == case.row and bucket.max() == case.bucket
    assert lc.row_class(int(rows.max())) == case.row_class
    assert lc.bucket_class(int(bucket.max())) == case.bucket_class
    # what the counts are: two contributions per corner of a cover face, three records per triangle
    L, _ = lc.expected(case)
    assert rows.sum() % 12 == 0 and bucket.sum() * 4 == rows.sum()
    assert np.all(np.diff(L.indptr) - 1 <= rows // 2)      # the cover is closed: every edge has two faces


def test_counts_leave_the_laplacian_as_it_was():
    case = lc.BY_NAME["hub40_s0_c20_k20"]
    L0, M0 = oracle.point_cloud_laplacian(case.points, case.k, lc.MOLL)
    oracle.point_cloud_laplacian_counts(case.points, case.k, lc.MOLL)
    L1, M1 = oracle.point_cloud_laplacian(case.points, case.k, lc.MOLL)
    assert lc.pattern(L0) == lc.pattern(L1) and L0.data.tobytes() == L1.data.tobytes()
    assert M0.tobytes() == M1.tobytes()
    with pytest.raises(RuntimeError):
        oracle.point_cloud_laplacian_counts(case.points, 65, lc.MOLL)


def test_the_table_covers_every_class():
    rows = [c.row for c in lc.CASES]
    assert {c.row_class for c in lc.CASES} == {"sort_row_wave<1>", "sort_row_wave<2>", "sort_row_wave<4>",
                                               "sort_row_wave<8>", "serial sort"}
    assert {64, 128, 256, 258, 512, 514} <= set(rows)          # a full <1>, <2>, <4>, <8> and the next above
    assert min(r for r in rows if r > 64) == 68 and min(r for r in rows if r > 128) == 132
    buckets = [c.bucket for c in lc.CASES]
    assert 64 in buckets and 66 in buckets and max(buckets) > 512
    assert {c.fans_class for c in lc.CASES} == {"k_fans<1>", "k_fans<2>", "k_fans<2>, dead half-wave"}
    assert {c.k for c in lc.CASES if c.cloud == "forest"} == {31, 32, 33, 48, 64}
    assert all(len(c.points) == 2001 for c in lc.CASES if c.cloud == "forest")
    assert [(len(c.points), c.k) for c in lc.CASES if c.cloud == "sheet"] == [(10, 20), (20, 20), (21, 20), (65, 64)]
    # the centre first, in the middle and last: where the diagonal goes into the long row
    for M, k in ((40, 20), (180, 64)):
        assert {c.args[2] for c in lc.CASES if c.cloud == "hub" and c.args[0] == M and c.k == k} == {0, M // 2, M}
    for c in lc.CASES:
        if c.cloud == "hub" and c.row > 128:
            assert int(np.argmax(lc.counts(c)[1])) == c.args[2]    # the long row IS the centre's
    assert set(lc.LONGEST_ROWS) == {c.name for c in lc.CASES if c.cloud == "hub" and c.args[0] == 180}
    assert set(lc.PUSH_ALL_CASES) <= set(lc.BY_NAME)


def test_two_centres_and_the_hub_beside_the_forest():
    rows = lc.counts(lc.BY_NAME["two_centres40_gap0.05_k32"])[1]
    assert (rows[0], rows[1]) == (258, 234)                    # one cloud, both sides of 256
    for name, at in (("forest800_then_hub70_k32", lc.N_FOREST_BESIDE), ("hub70_then_forest800_k32", 0)):
        case = lc.BY_NAME[name]
        bucket, rows = lc.counts(case)
        assert len(case.points) == 871
        assert np.argmax(rows) == at and np.argmax(bucket) == at
        assert (rows > 512).sum() == 1 and (bucket > 64).sum() == 1


def _invariants(L, M):
    scale = abs(L).max()
    assert abs(L - L.T).max() == 0.0                              # exactly symmetric
    assert abs(np.asarray(L.sum(axis=1))).max() <= 1e-12 * scale
    off = (L - diags(L.diagonal())).tocsr()
    off.eliminate_zeros()
    assert off.nnz == 0 or off.data.max() <= 0.0                  # no positive off-diagonal entry
    assert np.all(M > 0)


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_oracle_invariants(case):
    _invariants(*lc.expected(case))


def _moved(P, seed=99):
    return P + np.random.default_rng(seed).uniform(-1e-13, 1e-13, P.shape)


@pytest.mark.parametrize("case", lc.CASES, ids=repr)
def test_pattern_is_stable_under_coordinate_noise(case):
    L0, M0 = lc.expected(case)
    L1, M1 = oracle.point_cloud_laplacian(_moved(case.points), case.k, lc.MOLL)
    assert lc.pattern(L0) == lc.pattern(L1)
    moved = np.abs(L1.data - L0.data).max() / np.abs(L0.data).max()
    print(f"{case.name}: values move by {moved:.1e} of the largest entry")
    assert moved <= 1e-9      # far below the GPU test's bound: the noise is not what that bound measures


def test_segments_of_the_stacked_call():
    segs = lc.segments()
    assert [len(s) for s in segs] == [71, 801, 42] and all(len(s) > lc.SEG_K for s in segs)
    for j, P in enumerate(segs):
        L0, M0 = lc.expected_segment(j)
        _invariants(L0, M0)
        L1, _ = oracle.point_cloud_laplacian(_moved(P), lc.SEG_K, lc.SEG_MOLL)
        assert lc.pattern(L0) == lc.pattern(L1)
    # clouds on the lattice keep to themselves: the k nearest of every point are in its own cloud
    P = np.concatenate(segs)
    start = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    idx, _ = oracle.knn(P, lc.SEG_K, True)
    for j in range(len(segs)):
        own = idx[start[j]:start[j + 1]]
        assert own.min() >= start[j] and own.max() < start[j + 1]
    # The mollification length shows at SEG_MOLL. The hubs' triangles keep the triangle inequality with a
    # margin and their own length is zero; the forest has nearly collinear triples and a positive one. One
    # length for the whole stack (the oracle on the stacked cloud) gives the hub the forest's: another block.
    stacked, _ = oracle.point_cloud_laplacian(P, lc.SEG_K, lc.SEG_MOLL)
    hub_block = stacked[:start[1], :start[1]].tocsr()
    hub_block.sort_indices()
    own, _ = lc.expected_segment(0)
    assert (lc.pattern(hub_block) != lc.pattern(own)
            or np.abs(hub_block.data - own.data).max() > 1e-6 * np.abs(own.data).max())
