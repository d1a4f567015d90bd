"""pyqsm_cluster_adjacency on the GPU against the CPU statement of its contract
(tests/adjacency_restatement.py, itself pinned to SciPy's sparse_distance_matrix loop by
tests/test_adjacency_host.py): the same cluster pairs, minimum distances equal bit for bit, the same
pair counts and, where asked for, the same closest point pair."""
import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd import cluster_joining as cj
from tests import adjacency_restatement as R

pytestmark = pytest.mark.gpu


def assert_same(res, ref, witness=False):
    """res: hip.ClusterAdjacency; ref: the restatement's dict."""
    keys = sorted(ref)
    assert list(zip(res.a.tolist(), res.b.tolist())) == keys            # the same pairs, ascending by (a, b)
    assert np.array_equal(res.dist, np.array([ref[k][0] for k in keys], dtype=np.float64))
    assert np.array_equal(res.n_pairs, np.array([ref[k][1] for k in keys], dtype=np.int64))
    if witness:
        assert np.array_equal(res.src_idx, np.array([ref[k][2] for k in keys], dtype=np.int64))
        assert np.array_equal(res.tgt_idx, np.array([ref[k][3] for k in keys], dtype=np.int64))
    else:
        assert res.src_idx is None and res.tgt_idx is None


@pytest.fixture(scope="module")
def cloud():
    return R.block_cloud()


@pytest.fixture(scope="module")
def blocks(cloud):
    return R.split_blocks(*cloud)


@pytest.fixture(scope="module")
def ref035(blocks):
    return R.adjacency(*blocks, 0.35, witness=True)


def _plain(ref):
    return {k: v[:2] for k, v in ref.items()}


@pytest.mark.parametrize("threshold,pairs,point_pairs", [(0.35, 178, 471650), (0.2, 155, 107017), (0.01, None, None)])
def test_block_cloud(gpu, blocks, threshold, pairs, point_pairs):
    ref = R.adjacency(*blocks, threshold, witness=True)
    assert len(ref) >= 1
    if pairs is not None:
        assert (len(ref), sum(v[1] for v in ref.values())) == (pairs, point_pairs)
    s, sl, t, tl = blocks
    assert_same(hip.cluster_adjacency(s, sl, threshold, t, tl, return_pairs=True), ref, witness=True)
    assert_same(hip.cluster_adjacency(s, sl, threshold, t, tl), _plain(ref))


@pytest.mark.parametrize("threshold", [0.35, 0.01])
def test_block_cloud_fp64_records(gpu, cloud, threshold):
    """Coordinates that are not fp32-representable: the grid keeps fp64 records."""
    P, lab = cloud
    P = P + 1e-9 * np.random.default_rng(11).standard_normal(P.shape)
    assert not np.array_equal(P.astype(np.float32).astype(np.float64), P)
    s, sl, t, tl = R.split_blocks(P, lab)
    ref = R.adjacency(s, sl, t, tl, threshold, witness=True)
    assert len(ref) >= 1
    assert_same(hip.cluster_adjacency(s, sl, threshold, t, tl, return_pairs=True), ref, witness=True)


def test_lattice_ties_on_the_inclusive_bound(gpu):
    s, sl, t, tl = R.lattice()
    ref = R.adjacency(s, sl, t, tl, 0.25, witness=True)
    assert _plain(ref) == {(0, 1): (0.25, 18), (0, 2): (0.25, 18), (0, 7): (0.0, 4)}
    assert_same(hip.cluster_adjacency(s, sl, 0.25, t, tl, return_pairs=True), ref, witness=True)


def test_same_cloud_form(gpu, cloud):
    P, lab = cloud
    ref = R.adjacency(P, lab, P, lab, 0.35, same_cloud=True, witness=True)
    res = hip.cluster_adjacency(P, lab, 0.35, return_pairs=True)
    assert np.all(res.a < res.b)
    assert_same(res, ref, witness=True)
    # every unordered point pair once: the ordered form over all pairs counts each of them twice
    both = hip.cluster_adjacency(P, lab, 0.35, P, lab)
    off = both.a != both.b
    assert int(both.n_pairs[off].sum()) == 2 * int(res.n_pairs.sum())
    # tiled by source label range, the same rows
    assert_same(hip.cluster_adjacency(P, lab, 0.35, return_pairs=True, max_table=5000), ref, witness=True)


def test_many_labels_within_one_lanes_reach(gpu):
    """Every target its own cluster: a lane meets far more clusters than it can hold in registers."""
    rng = np.random.default_rng(4)
    t = rng.uniform(0, 0.5, (4096, 3))
    s = rng.uniform(0, 0.5, (520, 3))
    sl = rng.integers(0, 8, 520)
    tl = np.arange(4096)
    ref = R.adjacency(s, sl, t, tl, 0.2, witness=True)
    assert len(ref) > 4096
    assert_same(hip.cluster_adjacency(s, sl, 0.2, t, tl, return_pairs=True), ref, witness=True)
    assert_same(hip.cluster_adjacency(s, sl, 0.2, t, tl, cache=False), _plain(ref))


@pytest.mark.parametrize("count", [1, 63, 65, 257])
def test_wave_and_block_edges(gpu, blocks, count):
    s, sl, t, tl = blocks
    pick = np.random.default_rng(count).choice(len(s), count, replace=False)
    ref = R.adjacency(s[pick], sl[pick], t, tl, 0.35, witness=True)
    assert_same(hip.cluster_adjacency(s[pick], sl[pick], 0.35, t, tl, return_pairs=True), ref, witness=True)


def test_stray_points_are_found_through_the_outer_cells(gpu, blocks, ref035):
    s, sl, t, tl = blocks
    far = np.array([1000.0, 1003.0, 998.0])
    s2 = np.concatenate([s, far + [[0, 0, 0], [0.125, 0, 0], [0, 0.125, 0]]])
    t2 = np.concatenate([t, far + [[0, 0, 0.125], [0.125, 0.125, 0], [0.0625, 0.0625, 0.0625]]])
    sl2 = np.concatenate([sl, [9000, 9000, 9003]])
    tl2 = np.concatenate([tl, [9001, 9001, 9002]])
    ref = R.adjacency(s2, sl2, t2, tl2, 0.35, witness=True)
    assert {k: v for k, v in ref.items() if k[0] < 9000} == ref035       # the rest does not change
    assert {k: v[1] for k, v in ref.items() if k[0] >= 9000} == {(9000, 9001): 4, (9000, 9002): 2,
                                                                 (9003, 9001): 2, (9003, 9002): 1}
    assert_same(hip.cluster_adjacency(s2, sl2, 0.35, t2, tl2, return_pairs=True), ref, witness=True)


def test_ignored_empty_and_large_labels(gpu, blocks):
    s, sl, t, tl = blocks
    s, sl, t, tl = s[:3000], sl[:3000].copy(), t[:6000], tl[:6000].copy()
    sl[::3] = -1
    tl[1::4] = -7
    # non-contiguous and large label values; three targets that have a neighbour get 7, 1000 and 2^31 - 2
    vals = np.unique(tl[tl >= 0])
    new = 2**31 + 5 * np.arange(len(vals))
    hit = sorted({k[1] for k in R.adjacency(s, sl, t, tl, 0.35)})[:3]
    new[np.searchsorted(vals, hit)] = [7, 1000, 2**31 - 2]
    tl = np.where(tl >= 0, new[np.searchsorted(vals, np.maximum(tl, 0))], tl)
    ref = R.adjacency(s, sl, t, tl, 0.35, witness=True)
    assert {7, 1000, 2**31 - 2} <= {k[1] for k in ref}
    assert_same(hip.cluster_adjacency(s, sl, 0.35, t, tl, return_pairs=True), ref, witness=True)
    for res in (hip.cluster_adjacency(s, np.full(len(s), -1), 0.35, t, tl),
                hip.cluster_adjacency(s, sl, 0.35, t, np.full(len(t), -3)),
                hip.cluster_adjacency(s[:0], sl[:0], 0.35, t, tl),
                hip.cluster_adjacency(s, sl, 0.35, t[:0], tl[:0]),
                hip.cluster_adjacency(s, np.full(len(s), -1), 0.35)):
        assert len(res.a) == len(res.b) == len(res.dist) == len(res.n_pairs) == 0


def test_tiling_equals_the_single_call(gpu, blocks, ref035):
    s, sl, t, tl = blocks
    assert len(np.unique(sl)) * len(np.unique(tl)) > 10 * 1000
    assert_same(hip.cluster_adjacency(s, sl, 0.35, t, tl, return_pairs=True, max_table=1000), ref035, witness=True)


def test_reproducible_bit_for_bit(gpu, blocks):
    s, sl, t, tl = blocks
    r1 = hip.cluster_adjacency(s, sl, 0.35, t, tl, return_pairs=True)
    r2 = hip.cluster_adjacency(s, sl, 0.35, t, tl, return_pairs=True)
    for x, y in zip(r1, r2):
        assert x.tobytes() == y.tobytes()


def test_small_capacity_is_followed_by_a_second_call(gpu, blocks, ref035):
    """The C-ABI's sizing convention: at most `capacity` rows are written, *count is what was found."""
    import ctypes
    s, sl, t, tl = blocks
    us, ds = np.unique(sl, return_inverse=True)
    ut, dt = np.unique(tl, return_inverse=True)
    ds, dt = ds.astype(np.int32), dt.astype(np.int32)
    cap = 10
    a, b = np.full(cap + 1, -5, np.int32), np.full(cap + 1, -5, np.int32)
    d2, cnt = np.full(cap + 1, -5.0), np.full(cap + 1, -5, np.int64)
    found = ctypes.c_int64(0)
    _lib.check(_lib.load().pyqsm_cluster_adjacency(
        hip._p(s), hip._p(ds), len(s), len(us), hip._p(t), hip._p(dt), len(t), len(ut), 0.35, 0, cap,
        hip._p(a), hip._p(b), hip._p(d2), hip._p(cnt), None, None, ctypes.byref(found), None, 0))
    keys = sorted(ref035)
    assert found.value == len(keys) > cap
    assert [(int(us[i]), int(ut[j])) for i, j in zip(a[:cap], b[:cap])] == keys[:cap]
    assert np.array_equal(np.sqrt(d2[:cap]), [ref035[k][0] for k in keys[:cap]])
    assert a[cap] == -5 and b[cap] == -5 and d2[cap] == -5.0 and cnt[cap] == -5


def test_table_bound_is_an_error_not_a_wrong_answer(gpu):
    import ctypes
    p = np.zeros((2, 3))
    lab = np.zeros(2, np.int32)
    found = ctypes.c_int64(0)
    code = _lib.load().pyqsm_cluster_adjacency(hip._p(p), hip._p(lab), 2, 1 << 14, hip._p(p), hip._p(lab), 2,
                                               (1 << 12) + 1, 0.35, 0, 0, None, None, None, None, None, None,
                                               ctypes.byref(found), None, 0)
    assert code == -4                                                     # PYQSM_ERANGE


def test_determine_adjacency_end_to_end(gpu, blocks):
    s, sl, t, tl = blocks
    src = [(int(l), s[sl == l]) for l in np.unique(sl)]
    tgt = [(int(l), t[tl == l]) for l in np.unique(tl)]
    everything = src + tgt
    label_list = [l for l, _ in src]
    adj = cj.determine_adjacency(label_list, everything, threshold=0.35)
    want = {l: {} for l in label_list}
    for (a, b), (dist, _) in R.scipy_loop(s, sl, t, tl, 0.35).items():
        want[a][b] = dist
    assert adj == want
    assert [list(v) for v in adj.values()] == [list(v) for v in want.values()]   # inner order too
    assert 0 in label_list                                              # label 0 as a source is served
    # the same through separate source and candidate lists, label 0 among the candidates skipped
    t0 = [(0, t[:50] + 0.0)] + tgt
    assert cj.determine_adjacency(label_list[1:], t0, threshold=0.35, src_kdtrees=src) == \
        {l: want[l] for l in label_list[1:]}


def test_errors(gpu, blocks):
    s, sl, t, tl = blocks
    bad = s.copy()
    bad[17, 2] = np.nan
    for call in (lambda: hip.cluster_adjacency(bad, sl, 0.35, t, tl),
                 lambda: hip.cluster_adjacency(s, sl, 0.35, np.where(t > 1e9, t, np.inf), tl),
                 lambda: hip.cluster_adjacency(s, sl, 0.0, t, tl),
                 lambda: hip.cluster_adjacency(s, sl, -1.0, t, tl),
                 lambda: hip.cluster_adjacency(s, sl, float("nan"), t, tl)):
        with pytest.raises(_lib.PyQSMHipError) as e:
            call()
        assert e.value.code == -1                                         # PYQSM_EINVAL
    with pytest.raises(ValueError):
        hip.cluster_adjacency(s, sl[:-1], 0.35, t, tl)
    with pytest.raises(ValueError):
        hip.cluster_adjacency(s, sl, 0.35, t, tl[:-1])
    with pytest.raises(ValueError):
        hip.cluster_adjacency(s, sl, 0.35, t, tl, max_table=10)           # fewer entries than target clusters
