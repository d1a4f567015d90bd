"""pyqsm_pdist_select and the stem-width wrappers on the GPU against the CPU statement of their
contract (tests/width_restatement.py, itself held to NumPy and SciPy by tests/test_width_host.py).
Every comparison is exact: the values are the bits of sort(pdist(P))[rank]."""
import functools

import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry import stem_width as sw
from pyqsm_amd.geometry.cloud import PointCloud
from tests import width_restatement as R

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 513, 1025]     # the tile edge is 256
MAX_RANKS = 32


@functools.lru_cache(maxsize=None)
def case(kind, n, dim):
    """(points, sorted pdist, farthest pair) of one input, computed once."""
    P = R.make_points(kind, n, dim, seed=1000 * dim + n)
    P.setflags(write=False)
    d = R.sorted_pdist(P)
    d.setflags(write=False)
    return P, d, R.farthest_pair(P)


def select(P, ranks, **kw):
    """hip.pdist_select on one segment for any number of ranks, in calls of 32."""
    ranks = np.asarray(ranks, np.int64)
    vals, res = [], None
    for c0 in range(0, max(len(ranks), 1), MAX_RANKS):
        part = ranks[c0:c0 + MAX_RANKS]
        part = np.concatenate([part, np.full(-len(part) % MAX_RANKS if c0 else 0, -1, np.int64)])
        res = hip.pdist_select(P, None, part, **kw)
        vals.append(res.values[0, :len(ranks[c0:c0 + MAX_RANKS])])
    return np.concatenate(vals), res


def expected(d, ranks):
    ranks = np.asarray(ranks, np.int64)
    out = np.zeros(len(ranks))
    out[ranks >= 0] = d[ranks[ranks >= 0]]
    return out


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", R.KINDS)
def test_shapes_and_kinds(gpu, kind, dim):
    rng = np.random.default_rng(7)
    for n in SIZES:
        P, d, far = case(kind, n, dim)
        m = len(d)
        if m == 0:
            ranks = [-1, -1, -1]
        else:
            twice = int(rng.integers(0, m))
            ranks = [0, m - 1, (m - 1) // 2, m // 2, *rng.integers(0, m, 30).tolist(), twice, -1, twice]
        got, res = select(P, ranks)
        np.testing.assert_array_equal(got, expected(d, ranks), err_msg=f"n = {n}")
        assert int(res.n_pairs[0]) == m == res.stats["pairs"]
        assert tuple(res.max_pair[0]) == far, n


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_rank_of_24_points(gpu, kind):
    P, d, _ = case(kind, 24, 2)
    assert len(d) == 276
    got, _ = select(P, np.arange(276))
    np.testing.assert_array_equal(got, d)


@pytest.mark.parametrize("dim", [2, 3])
def test_ends_of_every_run_of_equal_values(gpu, dim):
    P, d, _ = case("lattice", 513, dim)
    first = np.nonzero(np.concatenate([[True], d[1:] != d[:-1]]))[0]
    last = np.concatenate([first[1:] - 1, [len(d) - 1]])
    assert len(first) > 10 and d[0] == 0.0 and last[0] > 100       # many zero distances
    ranks = np.stack([first, last], axis=1).reshape(-1)
    got, _ = select(P, ranks)
    np.testing.assert_array_equal(got, d[ranks])


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", ["normal", "lattice"])
def test_batch_equals_single_calls(gpu, kind, dim):
    sizes = (257, 0, 1, 64, 2, 513, 3)
    rng = np.random.default_rng(11)
    parts = [case(kind, n, dim) for n in sizes]
    seg = np.concatenate([[0], np.cumsum(sizes)])
    ranks = np.full((len(sizes), 9), -1, np.int64)
    for s, (_, d, _) in enumerate(parts):
        if len(d):
            ranks[s, :8] = rng.integers(0, len(d), 8)
            ranks[s, 3] = len(d) - 1
            ranks[s, rng.integers(0, 8)] = -1                       # an unused slot somewhere else per segment
    res = hip.pdist_select(np.concatenate([p[0] for p in parts]), seg, ranks)
    for s, (P, d, far) in enumerate(parts):
        one = hip.pdist_select(P, None, ranks[s])
        np.testing.assert_array_equal(res.values[s], one.values[0])
        np.testing.assert_array_equal(res.values[s], expected(d, ranks[s]))
        assert int(res.n_pairs[s]) == int(one.n_pairs[0]) == len(d)
        assert tuple(res.max_pair[s]) == tuple(one.max_pair[0]) == far     # on the lattice: the tie rule
    if kind == "lattice":
        d2 = R.squared_keys(parts[5][0])[0]
        assert (d2 == d2.max()).sum() > 1


def test_more_tiles_than_blocks(gpu):
    """A launch has at most 8 blocks per CU (2048): with more tiles a block walks several, of one
    segment (the 513 points in the middle: six tiles) or of several, and hands its counts on in between."""
    rng = np.random.default_rng(13)
    sizes = [2, 3, 0, 5, 1, 7] * 1250
    sizes[3000:3000] = [513]
    assert sum(1 for n in sizes if n > 1) + 5 > 2 * 2048
    pts = rng.integers(0, 4, size=(sum(sizes), 2)).astype(np.float64)
    seg = np.concatenate([[0], np.cumsum(sizes)])
    m = np.diff(seg) * (np.diff(seg) - 1) // 2
    ranks = np.where(m[:, None] > 0, np.stack([np.zeros_like(m), m - 1, rng.integers(0, np.maximum(m, 1))], axis=1), -1)
    res = hip.pdist_select(pts, seg, ranks)
    np.testing.assert_array_equal(res.n_pairs, m)
    want = np.zeros(ranks.shape)
    far = np.full((len(sizes), 2), -1)
    for s in range(len(sizes)):
        if m[s]:
            P = pts[seg[s]:seg[s + 1]]
            want[s] = R.sorted_pdist(P)[ranks[s]]
            far[s] = R.farthest_pair(P)
    np.testing.assert_array_equal(res.values, want)
    np.testing.assert_array_equal(res.max_pair, far)


def test_more_than_2_to_the_32_pairs(gpu):
    """93 000 points in a row, one unit apart: distance d occurs n - d times, so the element of every
    rank is known without the 4.3e9 distances, and ranks, counts and histogram bins pass 2^32."""
    n = 93_000
    P = np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], axis=1)
    m = n * (n - 1) // 2
    assert m > 1 << 32
    upto = np.cumsum(n - np.arange(1, n, dtype=np.int64))           # pairs at distance <= d, d = 1 ...
    ranks = np.array([0, n - 2, n - 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, m // 2, m - 2, m - 1], np.int64)
    res = hip.pdist_select(P, None, ranks)
    np.testing.assert_array_equal(res.values[0], 1.0 + np.searchsorted(upto, ranks, side="right"))
    assert int(res.n_pairs[0]) == m and tuple(res.max_pair[0]) == (0, n - 1)
    assert res.stats["pair_evaluations"] == res.stats["passes"] * m


def test_errors(gpu):
    P = case("normal", 65, 2)[0]
    m = 65 * 64 // 2
    for pts, seg, ranks in [(P, [0, 65], [[m]]), (np.zeros((65, 4)), [0, 65], [[0]]),
                            (P, [0, 65], [list(range(33))]), (P, [0, 64], [[0]])]:
        with pytest.raises(_lib.PyQSMHipError) as e:
            hip.pdist_select(pts, seg, ranks)
        assert e.value.code == -1
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.pdist_select(P, [0, 65], [[0]], max_pairs=m - 1)
    assert e.value.code == -4
    assert hip.pdist_select(P, [0, 65], [[0]], max_pairs=m).stats["pairs"] == m


def test_stats_and_repeatability(gpu):
    P, d, far = case("logspread", 1025, 3)
    ranks = np.random.default_rng(3).integers(0, len(d), 32)
    a = hip.pdist_select(P, None, ranks)
    b = hip.pdist_select(P, None, ranks)
    assert a.stats == b.stats
    assert 1 <= a.stats["passes"] and a.stats["pair_evaluations"] <= a.stats["passes"] * len(d)
    np.testing.assert_array_equal(a.values, b.values)
    np.testing.assert_array_equal(a.max_pair, b.max_pair)
    np.testing.assert_array_equal(a.values[0], d[ranks])


def test_quantiles_are_numpys(gpu):
    qs = np.linspace(0, 100, 21)                                    # more than 16: two calls
    parts = [case("normal", 257, 2)[0], case("lattice", 64, 2)[0], case("logspread", 65, 2)[0]]
    seg = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    got = sw.pairwise_distance_quantiles(np.concatenate(parts), qs, seg_start=seg)
    for s, P in enumerate(parts):
        np.testing.assert_array_equal(got[s], np.percentile(R.sorted_pdist(P), qs))
    one = sw.pairwise_distance_quantiles(parts[0], 95.0)
    assert one == np.percentile(R.sorted_pdist(parts[0]), 95.0) and np.ndim(one) == 0


@functools.lru_cache(maxsize=None)
def cylinder():
    pts = R.cylinder()
    pts.setflags(write=False)
    return pts


def kept_indices(pts, height, tolerance=0.1):
    """The indices the project's own outlier step keeps of the slab."""
    idx = R.slab(pts, height, tolerance)
    if len(idx) == 0:
        return idx
    return idx[PointCloud(pts[idx]).remove_statistical_outlier(15, 0.95)[1]]


def assert_same_widths(got, want):
    for key, value in want.items():
        np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(value), err_msg=key)


def test_width_at_height(gpu):
    pts = cylinder()
    kept = kept_indices(pts, 1.37)
    assert 150 < len(kept) < 250
    w = sw.width_at_height(pts, seed="t1")
    assert w["seed"] == "t1"
    assert_same_widths(w, R.widths(pts, kept))
    assert w["median"] < w["p90"] < w["p95"] <= w["max_width"] and w["width"] == w["p95"]
    assert 0.25 < w["max_width"] < 0.35
    same = sw.width_at_height({"seed": 4, "clean_pcd": PointCloud(pts)})
    assert same["seed"] == 4
    assert_same_widths(same, R.widths(pts, kept))
    raw = sw.width_at_height(pts, nb_neighbors=None)
    assert_same_widths(raw, R.widths(pts, R.slab(pts, 1.37, 0.1)))
    turned = sw.width_at_height(pts[:, [2, 0, 1]], axis=0, nb_neighbors=None)   # the height along x
    assert turned["p95"] == raw["p95"] and turned["max_pair"] == raw["max_pair"]


def test_width_profile_equals_single_calls(gpu):
    pts = cylinder()
    heights = np.concatenate([np.linspace(0.2, 2.8, 11), [3.5]])
    prof = sw.width_profile(pts, heights)
    assert prof["n_points"][-1] == 0 and (prof["n_points"][:-1] > 100).all()
    for k, h in enumerate(heights):
        one = sw.width_at_height(pts, height=float(h))
        for key in ("width", "bounds", "p90", "p95", "median", "max_width", "max_pair", "n_points", "n_pairs"):
            np.testing.assert_array_equal(prof[key][k], np.asarray(one[key]), err_msg=f"{key} at {h}")
    for key in ("width", "p90", "p95", "median", "max_width", "n_pairs"):
        assert prof[key][-1] == 0
    np.testing.assert_array_equal(prof["bounds"][-1], np.zeros(3))
    np.testing.assert_array_equal(prof["max_pair"][-1], [-1, -1])
