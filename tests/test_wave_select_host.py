"""The preconditions of the GPU cases built from tests/wave_select_cases.py, checked without a GPU: which
side of the 64-candidate step, of the power-of-two padding and of the 512-pair cap every case falls on,
and that the exact ties the tie rules are tested with are really there."""
import numpy as np
import pytest

from tests import features_restatement as F
from tests import voxelgrid_restatement as V
from tests import wave_select_cases as C

CAP = 512   # kNormCap (normals.hip) and kQueryCap (features.hip)


@pytest.mark.parametrize("jitter", [False, True])
def test_clump_counts_straddle_the_step_the_padding_and_the_cap(jitter):
    P, size = C.clumps(jitter=jitter)          # asserts count == clump size per point itself
    assert len(P) == sum(C.SIZES) and set(size) == set(C.SIZES)
    for edge in (64, 128, CAP):                # one candidate fewer, exactly, one more
        assert {edge - 1, edge, edge + 1} <= set(C.SIZES)
    assert max(C.SIZES) > CAP and sorted(s for s in C.SIZES if s > CAP) == [513, 700]
    # the queries of the radius kernels see the same counts: min(size, k) hits 63 / 64 and 511 / 512
    Q = C.clump_queries(P)
    for k in (64, 512):
        idx, cnt, in_range = V.neighbours(P, Q, C.RADIUS, k)
        assert np.array_equal(in_range[:-1], np.minimum(size, k + 8)) and in_range[-1] == 0   # exact up to k + 8
        assert {k - 1, k} <= set(cnt) and (in_range > k).any()
        # no tie at the k-th place: the restatement's (d2, index) order settles every row
        d2 = np.sort(np.where(C.sqdist(P, Q) < C.RADIUS ** 2, C.sqdist(P, Q), np.inf), axis=1)
        assert not (np.isfinite(d2[:, k]) & (d2[:, k - 1] == d2[:, k])).any()


def test_lattice_ties_at_the_feature_cap():
    P = C.lattice_clump(513)
    assert len(np.unique(P, axis=0)) == 513 and P[:, 2].max() == 1.0
    d2 = C.sqdist(P, P)
    assert (d2 <= 2.0 ** 2).all()              # radius 2.0: every ball is the whole clump, 513 > max_k = 100
    assert C.tie_at(P, P, 100).any()


@pytest.mark.parametrize("m", [511, 512, 513, 700])
def test_far_queries_see_the_whole_cloud_and_ties(m):
    src = C.random_cube(m) if m == 700 else C.lattice_clump(m)
    Q = C.far_queries(src)
    for k in C.SMOOTH_KS:
        for q in Q[:6]:                        # the first radius with k points inside holds all m
            assert C.first_sufficient_radius(src, q, k)[1] == m
        # the restatement agrees with all m * n distances sorted, ties by index
        assert np.array_equal(F.knn(src, Q, k), C.brute_knn(src, Q, k))
    assert (m > CAP) == (m in (513, 700))


@pytest.mark.parametrize("k", C.SMOOTH_KS)
def test_a_far_query_has_a_tie_at_the_kth_place(k):
    """On some lattice source (at k = 64 the full cube's nearest layer is exactly 64 sites: no tie there,
    but the 511- and 513-site lattices have one)."""
    ties = {m: C.tie_at(C.lattice_clump(m), C.far_queries(C.lattice_clump(m))[:6], k).any() for m in (511, 512, 513)}
    assert any(ties.values())
    assert ties[513]                           # above the cap, where the index bisection settles it


def test_normals_overflow_clouds():
    for near, far, fits in ((600, 0, False), (400, 200, True)):
        P = C.stacked(near, far)
        d2 = C.sqdist(P, P[:1])[0]
        assert (d2 < C.RADIUS ** 2).sum() == 601 > CAP        # the origin's ball: the bisection runs
        tau = np.sort(d2)[30 - 1]                             # max_nn = 30
        assert tau == d2[1] and ((d2 <= tau).sum() <= CAP) == fits
    assert 601 > CAP >= 401
