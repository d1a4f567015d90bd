"""Every input of tests/knn_cases.py has the property that tests/test_gpu_knn_f64.py depends on, shown
on the CPU with oracle.knn alone. Without these a GPU test could pass on a path it never took: a cloud
that happens to be fp32-representable gets fp32 records, a tie count on the other side of n // 16
takes the other tie pass, strays that are not far enough are answered by the first grid.

Measured with the oracle: few_ties ties at the k-th place for 29 / 33 / 37 of 8 000 queries at
k = 8 / 20 / 32 (n // 16 = 500); many_ties for 3 382 / 3 670 of 4 000 at k = 8 / 20 (n // 16 = 250);
contracted has a zero nearest distance for 20 % of its queries, 722 ties at k = 20 and nearest
distances from 3e-11 to 0.3."""
import numpy as np
import pytest

import oracle

from tests import knn_cases as kc


@pytest.mark.parametrize("n,seed", [(5000, 0), (6000, 5), (8000, 5)])
def test_offgrid_leaves_no_row_on_the_f32_lattice(n, seed):
    P, twin = kc.offgrid(n, seed), kc.forest(n, seed)
    assert P.shape == (n, 3) and P.dtype == np.float64
    assert kc.f32_representable(twin).all()             # the twin gets fp32 records by itself
    assert not kc.f32_representable(P).any()            # every row has a coordinate no float holds
    assert not (P.astype(np.float32) == P).all(axis=1).any()
    assert np.abs(P - kc.SHIFT - twin).max() < 1e-7     # the same cloud, moved


def test_lattice_twin_is_f32_representable_and_full_of_ties():
    P = kc.lattice()
    assert kc.f32_representable(P).all()
    assert kc.ties_at_kth(P, 20) > len(P) // 16


@pytest.mark.parametrize("k", kc.FEW_TIES_KS)
def test_few_ties_stay_with_the_wave_tie_pass(k):
    P = kc.few_ties()
    n = len(P)
    assert n == 8000 and not kc.f32_representable(P).all()
    ties = kc.ties_at_kth(P, k)
    print(f"few_ties k={k}: {ties} of {n} queries tie at the k-th place (n // 16 = {n // 16})")
    assert 0 < ties <= n // 16


@pytest.mark.parametrize("k", kc.MANY_TIES_KS)
def test_many_ties_go_to_the_per_lane_pass(k):
    P = kc.many_ties()
    n = len(P)
    assert n == 4000 and not kc.f32_representable(P).all()
    ties = kc.ties_at_kth(P, k)
    print(f"many_ties k={k}: {ties} of {n} queries tie at the k-th place (n // 16 = {n // 16})")
    assert ties > n // 16


@pytest.mark.parametrize("k", kc.SPREAD_TIES_KS)
def test_spread_ties_tie_as_often_with_a_point_per_node(k):
    P = kc.spread_ties()
    n = len(P)
    assert n == 4000 and not kc.f32_representable(P).all()
    ties = kc.ties_at_kth(P, k)
    nodes = len(np.unique(np.round(P * 10).astype(np.int64), axis=0))
    print(f"spread_ties k={k}: {ties} of {n} queries tie at the k-th place, {nodes} nodes hold the points")
    assert ties > n // 16
    assert nodes > n // 2                      # many_ties: 729 nodes for as many points


def test_contracted_has_duplicates_contrast_and_ties():
    P, dst, src = kc.contracted()
    n = len(P)
    assert n == 8000 and not kc.f32_representable(P).all()
    # the copies: exact, 800 of them, no point both a copy and a source
    assert len(dst) == len(src) == kc.N_COPIES == 800 and not np.intersect1d(dst, src).size
    assert np.array_equal(P[dst], P[src])
    _, d2 = oracle.knn(P, 21, True)
    zero = float((d2[:, 0] == 0).mean())
    # every copy and every source has a twin at distance zero: at least 1 600 of 8 000 queries
    assert zero >= 2 * kc.N_COPIES / n
    ties = int((d2[:, 19] == d2[:, 20]).sum())
    near = np.sqrt(d2[:, 0][d2[:, 0] > 0])
    print(f"contracted: {zero:.1%} zero nearest distances, {ties} ties at k = 20, nearest distances "
          f"{near.min():.2g} .. {near.max():.2g}")
    assert ties > 0
    # six orders of magnitude between the pulled points' spacing and the untouched ones'
    assert near.min() < 1e-8 and np.percentile(near, 99) > 1e-2
    # 70 % of the points lie within the largest pull (per axis) of a lattice node
    off = np.abs(P - np.round(P / kc.LATTICE_STEP) * kc.LATTICE_STEP).max(axis=1)
    assert 0.6 < float((off <= max(kc.PULLS)).mean()) < 0.8


@pytest.mark.parametrize("representable", [True, False])
@pytest.mark.parametrize("name,n_base", [("few_strays", 6000), ("few_strays", 60000), ("many_strays", 8000),
                                         ("axis_strays", 6000)])
def test_strays_are_what_they_are_called(name, n_base, representable):
    X, stray = kc.few_strays(representable, n_base) if name == "few_strays" else kc.STRAYS[name](representable)
    base = X[~stray]
    n_stray = {"few_strays": 40, "many_strays": 400, "axis_strays": 40}[name]
    assert len(base) == n_base and int(stray.sum()) == n_stray
    if representable:
        assert kc.f32_representable(X).all()
    else:
        assert not kc.f32_representable(base).any() and not kc.f32_representable(X).all()
    lo, hi = base.min(0), base.max(0)
    ext = hi - lo
    centre = base.mean(0)
    far = X[stray]
    # (the oracle on the base alone and the strays by hand: its grid over the strays' box costs seconds)
    spacing = float(np.median(np.sqrt(oracle.knn(base, 8, True)[1][:, 7])))  # the base's 8th-neighbour distance
    pair = ((far[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    pair[np.arange(len(far)), np.flatnonzero(stray)] = np.inf
    alone = np.sqrt(pair.min(axis=1))                        # every stray's nearest other point
    if name == "few_strays":
        rel = np.abs(far - centre) / ext
        assert rel.min() > 19 and rel.max() < 61             # 20 to 60 extents away on every axis
        # five of them within millimetres of each other, the other 35 alone
        assert int((alone < 0.01).sum()) == 5 and np.sort(alone)[5] > 100 * spacing
    elif name == "many_strays":
        assert (far >= lo - 25 * ext - 1e-3).all() and (far <= hi + 25 * ext + 1e-3).all()
        box = (far.max(0) - far.min(0)) / ext
        assert box.min() > 40                                # they do fill a box some 50 times the cloud's
        assert alone.min() > 10 * spacing
    else:
        assert (far[:, 1:] >= lo[1:]).all() and (far[:, 1:] <= hi[1:]).all()      # along x only
        rel = (far[:, 0] - hi[0]) / ext[0]
        assert rel.min() > 2.9 and rel.max() < 8.1
        assert alone.min() > 4 * spacing
    # the strays are spread through the array, not appended to it
    assert stray[: len(X) // 2].any() and stray[len(X) // 2:].any()


def test_degenerate_clouds():
    assert kc.IDENTICAL.shape == (40, 3) and (kc.IDENTICAL == 0.1).all()
    assert not kc.f32_representable(kc.IDENTICAL).any()
    assert (kc.IDENTICAL.max(0) - kc.IDENTICAL.min(0) == 0).all()            # extent 0
    idx, d2 = oracle.knn(kc.IDENTICAL, 3, True)
    assert (d2 == 0).all() and list(idx[0]) == [1, 2, 3] and list(idx[39]) == [0, 1, 2]
    assert kc.THREE.shape == (3, 3) and not kc.f32_representable(kc.THREE).any()
    idx, d2 = oracle.knn(kc.THREE, 5, True)                                  # fewer points than k: padded
    assert list(idx[0]) == [1, 2, 3, 3, 3] and np.isinf(d2[:, 2:]).all() and np.isfinite(d2[:, :2]).all()
    assert kc.ONE.shape == (1, 3) and not kc.f32_representable(kc.ONE).any()
    idx, d2 = oracle.knn(kc.ONE, 2, True)
    assert idx.tolist() == [[1, 1]] and np.isinf(d2).all()
    idx, d2 = oracle.knn(kc.ONE, 2, False)
    assert idx.tolist() == [[0, 1]] and d2[0, 0] == 0 and np.isinf(d2[0, 1])


@pytest.mark.parametrize("name,args", [("many_ties", ()), ("few_ties", ()), ("contracted", ()),
                                       ("axis_strays", (False,))])
@pytest.mark.parametrize("excl", [True, False])
def test_expected_is_the_oracle_at_that_k(name, args, excl):
    """expected() cuts the oracle's answer at K_REF down to k: the same arrays as asking at k, on the
    clouds where most rows tie across the cut, and with the query itself kept or left out."""
    P = kc.cloud(name, *args)
    for k in (1, 8, 20, 33, 150, kc.K_REF):
        idx, d2 = oracle.knn(P, k, excl)
        idx0, d20 = kc.expected(name, *args, k=k, exclude_self=excl)
        assert idx0.shape == (len(P), k)
        assert np.array_equal(idx, idx0) and np.array_equal(d2, d20), (name, k, excl)


def test_expected_is_shared_and_read_only():
    a = kc.expected("offgrid", 5000, k=20)
    b = kc.expected("offgrid", 5000, k=20, exclude_self=True)
    assert a[0] is b[0] and a[1] is b[1]
    assert not a[0].flags.writeable and not a[1].flags.writeable and not kc.offgrid(5000).flags.writeable
    idx, d2 = oracle.knn(kc.offgrid(5000), 20, True)
    assert np.array_equal(idx, a[0]) and np.array_equal(d2, a[1])
