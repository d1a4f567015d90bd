"""Plane segmentation without a GPU: the NumPy contract on known answers, the drawers, the C-ABI's
declarations and its argument checks (which return before any device is touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

from pyqsm_amd import _lib
from pyqsm_amd.math_utils import fit
from tests import plane_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pyqsm_plane_models", "pyqsm_plane_count", "pyqsm_segment_plane", "pyqsm_segment_planes"]
EINVAL = -1


def test_three_axis_points_give_the_z_plane():
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    np.testing.assert_array_equal(R.hypothesis(P, [0, 1, 2]), [0.0, 0.0, 1.0, 0.0])
    np.testing.assert_array_equal(R.hypothesis(P, [0, 2, 1]), [0.0, 0.0, 1.0, 0.0])  # the sign rule, not the order
    np.testing.assert_array_equal(R.hypothesis(P + [0, 0, 2.0], [0, 1, 2]), [0.0, 0.0, 1.0, -2.0])


def test_sign_rule_on_each_branch():
    np.testing.assert_array_equal(R.orient([0.6, 0.0, -0.8, 1.0]), [-0.6, -0.0, 0.8, -1.0])   # c decides
    np.testing.assert_array_equal(R.orient([0.6, 0.0, 0.8, 1.0]), [0.6, 0.0, 0.8, 1.0])
    np.testing.assert_array_equal(R.orient([0.6, -0.8, 0.0, 2.0]), [-0.6, 0.8, 0.0, -2.0])    # c == 0: b decides
    np.testing.assert_array_equal(R.orient([-0.6, 0.8, 0.0, 2.0]), [-0.6, 0.8, 0.0, 2.0])
    np.testing.assert_array_equal(R.orient([-1.0, 0.0, 0.0, 3.0]), [1.0, 0.0, 0.0, -3.0])     # c == b == 0: a decides
    np.testing.assert_array_equal(R.orient([1.0, 0.0, 0.0, 3.0]), [1.0, 0.0, 0.0, 3.0])
    # through the construction: a wall x = 2 sampled in either orientation
    W = np.array([[2.0, 0.0, 0.0], [2.0, 1.0, 0.0], [2.0, 0.0, 1.0]])
    np.testing.assert_array_equal(R.hypothesis(W, [0, 1, 2]), [1.0, 0.0, 0.0, -2.0])
    np.testing.assert_array_equal(R.hypothesis(W, [0, 2, 1]), [1.0, 0.0, 0.0, -2.0])


def test_invalid_hypotheses_are_zero_rows():
    P = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 1.0, 0.0]])
    for idx in ([0, 1, 2], [0, 0, 3], [0, 1, 4], [-1, 1, 3]):  # collinear, repeated, out of range twice
        np.testing.assert_array_equal(R.hypothesis(P, idx), np.zeros(4))
    assert R.count(P, np.zeros((1, 4)), 1.0)[0] == 0
    # the cone: the plane z = 0 is 90 degrees from the x axis
    Z = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    np.testing.assert_array_equal(R.hypothesis(Z, [0, 1, 2], axis=[1.0, 0.0, 0.0], cos_limit=0.5), np.zeros(4))
    np.testing.assert_array_equal(R.hypothesis(Z, [0, 1, 2], axis=[0.0, 0.0, 1.0], cos_limit=0.5), [0, 0, 1.0, 0])


def test_more_samples_give_the_least_squares_plane():
    rng = np.random.default_rng(3)
    xy = rng.uniform(-1, 1, (10, 2))
    P = np.column_stack([xy, 0.25 * xy[:, 0] - 0.5 * xy[:, 1] + 1.0])  # exactly planar
    p = R.hypothesis(P, list(range(10)))
    want = np.array([-0.25, 0.5, 1.0, -1.0]) / np.sqrt(0.25**2 + 0.5**2 + 1.0)
    np.testing.assert_allclose(p, want, atol=1e-14)


def test_selection_rule_hand_worked():
    # n = 100, m = 3. Row 0 counts 50: f = 0.5, f^3 = 0.125; at probability 0.5 the bound is
    # log(0.5) / log(0.875) = 5.19..., so rows 0 ... 5 are looked at and row 6 is not: used = 6.
    c = np.array([50, 10, 50, 20, 30, 40, 90, 90, 5, 5], dtype=np.int32)
    assert R.select(c, 100, 3, 0.5) == (0, 50, 6)           # the 90 at row 6 is never seen
    assert R.select(c, 100, 3, 1.0) == (6, 90, 10)          # probability 1: every row, ties keep row 6
    # after row 6 at the default probability: log(1e-8) / log(1 - 0.729) = 14.1 > H: all rows
    assert R.select(c, 100, 3, 0.99999999) == (6, 90, 10)
    assert R.select(np.array([7, 100, 100], dtype=np.int32), 100, 3, 0.5) == (1, 100, 2)  # f == 1 stops at once
    assert R.select(np.array([3, 3, 3], dtype=np.int32), 100, 3, 1.0) == (0, 3, 3)         # ties keep the lower row
    assert R.select(np.zeros(4, dtype=np.int32), 100, 3, 0.5) == (-1, 0, 4)
    assert R.select(np.zeros(0, dtype=np.int32), 100, 3, 0.5) == (-1, 0, 0)
    # f^m vanishes next to 1 (1e-20): the bound is H, not a division by log(1) = 0
    assert R.select(np.array([1, 2], dtype=np.int32), 100, 10, 0.5) == (1, 2, 2)


def test_mulhi64_against_python_integers():
    rng = np.random.default_rng(5)
    u = fit.draw_u64(2000, seed=rng)
    edge = np.array([0, 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1], dtype=np.uint64)
    for n in (1, 2, 3, 63, 2500, 2**31 - 1, 2**32 + 7, 2**63 + 11, 2**64 - 1):
        for arr in (u, edge):
            got = fit.mulhi64(arr, n)
            want = [(int(x) * n) >> 64 for x in arr]
            assert got.dtype == np.uint64 and [int(g) for g in got] == want
            assert all(R.mulhi64(int(x), n) == w for x, w in zip(arr, want))
            assert n >= 2**64 - 1 or all(w < n for w in want)


@pytest.mark.parametrize("m", [3, 4, 10, 32])
def test_sample_drawer(m):
    for n in (m, m + 1, 1000):
        S = fit.draw_plane_samples(n, 500, m, seed=11)
        assert S.shape == (500, m) and S.dtype == np.int64
        assert S.min() >= 0 and S.max() < n
        srt = np.sort(S, axis=1)
        assert (np.diff(srt, axis=1) > 0).all()  # distinct within a row
        np.testing.assert_array_equal(S, fit.draw_plane_samples(n, 500, m, seed=11))
        assert n == m or not np.array_equal(S, fit.draw_plane_samples(n, 500, m, seed=12))
    if m == 3:
        np.testing.assert_array_equal(fit.draw_plane_samples(50, 20, 3, seed=4), fit.draw_samples(50, 20, seed=4))
    with pytest.raises(ValueError):
        fit.draw_plane_samples(m - 1, 5, m)


def test_sample_drawer_covers_every_index():
    S = fit.draw_plane_samples(12, 4000, 10, seed=2)
    assert np.bincount(S.ravel(), minlength=12).min() > 2500  # 4000 * 10 / 12 = 3333 each


def test_u64_drawer():
    d = fit.draw_u64((4, 256, 3), seed=9)
    assert d.shape == (4, 256, 3) and d.dtype == np.uint64
    np.testing.assert_array_equal(d, fit.draw_u64((4, 256, 3), seed=9))
    assert not np.array_equal(d, fit.draw_u64((4, 256, 3), seed=10))
    assert (d >> np.uint64(63)).mean() > 0.4  # the top bit is in use: the whole 64-bit range
    idx = fit.mulhi64(d, 2500)
    assert idx.max() < 2500 and np.bincount(idx.ravel().astype(np.int64), minlength=2500).max() < 12


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "pyqsm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pyqsm_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_arguments_are_checked_before_any_device():
    """Every EINVAL case, with a device number that does not exist: a call that got as far as the
    device would answer ENODEV (or run)."""
    lib = _lib.load()
    dev = 99
    P = np.ascontiguousarray(np.random.default_rng(0).normal(size=(40, 3)))
    nan = P.copy()
    nan[17, 1] = np.nan
    inf = P.copy()
    inf[39, 2] = np.inf
    planes = np.zeros((5, 4))
    counts = np.zeros(5, dtype=np.int32)
    fitp, hyp = np.zeros(4), np.zeros(4)
    inl = np.zeros(40, dtype=np.int64)
    n_in, best, used, k = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    labels = np.zeros(40, dtype=np.int32)
    pf, ph = np.zeros((2, 4)), np.zeros((2, 4))
    cnt, bst, usd = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)

    def models(pts=P, n=40, H=5, m=3):
        smp = np.zeros((5, 40), dtype=np.int64)
        return lib.pyqsm_plane_models(_ptr(pts), n, _ptr(smp), H, m, None, 0.0, _ptr(planes), dev)

    def count(pts=P, H=5, thresh=0.1):
        return lib.pyqsm_plane_count(_ptr(pts), 40, _ptr(planes), H, thresh, _ptr(counts), dev)

    def one(pts=P, n=40, H=5, m=3, thresh=0.1, prob=0.99):
        smp = np.zeros((5, 40), dtype=np.int64)
        return lib.pyqsm_segment_plane(_ptr(pts), n, _ptr(smp), H, m, thresh, prob, None, 0.0, _ptr(fitp), _ptr(hyp),
                                       _ptr(inl), ctypes.byref(n_in), ctypes.byref(best), ctypes.byref(used), dev)

    def many(pts=P, n=40, P_=2, H=5, m=3, thresh=0.1, prob=0.99):
        dr = np.zeros((2, 5, 40), dtype=np.uint64)
        return lib.pyqsm_segment_planes(_ptr(pts), n, _ptr(dr), P_, H, m, thresh, prob, 1, None, 0.0, _ptr(labels),
                                        _ptr(pf), _ptr(ph), _ptr(cnt), _ptr(bst), _ptr(usd), ctypes.byref(k), dev)

    for m in (2, 0, -1, 33):
        assert models(m=m) == EINVAL and one(m=m) == EINVAL and many(m=m) == EINVAL
    assert one(n=9, m=10) == EINVAL and many(n=9, m=10) == EINVAL  # fewer points than samples
    assert one(n=2) == EINVAL and many(n=2) == EINVAL
    for t in (0.0, -0.1, float("nan"), float("inf")):
        assert count(thresh=t) == EINVAL and one(thresh=t) == EINVAL and many(thresh=t) == EINVAL
    for pr in (0.0, -0.5, 1.0000001, float("nan")):
        assert one(prob=pr) == EINVAL and many(prob=pr) == EINVAL
    for bad in (nan, inf):
        assert models(pts=bad) == EINVAL and count(pts=bad) == EINVAL
        assert one(pts=bad) == EINVAL and many(pts=bad) == EINVAL
    assert many(P_=0) == EINVAL and many(P_=-1) == EINVAL
    assert models(H=-1) == EINVAL and count(H=-1) == EINVAL and one(H=-1) == EINVAL and many(H=-1) == EINVAL
    # H == 0 is valid and finds nothing, without a device
    assert models(H=0) == 0 and count(H=0) == 0
    best.value, used.value, n_in.value = 5, 5, 5
    assert one(H=0) == 0 and (best.value, used.value, n_in.value) == (-1, 0, 0)
    k.value = 7
    labels[:] = 3
    assert many(H=0) == 0 and k.value == 0 and (labels == -1).all() and (bst == -1).all()
