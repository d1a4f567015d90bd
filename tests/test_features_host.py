"""Host-side checks of the geometric features and the smoothing: the restatement against analytic
answers, wrapper validation before any device call, the no-GPU failure mode of the new entry points,
and (with the device call replaced) the NaN fill of exploration.compute_features and the dtype rules
of smooth_feature."""
import numpy as np
import pytest

from pyqsm_amd import _lib, exploration, hip
from pyqsm_amd.geometry import features as gf
from pyqsm_amd.utils import algo
from tests import features_restatement as R

IDX = {f: j for j, f in enumerate(R.FEATURE_NAMES)}


def _feat(P, radius, q=0, **kw):
    f, cnt, _ = R.compute_features(P, radius, qidx=np.array([q]), **kw)
    return {name: f[0, j] for name, j in IDX.items()}, cnt[0]


def test_feature_names_match():
    assert tuple(gf.FEATURE_NAMES) == R.FEATURE_NAMES == hip.FEATURE_NAMES


def test_line():
    P = np.zeros((41, 3))
    P[:, 0] = np.linspace(-1, 1, 41)
    f, _ = _feat(P, 0.5, q=20)
    assert f["linearity"] == pytest.approx(1.0, abs=1e-12)
    assert f["planarity"] == pytest.approx(0.0, abs=1e-12)
    assert f["PCA1"] == pytest.approx(1.0, abs=1e-12)


def test_horizontal_disc():
    rng = np.random.default_rng(1)
    xy = rng.uniform(-1, 1, (20_000, 2))
    xy = xy[np.hypot(xy[:, 0], xy[:, 1]) < 1]
    P = np.column_stack([xy, np.zeros(len(xy))])
    q = int(np.argmin(np.hypot(P[:, 0], P[:, 1])))
    f, _ = _feat(P, 0.5, q=q)
    assert f["planarity"] == pytest.approx(1.0, abs=0.05)
    assert f["verticality"] == 0.0
    assert (f["nx"], f["ny"], f["nz"]) == (0.0, 0.0, 1.0)


def test_vertical_plane():
    rng = np.random.default_rng(2)
    P = np.column_stack([rng.uniform(-1, 1, 5000), np.zeros(5000), rng.uniform(-1, 1, 5000)])
    f, _ = _feat(P, 0.5, q=int(np.argmin(np.abs(P).sum(1))))
    assert f["verticality"] == pytest.approx(1.0, abs=1e-12)


def test_isotropic_ball():
    rng = np.random.default_rng(3)
    P = rng.uniform(-1, 1, (200_000, 3))
    P[0] = 0.0
    f, _ = _feat(P, 0.5, q=0)
    assert f["sphericity"] == pytest.approx(1.0, abs=0.05)


def test_nan_below_three_and_for_coincident_points():
    P = np.array([[0.0, 0, 0], [0.1, 0, 0], [5.0, 5, 5], [5.0, 5, 5], [5.0, 5, 5]])
    f, cnt, _ = R.compute_features(P, 0.5)
    assert list(cnt) == [2, 2, 3, 3, 3]
    assert np.isnan(f).all()


def test_l1_ball_is_inclusive_and_the_cap_keeps_the_nearest():
    g = np.arange(5, dtype=np.float64)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    c = int(np.flatnonzero((P == 2).all(1))[0])
    _, cnt, _ = R.compute_features(P, 1.0, qidx=np.array([c]))
    assert cnt[0] == 7
    _, cnt1, _ = R.compute_features(P, 2.0, qidx=np.array([c]), p=1)
    assert cnt1[0] == 25
    _, _, cov = R.neighbourhood_moments(P, np.array([c]), 1.0, max_k=4)
    # kept: the point itself, then the lowest-index three of its six unit neighbours
    kept = P[[c, c - 25, c - 5, c - 1]] - P[c]
    m = kept.mean(0)
    C = (kept - m).T @ (kept - m) / 3
    assert np.allclose(cov[0], C[[0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], atol=1e-15)


@pytest.mark.parametrize("bad", [dict(feature_names=["nope"]), dict(radius=0.0), dict(radius=-1.0),
                                 dict(radius=float("nan")), dict(radius=float("inf")), dict(max_k=0),
                                 dict(metric="chebyshev")])
def test_feature_validation_before_the_device(monkeypatch, bad):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("device called"))
    kw = dict(radius=0.5, feature_names=["planarity"])
    kw.update(bad)
    with pytest.raises(ValueError) as e:
        hip.geometric_features(np.zeros((10, 3)), **kw)
    if "feature_names" in bad:
        assert "verticality" in str(e.value)


@pytest.mark.parametrize("k", [0, 193, 11])
def test_smooth_validation_before_the_device(monkeypatch, k):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("device called"))
    with pytest.raises(ValueError):
        hip.smooth_values(np.zeros((10, 3)), np.zeros(10), k)
    with pytest.raises(ValueError):
        hip.smooth_values(np.zeros((10, 3)), np.zeros(9), 3)
    with pytest.raises(ValueError):
        hip.smooth_values(np.zeros((10, 3)), np.zeros(10), 3, reducer="mode")


@pytest.mark.skipif(_lib.device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_gpu_means_an_error():
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.geometric_features(np.zeros((10, 3)), 0.5)
    assert e.value.code == -3
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.smooth_values(np.zeros((10, 3)), np.zeros(10), 3)
    assert e.value.code == -3
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.smooth_values(np.zeros((10, 3)), np.zeros(10), 3, queries=np.ones((2, 3)))
    assert e.value.code == -3


def test_compute_features_fills_nan_with_the_column_nanmean(monkeypatch):
    raw = np.array([[1.0, np.nan, np.nan], [np.nan, 2.0, np.nan], [3.0, 4.0, np.nan]])
    monkeypatch.setattr(hip, "geometric_features", lambda *a, **k: raw.copy())
    out = exploration.compute_features(np.zeros((3, 3)), 0.6, ["planarity", "linearity", "nz"])
    assert out.dtype == np.float32
    assert np.array_equal(out[:, :2], np.array([[1, 3], [2, 2], [3, 4]], np.float32))
    assert np.isnan(out[:, 2]).all()


def _fake_smooth(monkeypatch, n, k):
    idx = (np.arange(n)[:, None] + np.arange(k)[None, :]) % n

    def fake(xyz, n_, qry, m, vals, F, kk, reducer, out, idx_p, device):
        import ctypes
        if idx_p is not None:
            np.ctypeslib.as_array(ctypes.cast(idx_p, ctypes.POINTER(ctypes.c_int32)), (m, kk))[:] = idx
        if reducer >= 0:
            v = np.ctypeslib.as_array(ctypes.cast(vals, ctypes.POINTER(ctypes.c_double)), (n_, F))
            red = [R.smooth, R.smooth, R.smooth, R.smooth][reducer]
            res = red(v, idx, ["mean", "median", "min", "max"][reducer])
            np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_double)), (m, F))[:] = res
        return 0

    class Lib:
        pyqsm_smooth_values = staticmethod(fake)

    monkeypatch.setattr(_lib, "load", lambda: Lib)
    return idx


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.int64])
@pytest.mark.parametrize("func", [np.mean, np.median, np.min, np.max, np.amin, np.amax, np.std])
def test_smooth_feature_dtypes(monkeypatch, dtype, func):
    n, k = 40, 5
    idx = _fake_smooth(monkeypatch, n, k)
    vals = (np.arange(n) * 3 % 17).astype(dtype)
    want = func(vals[idx], axis=1)
    for got in (exploration.smooth_feature(np.zeros((n, 3)), vals, n_nbrs=k, smoothing_func=func),
                algo.smooth_feature(np.zeros((n, 3)), vals, n_nbrs=k, nbr_func=func)):
        assert got.dtype == want.dtype
        assert got.shape == want.shape
        assert np.allclose(got, want, rtol=1e-6)
    V2 = np.stack([vals, vals[::-1]], 1)
    got2 = algo.smooth_feature(np.zeros((n, 3)), V2, n_nbrs=k, nbr_func=func)
    assert got2.shape == (n, 2) and got2.dtype == func(V2[idx], axis=1).dtype
