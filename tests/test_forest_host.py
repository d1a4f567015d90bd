"""Tree-ensemble inference, the part that needs no GPU: the NumPy restatement
(tests/forest_restatement.py) against a live scikit-learn and against the stored fixture, the
float32-floor threshold rule, conversion, and what is rejected before any device call."""
import os

import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.math_utils.forest import GPUForest
from tests import forest_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forest_small.npz")


def _fit(kind, C, F, T, n=1500, seed=0):
    from sklearn.ensemble import ExtraTreesClassifier, RandomForestClassifier
    from sklearn.tree import DecisionTreeClassifier
    X, y = R.gaussian_classes(n + 800, F, C, seed=seed, spread=0.5)
    y[:C] = np.arange(C)                       # every class present
    if kind == "tree":
        model = DecisionTreeClassifier(random_state=seed)
    else:
        cls = RandomForestClassifier if kind == "rf" else ExtraTreesClassifier
        model = cls(n_estimators=T, random_state=seed, n_jobs=1)
    model.fit(X[:n], y[:n])
    Xq = X[n:].copy()
    Xq[::11, (np.arange(0, len(Xq), 11) % F)] = np.nan
    return model, Xq


CASES = [("rf", 2, 1, 31), ("rf", 3, 7, 31), ("rf", 7, 32, 31), ("rf", 3, 7, 1),
         ("et", 2, 1, 31), ("et", 3, 7, 31), ("et", 7, 32, 31), ("et", 7, 32, 1),
         ("tree", 2, 1, 1), ("tree", 3, 7, 1), ("tree", 7, 32, 1)]


@pytest.mark.parametrize("kind,C,F,T", CASES)
def test_restatement_equals_sklearn(kind, C, F, T):
    model, Xq = _fit(kind, C, F, T)
    trees = R.trees_of(model)
    leaves = R.apply(trees, Xq)
    want = model.apply(Xq)
    assert np.array_equal(leaves if kind != "tree" else leaves[:, 0], want)
    proba = R.predict_proba(trees, Xq, leaves)
    ref = model.predict_proba(Xq)
    assert proba.dtype == ref.dtype == np.float64
    assert np.array_equal(proba.view(np.uint64), ref.view(np.uint64))
    assert np.array_equal(model.classes_[R.predict_index(trees, Xq, proba)], model.predict(Xq))


@pytest.mark.parametrize("kind,C,F,T", [("rf", 3, 7, 31), ("rf", 2, 1, 31), ("et", 7, 32, 31), ("tree", 3, 7, 1)])
def test_float32_floor_threshold_rule(kind, C, F, T):
    """For a float32 x, (double)x <= t and x <= t32 (t32 the largest float32 not above t) are the
    same predicate: checked at t32 and its two float32 neighbours for every internal node."""
    model, _ = _fit(kind, C, F, T)
    checked = 0
    for left, _, _, threshold, _, _ in R.trees_of(model):
        t = threshold[left != -1]
        t32 = R.floor_f32(t)
        assert (t32.astype(np.float64) <= t).all()
        assert (np.nextafter(t32, np.float32(np.inf)).astype(np.float64) > t).all()
        for x in (np.nextafter(t32, np.float32(-np.inf)), t32, np.nextafter(t32, np.float32(np.inf))):
            assert x.dtype == np.float32
            assert np.array_equal(x.astype(np.float64) <= t, x <= t32)
        checked += t.size
    assert checked > 0


def test_floor_f32_edge_values():
    t = np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -30, -1.0 - 2.0 ** -30, 1e300, -1e300, 3.5e38, 2.0 ** -160])
    t32 = R.floor_f32(t)
    fmax = np.finfo(np.float32).max
    assert t32[2] == 1.0 and t32[3] == 1.0 and t32[4] == np.nextafter(np.float32(-1), np.float32(-2))
    assert t32[5] == fmax and t32[6] == -np.inf and t32[7] == fmax and t32[8] == 0.0
    for x in np.array([0.0, -0.0, 1.0, -1.0, fmax, -fmax, 1e-45], np.float32):
        assert np.array_equal(np.float64(x) <= t, x <= t32)


def test_restatement_equals_the_fixture():
    g = np.load(GOLDEN)
    f = GPUForest(g["tree_offsets"], g["left"], g["right"], g["feature"], g["threshold"], g["missing_left"],
                  g["value"], g["classes"], g["X"].shape[1])
    trees = f.unpack()
    assert len(trees) == 15
    leaves = R.apply(trees, g["X"])
    assert np.array_equal(leaves, g["apply"])
    proba = R.predict_proba(trees, g["X"], leaves)
    assert np.array_equal(proba.view(np.uint64), g["predict_proba"].view(np.uint64))
    assert np.array_equal(g["classes"][R.predict_index(trees, g["X"], proba)], g["predict"])
    srt = np.sort(proba, axis=1)
    assert (srt[:, -1] == srt[:, -2]).sum() >= 50          # the tie rule is exercised
    assert np.isnan(g["X"]).any()
    # the device's float32 records walk the same way
    for k, t in enumerate(trees):
        assert np.array_equal(R.apply_tree(t, g["X"], wide_compare=False, t32=R.floor_f32(t[3])), g["apply"][:, k])
    assert os.path.getsize(GOLDEN) <= 710 * 1024


@pytest.mark.parametrize("kind,T", [("rf", 5), ("et", 5), ("tree", 1)])
def test_conversion_round_trip(kind, T):
    model, _ = _fit(kind, 3, 7, T, n=400)
    f = GPUForest.from_sklearn(model)
    assert f.n_trees == T and f.n_features_in_ == 7 and np.array_equal(f.classes_, model.classes_)
    assert f.single_tree == (kind == "tree")
    assert f.left.dtype == np.int32 and f.threshold.dtype == np.float64 and f.missing_left.dtype == np.uint8
    assert f.tree_offsets[0] == 0 and f.tree_offsets[-1] == len(f.left) == len(f.value)
    want = R.trees_of(model)
    got = f.unpack()
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    again = GPUForest.from_arrays(got, f.classes_, 7, single_tree=f.single_tree)
    for name in ("tree_offsets", "left", "right", "feature", "threshold", "missing_left", "value"):
        assert np.array_equal(getattr(again, name), getattr(f, name)), name


def test_string_classes_convert():
    from sklearn.tree import DecisionTreeClassifier
    X, y = R.gaussian_classes(200, 3, 3, seed=2)
    names = np.array(["epiphyte", "leaf", "wood"])
    f = GPUForest.from_sklearn(DecisionTreeClassifier(random_state=0).fit(X, names[y]))
    assert list(f.classes_) == list(names)


def test_regressors_and_multi_output_are_rejected():
    from sklearn.ensemble import RandomForestClassifier, RandomForestRegressor
    from sklearn.tree import DecisionTreeRegressor
    X, y = R.gaussian_classes(200, 4, 3, seed=1)
    with pytest.raises(ValueError, match="regressor"):
        GPUForest.from_sklearn(RandomForestRegressor(n_estimators=3, random_state=0).fit(X, y))
    with pytest.raises(ValueError, match="regressor"):
        GPUForest.from_sklearn(DecisionTreeRegressor(random_state=0).fit(X, y))
    multi = RandomForestClassifier(n_estimators=3, random_state=0).fit(X, np.stack([y, 2 - y], axis=1))
    with pytest.raises(ValueError, match="multi-output"):
        GPUForest.from_sklearn(multi)
    with pytest.raises(ValueError, match="regressor|unfitted"):
        GPUForest.from_sklearn(RandomForestClassifier())


def test_rows_are_checked_like_sklearn():
    ok = hip.forest_rows(np.array([[1.0, np.nan], [2, 3]]), 2)
    assert ok.dtype == np.float32 and ok.flags.c_contiguous and np.isnan(ok[0, 1])
    for bad in (np.inf, -np.inf, 1e39, -1e300):
        with pytest.raises(ValueError, match="infinity or a value too large"):
            hip.forest_rows(np.array([[1.0, bad]]), 2)
    with pytest.raises(ValueError, match="features"):
        hip.forest_rows(np.zeros((3, 3)), 2)
    with pytest.raises(ValueError, match="2D"):
        hip.forest_rows(np.zeros(3), 3)
    assert hip.forest_rows(np.zeros((0, 2)), 2).shape == (0, 2)


def _stump():
    """(tree_offsets, left, right, feature, threshold, missing_left, value): one split, two leaves."""
    return [np.array([0, 3]), np.array([1, -1, -1]), np.array([2, -1, -1]), np.array([0, -2, -2]),
            np.array([0.5, -2.0, -2.0]), np.zeros(3, np.uint8), np.array([[0.5, 0.5], [1.0, 0.0], [0.0, 1.0]])]


MALFORMED = {
    "left child out of range": lambda a: a[1].__setitem__(0, 3),
    "right child negative": lambda a: a[2].__setitem__(0, -5),
    "a cycle": lambda a: (a[1].__setitem__(1, 0), a[2].__setitem__(1, 2)),
    "both children the same node": lambda a: a[2].__setitem__(0, 1),
    "one child only": lambda a: a[2].__setitem__(1, 2),
    "feature out of range": lambda a: a[3].__setitem__(0, 2),
    "negative feature": lambda a: a[3].__setitem__(0, -1),
    "NaN threshold": lambda a: a[4].__setitem__(0, np.nan),
    "NaN leaf value": lambda a: a[6].__setitem__((1, 0), np.nan),
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_forests_are_an_error_code(what):
    """The topology is validated on the host, before the device is looked for: EINVAL with or
    without a GPU, never a kernel that walks out of bounds."""
    a = _stump()
    MALFORMED[what](a)
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.DeviceForest(*a, n_features=2)
    assert e.value.code == -1, what


def test_arguments_are_checked_before_any_device_call():
    a = _stump()
    with pytest.raises(ValueError, match="n_features"):
        hip.DeviceForest(*a, n_features=hip.FOREST_MAX_FEATURES + 1)
    with pytest.raises(ValueError, match="n_features"):
        hip.DeviceForest(*a, n_features=0)
    with pytest.raises(ValueError, match="tree_offsets"):
        hip.DeviceForest(np.array([0, 0, 3]), *a[1:], n_features=2)
    with pytest.raises(ValueError, match="shape"):
        hip.DeviceForest(a[0], a[1][:2], *a[2:], n_features=2)
    wide = np.zeros((3, hip.FOREST_MAX_CLASSES + 1))
    with pytest.raises(ValueError, match="classes"):
        hip.DeviceForest(*a[:6], wide, n_features=2)
    lib = _lib.load()
    assert lib.pyqsm_forest_predict(None, None, 0, None, None, None) == -1
    assert lib.pyqsm_forest_info(None, None) == -1
    assert lib.pyqsm_forest_stage(None, 0) == -1
    assert lib.pyqsm_forest_free(None) == 0


def test_limits_of_the_header_and_the_wrapper_agree():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                             "pyqsm_hip.h")).read()
    import re
    macro = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (PYQSM_FOREST_MAX_\w+) (\d+)", text)}
    assert macro == {"PYQSM_FOREST_MAX_FEATURES": hip.FOREST_MAX_FEATURES,
                     "PYQSM_FOREST_MAX_CLASSES": hip.FOREST_MAX_CLASSES,
                     "PYQSM_FOREST_MAX_TREE_NODES": hip.FOREST_MAX_TREE_NODES}


@pytest.mark.skipif(_lib.device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_gpu_means_an_error_not_a_fallback():
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.DeviceForest(*_stump(), n_features=2)
    assert e.value.code == -3
    g = np.load(GOLDEN)
    f = GPUForest(g["tree_offsets"], g["left"], g["right"], g["feature"], g["threshold"], g["missing_left"],
                  g["value"], g["classes"], g["X"].shape[1])
    for call in (f.predict_proba, f.predict, f.apply):
        with pytest.raises(_lib.PyQSMHipError) as e:
            call(g["X"])
        assert e.value.code == -3


def test_exploration_defines_the_classification():
    from pyqsm_amd import exploration
    assert exploration.random_forest_classification.__module__ == "pyqsm_amd.exploration"
