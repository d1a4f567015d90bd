"""Cloud cleaning without a GPU: the configuration pyQSM's clean_cloud reads, argument checks that
fire before the library is called, the no-GPU failure mode of the new entry points, and the
restatement (tests/clean_restatement.py) on clouds small enough to work out by hand."""
import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry import cleaning
from pyqsm_amd.geometry.cloud import PointCloud
from pyqsm_amd.set_config import config
from tests import clean_restatement as R


def test_config_has_initial_clean_with_pyqsm_values():
    assert config["initial_clean"] == {"voxel_size": 0.04, "neighbors": 2, "ratio": 4, "iters": 3}


def test_clean_cloud_defaults_come_from_the_config():
    import inspect
    d = inspect.signature(cleaning.clean_cloud).parameters
    assert (d["voxels"].default, d["neighbors"].default, d["ratio"].default, d["iters"].default) == \
        (0.04, 2, 4, 3)


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", boom)


@pytest.mark.parametrize("v", [0.0, -0.1, float("nan"), float("inf")])
def test_bad_voxel_size_raises_before_the_library(no_library, v):
    with pytest.raises(ValueError):
        hip.voxel_down_sample(np.zeros((4, 3)), v)
    with pytest.raises(ValueError):
        PointCloud(np.zeros((4, 3))).voxel_down_sample(v)


@pytest.mark.parametrize("nb,ratio", [(0, 2.0), (-3, 2.0), (2, 0.0), (2, -1.0), (2, float("nan"))])
def test_bad_outlier_arguments_raise_before_the_library(no_library, nb, ratio):
    with pytest.raises(ValueError):
        hip.stat_outlier(np.zeros((4, 3)), nb, ratio)
    with pytest.raises(ValueError):
        PointCloud(np.zeros((4, 3))).remove_statistical_outlier(nb, ratio)
    # (a zero turns clean_cloud's statistical step off, so it takes the nearest bad value instead)
    with pytest.raises(ValueError):
        cleaning.clean_cloud(np.zeros((4, 3)), 0.1, nb or 0.5, ratio or -1.0, 2)


def test_bad_shapes_raise_before_the_library(no_library):
    with pytest.raises(ValueError):
        hip.voxel_down_sample(np.zeros((4, 2)), 0.1)
    with pytest.raises(ValueError):
        hip.voxel_down_sample(np.zeros((4, 3)), 0.1, colors=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        hip.clean_cloud(np.zeros((4, 3)), 0.1, 2, 4, -1)


def test_stat_step_off_returns_the_input_without_the_library(no_library):
    pcd = PointCloud(np.arange(12.0).reshape(4, 3))
    assert cleaning.clean_cloud(pcd, voxels=0.5, neighbors=2, ratio=4, iters=0) is pcd
    assert cleaning.clean_cloud(pcd, voxels=0.5, neighbors=0, ratio=4, iters=3) is pcd


@pytest.mark.skipif(_lib.device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_gpu_means_an_error_not_a_fallback():
    P = np.random.default_rng(0).random((10, 3))
    for call in (lambda: hip.voxel_down_sample(P, 0.1),
                 lambda: hip.stat_outlier(P, 2, 1.0),
                 lambda: hip.clean_cloud(P, 0.1, 2, 4, 3)):
        with pytest.raises(_lib.PyQSMHipError) as e:
            call()
        assert e.value.code == -3


# ---- the restatement on hand-computed clouds ----------------------------------------------------

def test_restated_voxels_by_hand():
    # voxel 0.5 over min x = 0: vmin = -0.25, x keys floor((x + 0.25) / 0.5)
    P = np.array([[1.0, 0, 0], [0.0, 0, 0], [1.02, 0, 0], [0.1, 0, 0], [0.05, 0, 0]])
    C = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0, 1.0, 1.0], [1.0, 1.0, 1.0]])
    means, cm, inv, off, mem = R.voxel_down_sample(P, 0.5, C)
    # row 0 is the voxel of point 0 (x = 1.0, 1.02), row 1 the one of point 1 (x = 0, 0.1, 0.05)
    assert np.array_equal(means[:, 0], [(0.0 + 1.0 + 1.02) / 2, ((0.0 + 0.0) + 0.1 + 0.05) / 3])
    assert np.array_equal(means[:, 1:], np.zeros((2, 2)))
    assert np.array_equal(cm, [[0.5, 0, 0.5], [1 / 3, 1.0, 2 / 3]])
    assert inv.tolist() == [0, 1, 0, 1, 1]
    assert off.tolist() == [0, 2, 5] and mem.tolist() == [0, 2, 1, 3, 4]


def test_restated_voxel_faces_by_hand():
    # vmin = -0.25: x = 0.25 and 0.75 lie exactly on faces and open the next voxel
    P = np.array([[0.0, 0, 0], [0.25, 0, 0], [0.75, 0, 0], [0.7, 0, 0]])
    means, _, inv, off, _ = R.voxel_down_sample(P, 0.5)
    assert inv.tolist() == [0, 1, 2, 1] and off.tolist() == [0, 1, 3, 4]
    assert np.array_equal(means[:, 0], [0.0, (0.25 + 0.7) / 2, 0.75])


def test_restated_voxel_edge_cases():
    assert R.voxel_down_sample(np.zeros((0, 3)), 0.1)[0].shape == (0, 3)
    means, _, inv, off, mem = R.voxel_down_sample(np.array([[3.0, -2.0, 1.0]]), 0.1)
    assert means.tolist() == [[3.0, -2.0, 1.0]] and inv.tolist() == [0] and off.tolist() == [0, 1]
    with pytest.raises(R.VoxelRangeError):
        R.voxel_down_sample(np.array([[0.0, 0, 0], [1000.0, 1000.0, 1000.0]]), 1e-12)
    with pytest.raises(ValueError):
        R.voxel_down_sample(np.zeros((2, 3)), 0.0)


def test_restated_outlier_removal_by_hand():
    # x = 0, 1, 2, 10 with k = 2 (the point itself and its nearest other point):
    # avg = 0.5, 0.5, 0.5, 4; mean = 5.5 / 4 = 1.375; sq = 3 * 0.875^2 + 2.625^2 = 9.1875;
    # std = sqrt(9.1875 / 3) = 1.75
    P = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [10.0, 0, 0]])
    keep, avg, mean, std, thr = R.stat_outlier(P, 2, 1.0)
    assert avg.tolist() == [0.5, 0.5, 0.5, 4.0]
    assert (mean, std, thr) == (1.375, 1.75, 3.125)
    assert keep.tolist() == [0, 1, 2]
    assert R.stat_outlier(P, 2, 2.0)[0].tolist() == [0, 1, 2, 3]        # thr = 4.875
    # k = min(50, 4) = 4: avg of point 0 = (0 + 1 + 2 + 10) / 4
    assert R.stat_outlier(P, 50, 1.0)[1][0] == 13.0 / 4


def test_restated_outlier_duplicates_and_tiny_clouds():
    P = np.array([[0.0, 0, 0], [0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [3.0, 0, 0], [6.0, 0, 0]])
    keep, avg, *_ = R.stat_outlier(P, 2, 10.0)
    assert avg.tolist() == [0.0, 0.0, 0.5, 0.0, 0.0, 1.5]
    assert keep.tolist() == [2, 5]                                        # avg == 0 is dropped
    assert R.stat_outlier(P[:1], 2, 4.0)[0].size == 0                     # n = 1: 0 / 0
    assert R.stat_outlier(P[:0], 2, 4.0)[0].size == 0


def test_restated_clean_cloud_loop():
    P = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [10.0, 0, 0], [0.01, 0, 0]])
    # stat step off: the input comes back even with a voxel size
    assert np.array_equal(R.clean_cloud(P, 0.5, 2, 4, 0), P)
    assert np.array_equal(R.clean_cloud(P, 0.5, 0, 4, 3), P)
    # voxel 0.5 merges 0 and 0.01; one round at k = 2, ratio 1: x = 0.005, 1, 2, 10
    out = R.clean_cloud(P, 0.5, 2, 1.0, 1)
    assert np.array_equal(out[:, 0], [0.005, 1.0, 2.0])
