"""pyqsm_points_in_boxes on the GPU against its rule restated in NumPy (tests/hull_restatement.py
boxes_rule, held against a plain loop by tests/test_hull_host.py): bit for bit, faces included."""
import functools

import numpy as np
import pytest

from pyqsm_amd import hip
from pyqsm_amd.geometry import hull as gh
from pyqsm_amd.geometry import point_cloud_processing as pcp
from pyqsm_amd.geometry.cloud import PointCloud
from tests import hull_restatement as hr

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def scene():
    """100 000 points (not a multiple of a wave's 512), a PCA box rotated off axis, an axis-aligned box
    with points exactly on its faces, and a box far away."""
    rng = np.random.default_rng(31)
    pts = rng.normal(size=(100_000, 3)) * [4.0, 2.0, 1.0]
    ang = 0.6
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
    pts = pts @ Rz.T
    faces = np.array([[1.5, 0.25, 0.5], [-1.5, -1, 0], [0.5, 2.0, -0.5], [0.25, -2.0, 0.125], [0, 0.5, 0.75],
                      [1.5, 2.0, 0.75], [-1.5, -2.0, -0.75], [1.5000000000000002, 0, 0]])
    where = np.array([0, 63, 64, 511, 512, 51_234, 99_998, 99_999])
    pts[where] = faces
    pca = gh.OrientedBoundingBox.from_hull_points(pts[::50][:400])
    boxes = np.array([pca.as_row(),
                      np.r_[0, 0, 0, np.eye(3).ravel(), 1.5, 2.0, 0.75],
                      np.r_[500.0, 500.0, 500.0, Rz.ravel(), 1, 1, 1]])
    pts.setflags(write=False)
    return pts, boxes, where, hr.boxes_rule(pts, boxes)


def test_three_boxes_equal_the_rule(gpu):
    pts, boxes, where, (ptr0, idx0) = scene()
    ptr, idx = hip.points_in_boxes(pts, boxes)
    assert ptr.dtype == np.int64 and idx.dtype == np.int64
    assert np.array_equal(ptr, ptr0) and np.array_equal(idx, idx0)
    assert not np.allclose(boxes[0, 3:12].reshape(3, 3), np.eye(3)) and ptr[1] > 1000
    assert set(where[:7].tolist()) <= set(idx[ptr[1]:ptr[2]].tolist())       # on the faces: inside
    assert where[7] not in set(idx[ptr[1]:ptr[2]].tolist())                  # one ulp beyond: outside
    assert ptr[3] == ptr[2]                                                   # the far box holds nothing


def test_device_form_gives_the_same(gpu):
    pts, boxes, _, (ptr0, idx0) = scene()
    buf = hip.DeviceBuffer.from_array(pts)
    try:
        for part in (boxes, boxes[1:2], boxes[2:]):
            ptr, idx = hip.points_in_boxes(buf, part)
            want = hr.boxes_rule(pts, part) if part is not boxes else (ptr0, idx0)
            assert np.array_equal(ptr, want[0]) and np.array_equal(idx, want[1])
    finally:
        buf.free()


def test_257_boxes_are_chunked(gpu):
    pts, boxes, _, _ = scene()
    sub = np.ascontiguousarray(pts[:5000])
    rng = np.random.default_rng(32)
    many = np.tile(boxes[1], (257, 1))
    many[:, :3] = rng.normal(size=(257, 3)) * [4.0, 2.0, 1.0]
    many[:, 12:] = rng.uniform(0.0, 1.0, (257, 3))
    many[256] = boxes[0]
    ptr, idx = hip.points_in_boxes(sub, many)
    ptr0, idx0 = hr.boxes_rule(sub, many)
    assert len(ptr) == 258 and np.array_equal(ptr, ptr0) and np.array_equal(idx, idx0)


def test_zero_extent_and_empty_inputs(gpu):
    pts, boxes, where, _ = scene()
    dot = np.r_[pts[64], boxes[0, 3:12], 0, 0, 0][None, :]
    ptr, idx = hip.points_in_boxes(pts, dot)
    assert np.array_equal(ptr, hr.boxes_rule(pts, dot)[0]) and idx.tolist() == [64]
    ptr, idx = hip.points_in_boxes(np.zeros((0, 3)), boxes)
    assert ptr.tolist() == [0, 0, 0, 0] and len(idx) == 0
    ptr, idx = hip.points_in_boxes(pts, np.zeros((0, 15)))
    assert ptr.tolist() == [0] and len(idx) == 0


def test_box_object_and_query_via_bnd_box(gpu):
    rng = np.random.default_rng(33)
    trunk = np.c_[rng.normal(0, 0.15, (1500, 2)), rng.uniform(0, 3, 1500)]
    branches = np.concatenate([np.c_[rng.uniform(0, 1.5, 700), rng.normal(0, 0.05, 700), 2.0 + rng.uniform(0, 1.2, 700)],
                               np.c_[rng.normal(0, 0.05, 700), rng.uniform(-1.5, 0, 700), 2.5 + rng.uniform(0, 1.5, 700)]])
    source = np.concatenate([trunk, branches])
    pcd, src = PointCloud(trunk), PointCloud(source)
    obb = pcd.get_oriented_bounding_box()
    inside = obb.get_point_indices_within_bounding_box(source)
    assert np.array_equal(inside, hr.boxes_rule(source, obb.as_row()[None, :])[1])
    shifted = gh.OrientedBoundingBox(obb.center, obb.R, obb.extent).translate((0, 0, 1), relative=True)
    shifted.scale(1.1, center=obb.center)
    ptr, idx = hr.boxes_rule(source, np.array([shifted.as_row(), obb.as_row()]))
    want = np.setdiff1d(idx[ptr[0]:ptr[1]], idx[ptr[1]:ptr[2]])
    nbrs, new_idx = pcp.query_via_bnd_box(pcd, src)
    assert np.array_equal(new_idx, want) and len(want) > 0
    assert np.array_equal(np.asarray(nbrs.points), source[want])
