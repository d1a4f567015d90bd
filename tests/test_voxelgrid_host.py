"""Detail recovery without a GPU: the restatement of the voxel grid against an independent
formulation and against the cleaning restatement, a lattice whose points sit on voxel faces, the
derived error bound of the sequential neighbour mean, and the C-ABI's argument checks, which run
before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from tests import clean_restatement as C
from tests import voxelgrid_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["pyqsm_radius_reduce", "pyqsm_voxel_grid_create", "pyqsm_voxel_grid_free", "pyqsm_voxel_grid_info",
               "pyqsm_voxel_grid_query", "pyqsm_voxel_grid_query_dev", "pyqsm_voxel_grid_voxels"]


def _cloud(n=4000, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (n, 3)) * np.array([1.0, 0.6, 2.0])


@pytest.mark.parametrize("voxel_size", [0.3, 0.05, 0.011])
def test_membership_equals_a_set_of_index_tuples(voxel_size):
    P = _cloud()
    rng = np.random.default_rng(1)
    Q = np.concatenate([P[:500] + rng.normal(0, voxel_size, (500, 3)), rng.uniform(-3, 3, (500, 3)), P[500:600]])
    g = R.voxel_grid(P, voxel_size)
    origin = P.min(axis=0) - voxel_size * 0.5
    occupied = {tuple(int(v) for v in np.floor((p - origin) / voxel_size)) for p in P}
    want = np.array([tuple(int(v) for v in np.floor((q - origin) / voxel_size)) in occupied for q in Q])
    inc, row, idx, box = R.query(g, Q)
    assert np.array_equal(inc, want)
    assert 0 < inc.sum() < len(Q) and (box & ~inc).any() and (~box).any()
    assert np.array_equal(idx, np.flatnonzero(want))
    assert np.array_equal(R.query(g, Q, invert=True)[2], np.flatnonzero(~want))
    assert g.n_voxels == len(occupied)
    assert {tuple(int(v) for v in r) for r in g.grid_index} == occupied
    assert np.array_equal(g.grid_index[row[inc]], np.floor((Q[inc] - origin) / voxel_size).astype(np.int32))
    assert g.dims == [int(v) + 1 for v in g.grid_index.max(axis=0)]


@pytest.mark.parametrize("voxel_size", [0.3, 0.05])
def test_rows_equal_the_cleaning_restatements_voxel_order(voxel_size):
    P = _cloud(seed=2)
    col = np.random.default_rng(3).uniform(0, 1, P.shape)
    g = R.voxel_grid(P, voxel_size, col)
    means, cmeans, inverse, _, _ = C.voxel_down_sample(P, voxel_size, col)
    assert g.n_voxels == len(means)
    assert np.array_equal(R.query(g, P)[1], inverse)
    assert np.array_equal(g.colors, cmeans)
    # every voxel mean lies in its own voxel
    assert np.array_equal(R.query(g, means)[1], np.arange(g.n_voxels))


def test_lattice_on_voxel_faces():
    pts, qry = R.lattice()
    g = R.voxel_grid(pts, 0.25)
    assert np.array_equal(g.origin, [-0.125] * 3) and g.dims == [6, 6, 6]
    assert g.n_voxels == len(pts) == 108
    inc, row, idx, box = R.query(g, qry)
    n_c = 8 ** 3
    # corners: floor puts a corner into the voxel it is the low corner of; centres likewise
    assert int(inc[:n_c].sum()) == 108 and int(box[:n_c].sum()) == 216
    assert int(inc[n_c:2 * n_c].sum()) == 108 and int(box[n_c:2 * n_c].sum()) == 216
    assert not inc[2 * n_c:].any() and not box[2 * n_c:].any()
    assert np.array_equal(R.query(g, pts)[1], np.arange(108))


def test_empty_and_single_point_grids():
    g = R.voxel_grid(np.zeros((0, 3)), 0.5)
    assert g.n_voxels == 0 and g.dims == [0, 0, 0] and np.array_equal(g.origin, [-0.25] * 3)
    assert not R.query(g, np.zeros((3, 3)))[0].any()
    g = R.voxel_grid(np.array([[1.0, 2.0, 3.0]]), 0.5)
    assert g.dims == [1, 1, 1]
    inc = R.query(g, np.array([[1.0, 2.0, 3.0], [1.24, 2.24, 3.24], [1.25, 2.0, 3.0], [0.74, 2.0, 3.0],
                               [np.nan, 2.0, 3.0], [np.inf, 2.0, 3.0], [1.0, -np.inf, 3.0]]))[0]
    assert inc.tolist() == [True, True, False, False, False, False, False]
    with pytest.raises(R.VoxelRangeError):
        R.voxel_grid(np.array([[0.0, 0, 0], [1e9, 0, 0]]), 1e-3)
    with pytest.raises(R.VoxelRangeError):
        R.voxel_grid(np.array([[0.0, 0, 0], [1e6, 1e6, 1e6]]), 1e-3)


@pytest.mark.parametrize("radius,k", [(0.2, 500), (0.2, 12)])
def test_sequential_mean_is_within_the_derived_bound_of_np_mean(radius, k):
    """A sum of c <= k terms added one at a time carries at most (c - 1) roundings, each at most
    2^-53 relative to a partial sum of at most c * max|v|; the division adds one more. np.mean's
    pairwise sum obeys the same bound, so the two means differ by less than k * 2^-52 * max|v|."""
    src = _cloud(3000, seed=4)
    qry = np.concatenate([_cloud(400, seed=5), [[9.0, 9, 9], [1.0, 0.6, 2.3]]])
    vals = np.random.default_rng(6).normal(0, 10, (len(src), 3))
    idx, cnt, in_range = R.neighbours(src, qry, radius, k)
    assert (cnt == 0).any() and (cnt > 0).any()
    assert (in_range > k).any() == (k == 12)
    out = R.reduce_values(idx, cnt, vals, "mean", empty_row=0)
    bound = k * 2.0 ** -52 * np.abs(vals).max()
    for j in range(len(qry)):
        want = vals[idx[j, :cnt[j]]].mean(axis=0) if cnt[j] else vals[0]
        assert np.all(np.abs(out[j] - want) <= bound), j
    # and the neighbours are those of a brute-force search
    d2 = ((src[None] - qry[:, None]) ** 2).sum(-1)
    assert np.array_equal(np.minimum((d2 < radius * radius).sum(1), k), cnt)
    mn = R.reduce_values(idx, cnt, vals, "min", empty_row=-1)
    first = R.reduce_values(idx, cnt, vals, "first", empty_row=-1)
    for j in range(len(qry)):
        if cnt[j]:
            assert np.array_equal(mn[j], vals[idx[j, :cnt[j]]].min(axis=0))
            assert np.array_equal(first[j], vals[idx[j, 0]])
        else:
            assert np.isnan(mn[j]).all() and np.isnan(first[j]).all()


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "pyqsm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pyqsm_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+PYQSM_VOX_INVERT\s+1\b", text) and hip.VOX_INVERT == 1


def _code(fn):
    with pytest.raises(_lib.PyQSMHipError) as e:
        fn()
    return e.value.code


EINVAL, ENODEV, ERANGE = -1, -3, -4


def test_voxel_grid_arguments_are_checked_before_any_device():
    lib = _lib.load()
    P = np.ascontiguousarray(_cloud(10))
    h = ctypes.c_void_p()

    def create(pts, size):
        return lib.pyqsm_voxel_grid_create(pts.ctypes.data_as(ctypes.c_void_p), len(pts), None, size, 0, ctypes.byref(h))

    for size in (0.0, -1.0, float("nan"), float("inf")):
        assert create(P, size) == EINVAL and h.value is None
    bad = P.copy()
    bad[7, 1] = np.nan
    assert create(bad, 0.1) == EINVAL
    bad[7, 1] = -np.inf
    assert create(bad, 0.1) == EINVAL
    assert create(np.array([[0.0, 0, 0], [1e9, 0, 0]]), 1e-3) == ERANGE      # a dimension above 2^31 - 1
    assert create(np.array([[0.0, 0, 0], [1e6, 1e6, 1e6]]), 1e-3) == ERANGE  # 10^27 cells
    assert lib.pyqsm_voxel_grid_create(None, 5, None, 0.1, 0, ctypes.byref(h)) == EINVAL
    assert lib.pyqsm_voxel_grid_create(P.ctypes.data_as(ctypes.c_void_p), 10, None, 0.1, 0, None) == EINVAL
    assert lib.pyqsm_voxel_grid_free(None) == 0
    junk = (ctypes.c_uint64 * 32)()
    assert lib.pyqsm_voxel_grid_free(ctypes.cast(junk, ctypes.c_void_p)) == EINVAL
    assert lib.pyqsm_voxel_grid_query(ctypes.cast(junk, ctypes.c_void_p), None, 0, 0, None, None, None, None) == EINVAL
    assert lib.pyqsm_voxel_grid_info(None, None, None, None, None, None) == EINVAL
    with pytest.raises(ValueError):
        hip.VoxelGrid(P, 0.0)
    with pytest.raises(ValueError):
        hip.VoxelGrid(P, 0.1, colors=np.zeros((3, 3)))


def test_radius_reduce_arguments_are_checked_before_any_device():
    src, qry = _cloud(20), _cloud(5, seed=1)
    v = np.zeros((20, 2))
    assert _code(lambda: hip.radius_reduce(src, qry, v, 0.1, k=0)) == ERANGE
    assert _code(lambda: hip.radius_reduce(src, qry, v, 0.1, k=2049)) == ERANGE
    assert _code(lambda: hip.radius_reduce(src, qry, np.zeros((20, 65)), 0.1)) == ERANGE
    assert _code(lambda: hip.radius_reduce(src, qry, v, 0.0)) == EINVAL
    assert _code(lambda: hip.radius_reduce(src, qry, v, float("nan"))) == EINVAL
    assert _code(lambda: hip.radius_reduce(src, qry, v, 0.1, empty_row=20)) == EINVAL
    assert _code(lambda: hip.radius_reduce(src, qry, v, 0.1, empty_row=-2)) == EINVAL
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.zeros((5, 2))
    for reducer in (1, 5, -1):   # the median of pyqsm_smooth_values is not offered here
        assert lib.pyqsm_radius_reduce(p(src), 20, p(qry), 5, 0.1, 8, p(v), 2, reducer, 0, p(out), None, 0) == EINVAL
    with pytest.raises(ValueError):
        hip.radius_reduce(src, qry, v, 0.1, reducer="median")
    with pytest.raises(ValueError):
        hip.radius_reduce(src, qry, np.zeros(19), 0.1)
    # no source points: every neighbourhood is empty, and no device is needed to say so
    res, cnt = hip.radius_reduce(np.zeros((0, 3)), qry, np.zeros((0, 2)), 0.1, empty_row=-1, return_counts=True)
    assert np.isnan(res).all() and res.shape == (5, 2) and not cnt.any()


@pytest.mark.skipif(_lib.device_count() > 0, reason="checks the no-GPU failure mode")
def test_no_gpu_means_an_error_not_a_fallback():
    from pyqsm_amd.geometry.cloud import PointCloud, VoxelGrid
    from pyqsm_amd.geometry.reconstruction import expand_features_to_orig, overlap_voxel_grid, transfer_features
    from pyqsm_amd.tree_isolation import unassigned_search_cloud
    P = _cloud(50)
    assert _code(lambda: hip.VoxelGrid(P, 0.1)) == ENODEV
    assert _code(lambda: hip.VoxelGrid(np.zeros((0, 3)), 0.1)) == ENODEV
    assert _code(lambda: hip.radius_reduce(P, P[:5], np.zeros(50), 0.1)) == ENODEV
    assert _code(lambda: VoxelGrid.create_from_point_cloud(PointCloud(P), 0.1)) == ENODEV
    assert _code(lambda: overlap_voxel_grid(P, source_pcd=PointCloud(P))) == ENODEV
    assert _code(lambda: unassigned_search_cloud(PointCloud(P), [P[:10]])) == ENODEV
    assert _code(lambda: transfer_features(P, np.zeros(50), P[:5])) == ENODEV
    assert _code(lambda: expand_features_to_orig(PointCloud(P), PointCloud(P[:5]), {"points": P, "f": np.zeros(50)})) == ENODEV


def test_pcd_tiles_raise_a_clear_error(tmp_path):
    from pyqsm_amd.geometry import reconstruction
    from pyqsm_amd.geometry.cloud import VoxelGrid

    class NoDevice:
        device_grid = None

    (tmp_path / "tile_0.pcd").write_text("# .PCD")
    orig = VoxelGrid.create_from_point_cloud
    VoxelGrid.create_from_point_cloud = staticmethod(lambda *a, **k: NoDevice())
    try:
        with pytest.raises(ValueError, match=r"\.pcd tiles cannot be read"):
            reconstruction.get_nbrs_voxel_grid(_cloud(10), "t", str(tmp_path), "tile_*", out_folder=str(tmp_path / "d"))
    finally:
        VoxelGrid.create_from_point_cloud = orig


def test_tree_isolation_keeps_falling_through():
    import pyqsm_amd.tree_isolation as ti
    assert "pcds_from_extend_seed_file" not in vars(ti)
    assert callable(ti.unassigned_search_cloud)
