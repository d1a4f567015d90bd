"""The device voxel grid against tests/voxelgrid_restatement.py on an MI355X: a 200 000-point tile
checked against the grid of a 12 500-point tree at three voxel sizes (the last one a grid of
7.7e9 cells: 64-bit keys), exact in every output."""
import numpy as np
import pytest

from pyqsm_amd import hip
from pyqsm_amd.geometry.cloud import PointCloud, VoxelGrid
from tests import voxelgrid_restatement as R

pytestmark = pytest.mark.gpu

SIZES = [0.1, 0.02, 0.004]
VOXELS = {0.1: 2446, 0.02: 11222, 0.004: 12479}


def _shares(voxel_size):
    """The restatement's grid and tile query, with every branch of the kernel populated."""
    g, (inc, row, idx, box) = R.detail_grid(voxel_size, colored=True)
    assert g.n_voxels == VOXELS[voxel_size]
    assert inc.mean() >= 0.05 and (~box).mean() >= 0.05
    if voxel_size != 0.1:
        assert (box & ~inc).mean() >= 0.05
    assert (g.cells > 2 ** 32) == (voxel_size == 0.004)
    return g, inc, row, idx


@pytest.fixture(scope="module")
def grids(gpu):
    _, _, comp = R.detail_inputs()
    made = {s: hip.VoxelGrid(comp, s, colors=R.detail_colors()) for s in SIZES}
    yield made
    for g in made.values():
        g.close()


@pytest.mark.parametrize("voxel_size", SIZES)
@pytest.mark.parametrize("invert", [False, True])
def test_tile_query_equals_restatement(grids, voxel_size, invert):
    tile, _, _ = R.detail_inputs()
    g, inc, row, idx = _shares(voxel_size)
    d = grids[voxel_size]
    assert d.n_voxels == g.n_voxels and d.dims.tolist() == g.dims
    assert np.array_equal(d.origin, g.origin) and d.voxel_size == voxel_size
    got_inc, got_row, got_idx = d.query(tile, rows=True, indices=True, invert=invert)
    assert got_inc.dtype == bool and got_row.dtype == np.int32 and got_idx.dtype == np.int64
    assert np.array_equal(got_inc, inc)
    assert np.array_equal(got_row, row)
    assert np.array_equal(got_idx, np.flatnonzero(inc != invert))
    # outputs asked for one at a time
    assert np.array_equal(d.query(tile), inc)
    assert np.array_equal(d.query(tile, indices=True, invert=invert)[1], got_idx)


@pytest.mark.parametrize("voxel_size", [0.02, 0.004])
@pytest.mark.parametrize("invert", [False, True])
def test_chunked_host_form_equals_resident_form(grids, voxel_size, invert, monkeypatch):
    tile, _, _ = R.detail_inputs()
    _, inc, row, _ = _shares(voxel_size)
    d = grids[voxel_size]
    m = len(tile)
    q = hip.DeviceBuffer.from_array(tile)
    b_inc, b_row, b_idx = hip.DeviceBuffer(m), hip.DeviceBuffer(4 * m), hip.DeviceBuffer(8 * m)
    cnt = d.query_dev(q.ptr, m, b_inc.ptr, b_row.ptr, b_idx.ptr, invert=invert)
    dev = (b_inc.download(m, np.uint8).astype(bool), b_row.download(m, np.int32), b_idx.download(m, np.int64)[:cnt])
    assert d.query_dev(q.ptr, m, None, None, None, invert=invert) == cnt   # the count alone
    for buf in (q, b_inc, b_row, b_idx):
        buf.free()
    monkeypatch.setenv("PYQSM_VOX_CHUNK", "70001")   # three passes, the last one of 59 998
    host = d.query(tile, rows=True, indices=True, invert=invert)
    for a, b in zip(host, dev):
        assert np.array_equal(a, b)
    assert np.array_equal(host[0], inc) and np.array_equal(host[1], row)
    assert cnt == int((inc != invert).sum())


@pytest.mark.parametrize("voxel_size", SIZES)
def test_voxels_equal_restatement_bit_for_bit(grids, voxel_size):
    g = _shares(voxel_size)[0]
    gi, col = grids[voxel_size].voxels()
    assert gi.dtype == np.int32 and np.array_equal(gi, g.grid_index)
    assert np.array_equal(col, g.colors)
    assert grids[voxel_size].device_bytes > 0


@pytest.mark.parametrize("voxel_size", SIZES)
def test_a_cloud_in_its_own_grid_gives_the_down_sampling_trace(grids, voxel_size):
    _, _, comp = R.detail_inputs()
    xyz, _, (inverse, _, _) = hip.voxel_down_sample(comp, voxel_size, return_trace=True)
    inc, row = grids[voxel_size].query(comp, rows=True)
    assert inc.all() and np.array_equal(row, inverse)
    assert grids[voxel_size].n_voxels == len(xyz)


def test_lattice_on_voxel_faces(gpu):
    pts, qry = R.lattice()
    want = R.query(R.voxel_grid(pts, 0.25), qry)
    with hip.VoxelGrid(pts, 0.25) as d:
        assert d.dims.tolist() == [6, 6, 6] and d.n_voxels == 108
        inc, row, idx = d.query(qry, rows=True, indices=True)
    assert np.array_equal(inc, want[0]) and np.array_equal(row, want[1]) and np.array_equal(idx, want[2])
    assert int(inc.sum()) == 216


def test_coordinates_that_are_not_fp32_representable(gpu):
    tile, _, comp = R.detail_inputs()
    rng = np.random.default_rng(5)
    comp = comp + rng.uniform(-1e-9, 1e-9, comp.shape)
    qry = tile[:60_000] + rng.uniform(-1e-9, 1e-9, (60_000, 3))
    assert not np.array_equal(comp.astype(np.float32).astype(np.float64), comp)
    g = R.voxel_grid(comp, 0.02)
    want = R.query(g, qry)
    assert 0.05 < want[0].mean() < 0.95
    with hip.VoxelGrid(comp, 0.02) as d:
        inc, row = d.query(qry, rows=True)
        assert np.array_equal(d.origin, g.origin)
    assert np.array_equal(inc, want[0]) and np.array_equal(row, want[1])


def test_non_finite_queries_are_not_included(grids):
    _, _, comp = R.detail_inputs()
    q = np.repeat(comp[:1], 8, axis=0)
    q[1, 0], q[2, 1], q[3, 2] = np.nan, np.inf, -np.inf
    q[4] = np.nan
    q[5] = [np.inf, -np.inf, np.nan]
    q[6] = 1e300
    for d in grids.values():
        inc, row, idx = d.query(q, rows=True, indices=True, invert=True)
        assert inc.tolist() == [True, False, False, False, False, False, False, True]
        assert (row[1:7] == -1).all() and idx.tolist() == [1, 2, 3, 4, 5, 6]


def test_empty_grid_and_single_point(gpu):
    tile, _, _ = R.detail_inputs()
    with hip.VoxelGrid(np.zeros((0, 3)), 0.5) as d:
        assert d.n_voxels == 0 and d.dims.tolist() == [0, 0, 0] and np.array_equal(d.origin, [-0.25] * 3)
        inc, row, idx = d.query(tile[:1000], rows=True, indices=True)
        assert not inc.any() and (row == -1).all() and len(idx) == 0
        assert len(d.query(tile[:1000], indices=True, invert=True)[1]) == 1000
        assert d.voxels()[0].shape == (0, 3)
        assert d.query(np.zeros((0, 3))).shape == (0,)
    p = np.array([[1.0, 2.0, 3.0]])
    with hip.VoxelGrid(p, 0.5, colors=np.array([[0.25, 0.5, 1.0]])) as d:
        assert d.n_voxels == 1 and d.dims.tolist() == [1, 1, 1]
        q = np.array([[1.0, 2.0, 3.0], [1.24, 2.24, 3.24], [1.25, 2.0, 3.0], [0.74, 2.0, 3.0]])
        assert d.query(q).tolist() == [True, True, False, False]
        gi, col = d.voxels()
        assert gi.tolist() == [[0, 0, 0]] and col.tolist() == [[0.25, 0.5, 1.0]]
    with pytest.raises(ValueError):
        d.query(q)   # closed


def test_two_grids_alive_at_once(gpu):
    tile, tree, comp = R.detail_inputs()
    other = tile[50_000:100_000:4]
    a, b = hip.VoxelGrid(comp, 0.1), hip.VoxelGrid(other, 0.05)
    wa, wb = R.query(R.voxel_grid(comp, 0.1), tile)[0], R.query(R.voxel_grid(other, 0.05), tile)[0]
    assert np.array_equal(b.query(tile), wb) and np.array_equal(a.query(tile), wa)
    assert np.array_equal(b.query(tile), wb)
    assert not (wa & wb).all() and wa.any() and wb.any()
    a.close()
    assert np.array_equal(b.query(tile), wb)
    b.close()
    b.close()   # a second close is a no-op


def test_open3d_style_grid_and_wrappers(gpu, tmp_path):
    from pyqsm_amd.geometry.reconstruction import get_nbrs_voxel_grid, overlap_voxel_grid
    from pyqsm_amd.tree_isolation import unassigned_search_cloud
    tile, tree, comp = R.detail_inputs()
    comp_pcd = PointCloud(comp, colors=R.detail_colors())
    vg = VoxelGrid.create_from_point_cloud(comp_pcd, voxel_size=0.1)
    g, inc, row, idx = _shares(0.1)
    assert np.array_equal(vg.check_if_included(tile), inc)
    assert np.array_equal(vg.origin, g.origin) and vg.voxel_size == 0.1
    vox = vg.get_voxels()
    assert len(vox) == g.n_voxels and np.array_equal(vox[7].grid_index, g.grid_index[7])
    assert np.array_equal(vox[7].color, g.colors[7])
    # overlap_voxel_grid: a given grid, the default 0.2 grid of source_pcd, and the complement
    assert np.array_equal(overlap_voxel_grid(tile, vg), idx)
    assert np.array_equal(overlap_voxel_grid(tile, vg, invert=True), np.flatnonzero(~inc))
    w2 = R.query(R.voxel_grid(comp, 0.2), tile)[2]
    assert np.array_equal(overlap_voxel_grid(tile, source_pcd=comp_pcd), w2)
    far = tile + 100.0
    empty = overlap_voxel_grid(far, vg)
    assert empty.dtype == np.int64 and len(empty) == 0
    # unassigned_search_cloud: the points in no voxel of the clusters' union
    search, uniques = unassigned_search_cloud(PointCloud(tile), [comp[:5000], PointCloud(comp[5000:])])
    assert np.array_equal(uniques, np.flatnonzero(~inc)) and np.array_equal(search.points, tile[~inc])
    # get_nbrs_voxel_grid over two tiles; the second misses the box of the comp cloud and is skipped
    t0, t1 = tile[:60_000], tile[150_000:] + np.array([50.0, 0, 0])
    np.savez(tmp_path / "tile_0.npz", points=t0, intensity=np.arange(60_000.0), colors=np.tile(t0, 1))
    np.savez(tmp_path / "tile_1.npz", points=t1, intensity=np.arange(50_000.0), colors=np.tile(t1, 1))
    out = get_nbrs_voxel_grid(comp_pcd, "tree0", str(tmp_path), "tile_*.npz", out_folder=str(tmp_path / "detail"))
    want = idx[idx < 60_000]
    assert np.array_equal(out["points"], t0[want]) and np.array_equal(out["intensity"], want.astype(float))
    saved = np.load(tmp_path / "color_int_tree_nbrs" / "tile_0" / "detail_feats_tree0.npz")["nbrs"]
    assert np.array_equal(saved, want)
    assert not (tmp_path / "color_int_tree_nbrs" / "tile_1").exists()
    joined = np.load(tmp_path / "detail" / "tree0.npz")
    assert sorted(joined.files) == ["colors", "intensity", "points"] and np.array_equal(joined["points"], t0[want])
