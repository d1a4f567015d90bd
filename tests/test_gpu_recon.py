"""pyqsm_ball_pivot on the GPU against the CPU statements of its contract (tests/recon_restatement.py;
tests/test_recon_host.py pins the brute-force definition to the Delaunay route on the clouds in general
position): triangle arrays and levels are compared as integers, never within a tolerance."""
import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry import mesh_processing as mp
from pyqsm_amd.geometry import point_cloud_processing as pcp
from pyqsm_amd.geometry import surf_recon
from pyqsm_amd.geometry.cloud import PointCloud, TriangleMesh
from tests import recon_cases as C
from tests import recon_restatement as R

pytestmark = pytest.mark.gpu


def assert_same(res, ref):
    T, lv, unresolved = ref
    assert res.triangles.dtype == np.int32 and res.levels.dtype == np.int32
    assert np.array_equal(res.triangles, T)
    assert np.array_equal(res.levels, lv)
    assert res.n_unresolved_ties == unresolved


def float_cloud(P, Nr):
    """The lattice cloud as a PointCloud: snapping at quantum 1 gives it back."""
    return PointCloud(P.astype(np.float64), normals=Nr.astype(np.float64) / (1 << 14))


def test_sphere_is_closed(gpu):
    P, Nr, rho2 = R.sphere()
    res = hip.ball_pivot(P, Nr, rho2)
    assert_same(res, R.delaunay(P, Nr, rho2))
    T = res.triangles
    assert len(T) == 2 * len(P) - 4
    half = R.half_edges(T)
    assert len(set(half)) == len(half) and R.open_half_edges(T) == []
    assert (T[:, 0] < T[:, 1]).all() and (T[:, 0] < T[:, 2]).all()
    assert TriangleMesh(P.astype(np.float64), T).is_watertight()
    assert res.stats["tests"] > 0 and res.stats["tests"] <= res.stats["candidates"] * res.stats["max_stencil"]


def test_second_radius_closes_the_hole(gpu):
    P, Nr, rho2 = R.holed_sphere()
    ref = R.delaunay(P, Nr, rho2)
    first = hip.ball_pivot(P, Nr, rho2[:1])
    assert np.array_equal(first.triangles, ref[0][ref[1] == 0])
    rim = R.open_half_edges(first.triangles)
    assert len(rim) > 3 and R.loops(rim) == 1                   # one open loop
    both = hip.ball_pivot(P, Nr, rho2[::-1])                    # any order: processed ascending
    assert_same(both, ref)
    assert (both.levels == 1).sum() > 0 and R.open_half_edges(both.triangles) == []
    assert np.array_equal(both.triangles[both.levels == 0], first.triangles)


def test_plane_grid_tie_rule(gpu):
    P, Nr, rho2 = R.plane_grid()
    res = hip.ball_pivot(P, Nr, rho2)
    assert_same(res, R.brute(P, Nr, rho2))
    T = res.triangles
    assert len(T) == 72 and R.twice_area(P, T) == 720000
    half = R.half_edges(T)
    assert len(set(half)) == len(half)
    assert res.stats["exact_fallbacks"] > 0                      # cocircular squares: settled by the integers
    # all normals flipped: the same triangles, traversed the other way
    flipped = hip.ball_pivot(P, -Nr, rho2)
    assert sorted(map(tuple, flipped.triangles[:, [0, 2, 1]].tolist())) == sorted(map(tuple, T.tolist()))
    assert_same(flipped, R.brute(P, -Nr, rho2))
    # one normal flipped: no triangle touches that vertex
    v = 17
    one = Nr.copy()
    one[v] = -one[v]
    res1 = hip.ball_pivot(P, one, rho2)
    assert_same(res1, R.brute(P, one, rho2))
    assert len(res1.triangles) > 0 and not (res1.triangles == v).any()


def test_nested_surfaces_slices_chunks_and_empty_cells(gpu):
    P, Nr, rho2 = R.nested_surfaces()
    res = hip.ball_pivot(P, Nr, rho2)
    assert_same(res, R.delaunay(P, Nr, rho2))
    assert len(res.triangles) > 5000
    # the shapes this cloud is for, from the sizes
    assert res.stats["max_cell_points"] > hip.RECON_SLICE        # a cell takes several blocks
    assert res.stats["max_stencil"] > hip.RECON_CHUNK            # the LDS chunk is refilled
    edge = int(np.ceil(2 * np.sqrt(rho2[0]))) + 1
    cells = P // edge
    dims = cells.max(axis=0) + 1
    occupied = len(np.unique(cells @ np.array([1, dims[0], dims[0] * dims[1]])))
    assert occupied < int(dims.prod())                           # some cells are empty
    # The grid puts one empty border cell around the dims interior cells: an occupied cell with index 0 or
    # dims - 1 on an axis has border cells in its 27-cell stencil. Here every face of the box has such cells.
    for axis in range(3):
        assert (cells[:, axis] == 0).any() and (cells[:, axis] == dims[axis] - 1).any()


def test_same_bytes_and_input_order(gpu):
    P, Nr, rho2 = R.sphere()
    a = hip.ball_pivot(P, Nr, rho2)
    b = hip.ball_pivot(P, Nr, rho2)
    assert a.triangles.tobytes() == b.triangles.tobytes() and a.levels.tobytes() == b.levels.tobytes()
    perm = np.random.default_rng(1).permutation(len(P))          # new index i holds old point perm[i]
    c = hip.ball_pivot(P[perm], Nr[perm], rho2)
    back = perm[c.triangles]                                     # in the old numbering
    rot = np.argmin(back, axis=1)
    back = np.stack([back[np.arange(len(back)), (rot + k) % 3] for k in range(3)], axis=1)
    assert sorted(map(tuple, back.tolist())) == list(map(tuple, a.triangles.tolist()))


def test_empty_first_levels_after_a_multi_radius_call(gpu):
    """Levels that emit nothing leave no half-edge table: the levels after them must see no inner vertex,
    whatever an earlier call of the same size left in the scratch memory."""
    P, Nr, rho2 = R.holed_sphere_late()
    dirty = hip.ball_pivot(P, Nr, rho2[2:])                      # marks nearly every vertex inner
    assert (dirty.levels == 1).sum() > 0
    res = hip.ball_pivot(P, Nr, rho2)
    ref = R.delaunay(P, Nr, rho2)
    assert_same(res, ref)
    assert np.bincount(res.levels, minlength=4)[:2].tolist() == [0, 0] and (res.levels == 3).sum() > 0
    assert np.array_equal(res.triangles, dirty.triangles) and np.array_equal(res.levels, dirty.levels + 2)
    again = hip.ball_pivot(P, Nr, rho2)
    assert again.triangles.tobytes() == res.triangles.tobytes() and again.levels.tobytes() == res.levels.tobytes()
    # every counter but the integer fallbacks is the same on every run
    same = [k for k in res.stats if k != "exact_fallbacks"]
    assert [res.stats[k] for k in same] == [again.stats[k] for k in same]


def test_refusals(gpu):
    P, Nr, rho2 = R.sphere()
    with pytest.raises(ValueError, match="quantum 2\\^1 times as large would fit"):
        hip.ball_pivot(P, Nr, [hip.RECON_MAX_RHO2 + 1])
    cloud = float_cloud(P, Nr)
    with pytest.raises(ValueError, match="a quantum of 2.0 would fit"):
        TriangleMesh.create_from_point_cloud_ball_pivoting(cloud, [4096.0], quantum=1.0)
    with pytest.raises(ValueError, match="no normals"):
        TriangleMesh.create_from_point_cloud_ball_pivoting(PointCloud(P.astype(np.float64)), [700.0])
    bad = P.astype(np.float64)
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        TriangleMesh.create_from_point_cloud_ball_pivoting(PointCloud(bad, normals=cloud.normals), [700.0])
    nan_normals = cloud.normals.copy()
    nan_normals[0, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        hip.snap_normals(nan_normals)
    # a cap below the estimate: refused before the triangle pass, nothing of it has run
    with pytest.raises(ValueError, match="exceed max_tests") as e:
        hip.ball_pivot(P, Nr, rho2, max_tests=1000)
    assert isinstance(e.value, hip.BallPivotRefused) and isinstance(e.value, _lib.PyQSMHipError) and e.value.code == -4
    assert e.value.stats["estimated_tests"] > 1000
    assert e.value.stats["tests"] == 0 and e.value.stats["candidates"] == 0 and e.value.stats["blocks"] == 0
    # several radii, the cap between the estimates of the first and the last: no level's triangle pass has run
    H, Hn, h2 = R.holed_sphere()
    small = hip.ball_pivot(H, Hn, h2[:1]).stats["estimated_tests"]
    with pytest.raises(ValueError, match="exceed max_tests") as e:
        hip.ball_pivot(H, Hn, h2, max_tests=small)
    assert e.value.stats["estimated_tests"] > small
    assert e.value.stats["tests"] == 0 and e.value.stats["candidates"] == 0 and e.value.stats["blocks"] == 0


def test_tiny_clouds_and_unresolved_ties(gpu):
    for n in (0, 1, 2):
        res = hip.ball_pivot(np.arange(3 * n, dtype=np.int32).reshape(n, 3) * 10, np.zeros((n, 3), np.int16) + 5, [400])
        assert res.triangles.shape == (0, 3) and res.levels.shape == (0,) and res.stats["blocks"] == 0
    tri = np.array([[0, 0, 0], [30, 0, 0], [0, 30, 0]], np.int32)
    up = np.tile(np.array([0, 0, 1 << 14], np.int16), (3, 1))
    assert hip.ball_pivot(tri, up, [30 * 30]).triangles.tolist() == [[0, 1, 2]]
    assert hip.ball_pivot(tri, -up, [30 * 30]).triangles.tolist() == [[0, 2, 1]]
    assert len(hip.ball_pivot(tri, up, [21 * 21]).triangles) == 0          # circumradius 21.2
    P, Nr, rho2 = R.cospherical_five()
    res = hip.ball_pivot(P, Nr, rho2)
    ref = R.brute(P, Nr, rho2)
    assert ref[2] > 0
    assert_same(res, ref)


@pytest.mark.parametrize("count", [683, 2049])
def test_lone_triangles(gpu, count):
    """`count` right triangles of legs 30, more than 2 rho + 30 apart, normals up or down, points shuffled.
    683 triangles are 2049 half-edges, 2049 triangles 2049 rows: one radix tile of 2048 and one row in the
    sort passes by (u, v) and by (a, b, c), over ids of two 8-bit digits. One row is the single triangle of
    test_tiny_clouds, ids of one digit test_plane_grid_tie_rule, long lists test_nested_surfaces.
    The reference is the brute-force statement on each triangle by itself: a ball of radius rho on three
    points neither holds nor touches a point farther than 2 rho from them."""
    rng = np.random.default_rng(count)
    k = np.arange(count)
    at = np.stack([k % 46, k // 46, np.zeros(count, np.int64)], axis=1) * 100
    P = (at[:, None, :] + np.array([[0, 0, 0], [30, 0, 0], [0, 30, 0]])).reshape(-1, 3).astype(np.int32)
    up = rng.integers(0, 2, count) * 2 - 1
    Nr = (np.repeat(up, 3)[:, None] * np.array([0, 0, 1 << 14])).astype(np.int16)
    perm = rng.permutation(3 * count)                            # new index i holds old point perm[i]
    new_of = np.argsort(perm)
    rows = []
    for t in range(count):
        T, lv, unresolved = R.brute(P[3 * t:3 * t + 3], Nr[3 * t:3 * t + 3], (900,))
        assert len(T) == 1 and unresolved == 0
        a, b, c = new_of[3 * t + T[0]].tolist()
        rows.append(min((a, b, c), (b, c, a), (c, a, b)))        # the same cycle, lowest index first
    res = hip.ball_pivot(P[perm], Nr[perm], (900,))
    assert_same(res, (np.array(sorted(rows), np.int32), np.zeros(count, np.int32), 0))


def test_wrappers_return_a_closed_mesh(gpu):
    P, Nr, rho2 = R.sphere()
    cloud = float_cloud(P, Nr)
    rho = 0.35 * R.R_SPHERE
    direct = hip.ball_pivot(P, Nr, rho2).triangles
    at_one = TriangleMesh.create_from_point_cloud_ball_pivoting(cloud, [rho], quantum=1.0)
    assert at_one.quantum == 1.0 and np.array_equal(at_one.triangles, direct)
    mesh = pcp.get_ball_mesh(cloud, radii=[rho])
    # the default quantum: the finest power of two at which rho (716.8) is at most 2^11 units
    assert isinstance(mesh, TriangleMesh) and mesh.quantum == 0.5
    assert np.array_equal(mesh.triangles, hip.ball_pivot(2 * P, Nr, [int(np.floor((rho / 0.5) ** 2))]).triangles)
    nn = cloud.compute_nearest_neighbor_distance()
    assert nn.shape == (len(P),) and (nn > 0).all()
    d2 = ((P[:, None, :].astype(np.int64) - P[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, d2.max())
    assert np.array_equal(nn, np.sqrt(d2.min(axis=1).astype(np.float64)))
    # the whole chain (distances, normals, orientation, eleven radii) on evenly spread points, where
    # twice the mean nearest-neighbour distance spans every triangle
    F = R.fibonacci_sphere()
    mesh2 = surf_recon.pivot_ball_mesh(PointCloud(F))
    assert mesh2.triangle_levels.max() > 0 and len(F) == len(P)
    for m in (mesh, mesh2):
        assert isinstance(m, TriangleMesh) and len(m.triangles) == 2 * len(P) - 4
        props = mp.check_properties(m)
        assert props["watertight"] and props["edge_manifold"] and props["vertex_manifold"] and props["orientable"]
    vn = mesh2.vertex_normals
    assert vn.shape == (len(F), 3) and ((vn * (F - R.R_SPHERE)).sum(axis=1) > 0).all()   # outward


# ---- tie-dense lattices (tests/recon_cases.py; tests/test_recon_host.py proves what each input is for).
# Random clouds never come within 1e-6 of a tie, against the 2^-46 band of the fp64 filter: these clouds
# sit on it, up to the largest admitted radius. The reference is R.brute, and only that.

def lowest_first(T, lv):
    """Rows (a, b, c, level), each cycle turned so that its lowest index comes first, sorted."""
    T = np.asarray(T)
    rot = np.argmin(T, axis=1)
    T = np.stack([T[np.arange(len(T)), (rot + k) % 3] for k in range(3)], axis=1)
    return sorted(map(tuple, np.concatenate([T, np.asarray(lv)[:, None]], axis=1).tolist()))


@pytest.mark.parametrize("key", C.tie_lattice_keys(),
                         ids=lambda k: "seed%d-m%d-pitch%d-%s" % (k[0], k[1], k[2], "flat" if k[4] else "box"))
def test_tie_lattices(gpu, key):
    """Coincident points, half a cloud in one plane, normals exactly perpendicular to triangle normals,
    cocircular and cospherical ties at every pitch up to the bound (pitch 1182: rho^2 = 3 * 1182^2).
    The tie rule depends on the numbering of the points by design (the fan from the smallest index; a
    tie of a lower index than a drops the triple), so a permuted copy gives the renumbered triangles only
    where nothing ties. Coincident points tie in the plane of each other's triangles, so every case of this
    table has ties: the permuted copy is held against brute of the permuted copy, and against the
    renumbered triangles should a case ever be free of ties."""
    P, Nr, rho2 = C.tie_lattice(*key)
    ref = C.reference("tie_lattice", *key)
    res = hip.ball_pivot(P, Nr, rho2)
    assert_same(res, ref)
    pitch = key[2]
    if pitch >= 500:
        assert res.stats["exact_fallbacks"] > 0
    shift = np.array([-(1 << 30), (1 << 30) - 99991, 12345], np.int32)
    assert_same(hip.ball_pivot(P + shift, Nr, rho2), ref)
    perm = np.random.default_rng(key[0]).permutation(len(P))     # new index i holds old point perm[i]
    moved = hip.ball_pivot(P[perm], Nr[perm], rho2)
    assert_same(moved, R.brute(P[perm], Nr[perm], rho2))
    if ref[2] == 0 and C.census("tie_lattice", *key) == (0, 0):
        assert lowest_first(perm[moved.triangles], moved.levels) == lowest_first(ref[0], ref[1])


@pytest.mark.parametrize("inward", [True, False], ids=["inward", "outward"])
@pytest.mark.parametrize("r2", sorted(C.SPHERE_POINTS))
def test_cospherical_at_the_bound(gpu, r2, inward):
    """18 integer points of a sphere with rho^2 = r^2 just below 2^22: N and sqrt(H) D are about 2^72 and
    equal. With inward normals every candidate rests on the sphere itself and every other point ties."""
    P, Nr, rho2 = C.lattice_sphere(r2, 18, inward)
    res = hip.ball_pivot(P, Nr, rho2)
    assert_same(res, C.reference("lattice_sphere", r2, 18, inward))
    if inward:
        assert res.n_unresolved_ties == len(res.triangles) > 0
        assert res.stats["exact_fallbacks"] >= res.stats["candidates"] > 0


@pytest.mark.parametrize("sign", [1, -1], ids=["up", "down"])
@pytest.mark.parametrize("height", [50, 49])
def test_ball_centre_in_the_plane(gpu, height, sign):
    """H == 0: sqrt(H) = 0, both orientations share one ball; the fifth point ties off the plane or is inside."""
    P, Nr, rho2 = C.rectangle_h0(height)
    res = hip.ball_pivot(P, sign * Nr, rho2)
    assert_same(res, R.brute(P, sign * Nr, rho2))
    assert (res.n_unresolved_ties > 0) == (height == 50)


@pytest.fixture(scope="module")
def dense_box_reference():
    return C.reference("dense_box")


def test_dense_box_of_ties(gpu, dense_box_reference):
    P, Nr, rho2 = C.dense_box()
    res = hip.ball_pivot(P, Nr, rho2)
    assert_same(res, dense_box_reference)
    assert res.stats["max_stencil"] > hip.RECON_CHUNK            # the LDS chunk is refilled, on a cloud full of ties
    assert res.stats["max_cell_points"] > hip.RECON_SLICE
    assert res.stats["exact_fallbacks"] > 0
    again = hip.ball_pivot(P, Nr, rho2)
    assert again.triangles.tobytes() == res.triangles.tobytes() and again.levels.tobytes() == res.levels.tobytes()
    assert again.n_unresolved_ties == res.n_unresolved_ties


@pytest.mark.parametrize("low", C.FAR_LOWS, ids=["centred", "from_int32_min"])
def test_int32_extremes(gpu, low):
    """Two tie lattices 2^31 - 1 units apart along x, the largest admitted span, from -2^30 and from
    INT32_MIN: local coordinates are ijk - min, and the grid's cell count is capped."""
    P, Nr, rho2 = C.far_apart(low)
    res = hip.ball_pivot(P, Nr, rho2)
    assert_same(res, C.reference("far_apart", low))
    assert_same(res, C.far_apart_from_halves())                  # the halves by themselves, renumbered


def test_triangle_cap_is_a_refusal(gpu):
    """30 cospherical points expose about 4 060 triples against a cap of 8 n + 1024 = 1 264 rows: refused
    after the pass (the kernel counts every triangle and writes only the rows below the cap), and the
    next call finds the scratch in order."""
    P, Nr, rho2 = C.lattice_sphere(C.R2_CUBE, 30, True)
    with pytest.raises(hip.BallPivotRefused, match=r"more than 8 n \+ 1024 = 1264") as e:
        hip.ball_pivot(P, Nr, rho2)
    assert e.value.code == -4 and isinstance(e.value, ValueError)
    S, Sn, s2 = R.sphere()
    assert_same(hip.ball_pivot(S, Sn, s2), R.brute(S, Sn, s2))
