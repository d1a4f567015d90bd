"""GPU hole filling (csrc/holes.hip) against the NumPy restatement of its contract, bit for
bit: loops, flags, areas, rows, the loop of every row, statistics. Shapes: closed surfaces with pieces
cut out (the fill closes them again), tubes whose rims sit on the bounds of the two patch kernels,
exact and near ties, thousands of short holes, a rim of thousands of edges, pinch vertices, open
chains, degenerate inputs, determinism, and reconstruct -> meshfix -> check end to end."""
import functools

import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry import mesh_processing as mp
from pyqsm_amd.geometry import surf_recon
from pyqsm_amd.geometry.cloud import PointCloud, TriangleMesh
from tests import holes_restatement as R
from tests import recon_restatement as RR

pytestmark = pytest.mark.gpu

W = hip.FILL_WAVE_MAX


def same(got, want):
    """Every output of hip.mesh_fill_holes equals the restatement's, bit for bit."""
    assert [got.stats[k] for k in hip._FILL_STATS] == want.stats.tolist()
    assert got.ptr.dtype == np.int32 and np.array_equal(got.ptr, want.ptr)
    assert got.verts.dtype == np.int32 and np.array_equal(got.verts, want.verts)
    assert got.flags.dtype == np.uint8 and np.array_equal(got.flags, want.flags)
    assert got.area.dtype == np.float64 and got.area.tobytes() == want.area.tobytes()
    assert got.new_tris.dtype == np.int32 and np.array_equal(got.new_tris, want.new_tris)
    assert got.new_loop.dtype == np.int32 and np.array_equal(got.new_loop, want.new_loop)


def check(tris, verts, max_edges=None):
    got = hip.mesh_fill_holes(tris, verts, max_edges)
    want = R.fill(tris, verts, max_edges)
    same(got, want)
    loops = hip.mesh_boundary_loops(tris, len(verts))
    assert np.array_equal(loops.ptr, want.ptr) and np.array_equal(loops.verts, want.verts)
    assert [loops.stats[k] for k in hip._FILL_STATS] == [want.stats[0], want.stats[1], 0, 0, 0, want.stats[5], 0, 0]
    return got


def band(inner):
    """A band of triangles between the polygon `inner` and the same polygon scaled by two about its mean."""
    inner = np.asarray(inner, np.float64)
    c = inner.mean(axis=0)
    L = len(inner)
    return R.grid_surface(L, 1, True, False, lambda i, j: inner[i] if j == 0 else c + 2.0 * (inner[i] - c))


@functools.lru_cache(maxsize=None)
def closed(shape):
    return R.icosphere(2) if shape == "icosphere" else R.torus()


def cuts(tris):
    """Triangle sets to remove: one triangle, two adjacent ones, a vertex fan, a patch of two rings, and
    several of them at once, far from one another."""
    def fan(v):
        return np.nonzero((tris == v).any(axis=1))[0]

    def grown(seed):
        return np.nonzero(np.isin(tris, np.unique(tris[seed])).any(axis=1))[0]
    t0 = 0
    nb = [t for t in range(1, len(tris)) if len(set(tris[t0]) & set(tris[t])) == 2][0]
    out = {"one": np.array([t0]), "two": np.array([t0, nb]), "fan": fan(int(tris[t0, 0])),
           "patch": grown(fan(int(tris[t0, 0])))}
    taken, several = np.unique(tris[grown(out["patch"])]), [out["patch"]]
    for t in range(len(tris)):
        if len(several) < 4 and not np.isin(tris[t], taken).any():
            piece = fan(int(tris[t, 0])) if len(several) % 2 else np.array([t])
            if not np.isin(tris[piece], taken).any():
                several.append(piece)
                taken = np.union1d(taken, np.unique(tris[grown(piece)]))
    out["several"] = np.concatenate(several)
    return out


@pytest.mark.parametrize("shape", ["icosphere", "torus"])
@pytest.mark.parametrize("cut", ["one", "two", "fan", "patch", "several"])
def test_fill_closes_a_closed_surface_again(gpu, shape, cut):
    verts, tris = closed(shape)
    open_tris = np.delete(tris, cuts(tris)[cut], axis=0)
    got = check(open_tris, verts)
    assert got.stats["loops"] >= (4 if cut == "several" else 1) and got.stats["loops_filled"] == got.stats["loops"]
    if cut == "one":
        assert np.diff(got.ptr).tolist() == [3]
    if cut == "two":
        assert np.diff(got.ptr).tolist() == [4]
    mesh = TriangleMesh(verts, open_tris)
    filled = mesh.fill_holes()
    assert np.array_equal(filled.triangles[:len(open_tris)], open_tris)
    assert np.array_equal(filled.triangles[len(open_tris):], got.new_tris) and filled.last_fill.stats == got.stats
    assert [len(x) for x in mesh.get_boundary_loops()] == np.diff(got.ptr).tolist()
    s = hip.mesh_topology(filled.triangles, len(verts)).summary
    assert s["boundary_edges"] == 0 and s["orientable"] == 1 and s["over_two_edges"] == 0
    assert s["same_direction_edges"] == 0


@pytest.mark.parametrize("L", [3, 4, W, W + 1, 64, 65, hip.FILL_MAX_LOOP, hip.FILL_MAX_LOOP + 1])
def test_tube_rims_on_the_bounds_of_the_kernel_classes(gpu, L):
    verts, tris = R.tube(L)
    got = check(tris, verts)
    assert np.diff(got.ptr).tolist() == [L, L]
    if L > hip.FILL_MAX_LOOP:
        assert got.flags.tolist() == [hip.LOOP_TOO_LONG] * 2 and len(got.new_tris) == 0 and (got.area == 0).all()
        assert got.stats["loops_too_long"] == 2
    else:
        assert got.flags.tolist() == [0, 0] and len(got.new_tris) == 2 * (L - 2) and (got.area > 0).all()
        s = hip.mesh_topology(np.concatenate([tris, got.new_tris]), len(verts)).summary
        assert s["boundary_edges"] == 0 and s["orientable"] == 1 and s["over_two_edges"] == 0


@pytest.mark.parametrize("roll", [0, 1])
def test_exact_ties_go_to_the_lowest_apex(gpu, roll):
    """The 8-gon of a square hole (corners and edge midpoints, multiples of 0.25): every triangulation has
    the same total exactly. Starting at a midpoint (roll = 1) the fan has two flat rows per loop."""
    octagon = np.array([[0, 0, 0], [.75, 0, 0], [1.5, 0, 0], [1.5, .75, 0], [1.5, 1.5, 0], [.75, 1.5, 0], [0, 1.5, 0],
                        [0, .75, 0]], np.float64)
    verts, tris = band(np.roll(octagon, roll, axis=0))
    got = check(tris, verts)
    assert np.diff(got.ptr).tolist() == [8, 8] and got.area.tolist() == [2.25, 9.0]
    for l in range(2):
        ring = got.loop(l)
        assert got.new_tris[6 * l:6 * l + 6].tolist() == [[ring[m], ring[m + 1], ring[7]] for m in range(6)]
    assert got.stats["zero_area_rows"] == 4 * roll


def test_near_ties_of_a_regular_polygon(gpu):
    a = 2 * np.pi * np.arange(32) / 32
    verts, tris = band(np.stack([np.cos(a), np.sin(a), 0 * a], axis=1))
    got = check(tris, verts)
    assert np.diff(got.ptr).tolist() == [32, 32] and got.flags.tolist() == [0, 0]


def test_many_short_loops(gpu):
    verts, tris = R.sheet_with_holes(170)
    got = check(tris, verts)
    lengths = np.diff(got.ptr)
    assert got.stats["loops"] > 3000 and got.stats["loops_filled"] == got.stats["loops"] - 1
    assert len(np.unique(lengths)) >= 5 and lengths.max() == 4 * 170 and np.sort(lengths)[-2] <= W
    assert (np.diff(got.verts[got.ptr[:-1]]) > 0).all()          # ascending by v_0


def test_every_length_of_both_classes_in_one_call(gpu):
    """Tubes of 3 .. 40 edges in one mesh: the waves of a block hold loops of different lengths, and both
    patch kernels run in the same call."""
    parts, tris, n = [], [], 0
    for L in range(3, 41):
        v, t = R.tube(L, seed=L)
        parts.append(v + (3.0 * L, 0, 0))
        tris.append(t + n)
        n += len(v)
    got = check(np.concatenate(tris), np.concatenate(parts))
    assert sorted(np.diff(got.ptr).tolist()) == sorted(2 * list(range(3, 41))) and (got.flags == 0).all()
    assert len(got.new_tris) == 2 * sum(L - 2 for L in range(3, 41))


def test_a_rim_of_thousands_of_edges(gpu):
    verts, tris = R.tube(5000, rings=1)
    got = check(tris, verts)
    assert np.diff(got.ptr).tolist() == [5000, 5000] and got.flags.tolist() == [hip.LOOP_TOO_LONG] * 2
    assert got.stats["open_chain_half_edges"] == 0 and len(got.new_tris) == 0


def test_pinch_vertices(gpu):
    # two tubes whose rims share one vertex index: the rotation stays inside a fan, so the rims stay two
    # loops, each with the vertex once, both filled
    va, ta = R.tube(10, seed=1)
    vb, tb = R.tube(7, seed=2)
    tb = tb + len(va)
    tb[tb == len(va)] = 0                                         # rim vertex 0 of the second is the first's
    got = check(np.concatenate([ta, tb]), np.concatenate([va, vb + 5.0]))
    assert sorted(np.diff(got.ptr).tolist()) == [7, 7, 10, 10] and got.flags.tolist() == [0, 0, 0, 0]
    assert got.verts[got.ptr[0]] == 0 and got.verts[got.ptr[1]] == 0 and (got.verts == 0).sum() == 2
    # two holes of a sheet that touch diagonally: one loop that visits the vertex twice, flag 1, untouched
    verts, tris = R.grid_surface(6, 6, False, False, lambda i, j: (i, j, 0.1 * i * j))
    cut = np.delete(tris, [2 * 14, 2 * 14 + 1, 2 * 21, 2 * 21 + 1], axis=0)
    got = check(cut, verts)
    assert sorted(np.diff(got.ptr).tolist()) == [8, 24] and sorted(got.flags.tolist()) == [0, hip.LOOP_REPEATED_VERTEX]
    assert got.stats["loops_repeated_vertex"] == 1 and len(got.new_tris) == 22


def test_open_chains_are_counted_and_the_rest_is_filled(gpu):
    verts, tris = R.tube(12, rings=3)
    tris = tris.copy()
    tris[0] = tris[0, [0, 2, 1]]                                  # a rim triangle turned over: same-direction pairs
    mid = tris[2 * (3 * 5 + 1)]                                   # a triangle of the middle ring
    fin = [[mid[0], mid[1], len(verts)]]                          # a third triangle on one of its edges
    verts = np.concatenate([verts, [[0.0, 0.0, 1.5]]])
    tris = np.concatenate([tris, fin])
    top = hip.mesh_topology(tris, len(verts)).summary
    assert top["over_two_edges"] == 1 and top["same_direction_edges"] == 2
    got = check(tris, verts)
    assert got.stats["open_chain_half_edges"] >= 3 and got.stats["loops_filled"] >= 1
    assert got.stats["boundary_half_edges"] == got.ptr[-1] + got.stats["open_chain_half_edges"]


def test_degenerate_inputs(gpu):
    got = check(np.array([[0, 1, 2]]), np.eye(3))
    assert got.verts.tolist() == [0, 2, 1] and got.new_tris.tolist() == [[0, 2, 1]]
    # a folded quad whose cheaper diagonal is the edge its two triangles already share
    got = check(np.array([[0, 1, 2], [0, 2, 3]]), np.array([[0, 0, 0], [1, 0, 1], [1, 1, 0], [0, 1, 0]], np.float64))
    assert got.stats["existing_diagonals"] == 1 and len(got.new_tris) == 2
    empty = hip.mesh_fill_holes(np.zeros((0, 3), np.int32), np.zeros((0, 3)))
    assert empty.ptr.tolist() == [0] and len(empty.new_tris) == 0
    verts, tris = closed("icosphere")
    got = check(tris, verts)
    assert got.ptr.tolist() == [0] and len(got.new_tris) == 0 and set(got.stats.values()) == {0}
    verts, tris = R.sheet_with_holes(20, seed=3)
    got = check(tris, verts, max_edges=5)
    lengths = np.diff(got.ptr)
    assert (lengths <= 5).any() and (lengths > 5).any() and np.array_equal(got.flags == 0, lengths <= 5)
    assert np.array_equal(got.flags[lengths > 5], np.full((lengths > 5).sum(), hip.LOOP_TOO_LONG))
    filled, n = mp.fill_small_boundaries(TriangleMesh(verts, tris), nbe=5)
    assert n == got.stats["loops_filled"] and len(filled.triangles) == len(tris) + len(got.new_tris)
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.mesh_fill_holes(tris, verts, max_edges=hip.FILL_MAX_LOOP + 1)
    assert e.value.code == -1


def test_same_bytes_on_every_run_and_under_a_permutation(gpu):
    verts, tris = R.sheet_with_holes(30, seed=8)
    a, b = hip.mesh_fill_holes(tris, verts), hip.mesh_fill_holes(tris, verts)
    for x, y in zip(a[:6], b[:6]):
        assert x.tobytes() == y.tobytes()
    assert a.stats == b.stats
    perm = np.random.default_rng(4).permutation(len(tris))
    c = hip.mesh_fill_holes(tris[perm], verts)
    # no vertex lies on two loops here, so every v_0 is unique: the same loops, order and patches
    assert len(np.unique(a.verts)) == len(a.verts)
    for x, y in zip(a[:6], c[:6]):
        assert x.tobytes() == y.tobytes()
    assert a.stats == c.stats


def test_reconstruct_then_meshfix_then_check(gpu):
    F = RR.fibonacci_sphere()
    F = F[F[:, 2] < RR.R_SPHERE * 1.75]                           # without the cap around +z
    mesh = surf_recon.pivot_ball_mesh(PointCloud(F))
    before = mp.check_properties(mesh)
    assert len(before["boundary_edges"]) > 0 and not before["watertight"]
    for algo in ("pyt", "repair"):
        fixed = surf_recon.meshfix(mesh, algo=algo)
        st = fixed.last_fill.stats
        after = mp.check_properties(fixed)
        assert len(after["boundary_edges"]) < len(before["boundary_edges"])
        assert np.array_equal(fixed.vertex_normals, mesh.vertex_normals)
        if st["loops_filled"] == st["loops"] and st["open_chain_half_edges"] == 0:
            assert len(after["boundary_edges"]) == 0 and after["edge_manifold_boundary"]
        print(algo, st, len(before["boundary_edges"]), len(after["boundary_edges"]))
        assert st["loops"] >= 1
