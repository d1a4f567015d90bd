"""The hole-filling contract on the CPU (tests/holes_restatement.py): the table's total equals a
brute force over all triangulations, exact ties go to the lowest apex, the restatement's loops close the
meshes they were cut from, csrc/holes_exact.hpp gives the restatement's bits as a host program under the
sanitizers, and the host side of the wrappers (constants, refusals, empty input) holds without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from pyqsm_amd import _lib, _shadow, hip
from pyqsm_amd.geometry import mesh_processing as mp
from pyqsm_amd.geometry import surf_recon
from pyqsm_amd.geometry.cloud import TriangleMesh
from tests import holes_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CATALAN = {3: 1, 4: 2, 5: 5, 6: 14, 7: 42, 8: 132, 9: 429}


def saddle_loop(L, seed=0):
    rng = np.random.default_rng(100 * L + seed)
    a = 2 * np.pi * np.arange(L) / L
    return np.stack([np.cos(a), np.sin(a), 0.5 * np.cos(2 * a)], axis=1) + 0.05 * rng.standard_normal((L, 3))


def lattice_octagon():
    """The 8-gon around a square hole, corners and edge midpoints, coordinates in multiples of 0.25."""
    return np.array([[0, 0, 0], [.75, 0, 0], [1.5, 0, 0], [1.5, .75, 0], [1.5, 1.5, 0], [.75, 1.5, 0], [0, 1.5, 0],
                     [0, .75, 0]], np.float64)


def edge_counts(tris):
    t = np.asarray(tris, np.int64)
    a, b = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    und = np.unique((np.minimum(a, b) << 32) | np.maximum(a, b), return_counts=True)[1]
    directed = np.unique((a << 32) | b, return_counts=True)[1]
    return und, directed


@pytest.mark.parametrize("L", range(3, 10))
def test_table_total_equals_the_brute_force(L):
    for seed in range(3):
        p = saddle_loop(L, seed)
        W, split = R.min_area_table(p)
        best, count = R.brute_force_min_area(p)
        assert count == CATALAN[L]
        total = W[0, L - 1]
        print(L, seed, total, best, abs(total - best))
        assert abs(total - best) <= 4e-16 * L * total
        rows = R.rows_of(L, split)
        assert len(rows) == L - 2
        assert abs(sum(float(R.area(p[i], p[j], p[k])) for i, j, k in rows) - total) <= 4e-16 * L * total


def test_exact_ties_give_the_lowest_split_fan():
    p = lattice_octagon()
    W, split = R.min_area_table(p)
    assert W[0, 7] == 2.25
    best, count = R.brute_force_min_area(p)
    assert best == 2.25 and count == 132
    assert all(j == i + 1 for (i, k), j in split.items())
    assert R.rows_of(8, split) == [(m, m + 1, 7) for m in range(6)]


def test_single_triangle_and_direction():
    got = R.fill([[0, 1, 2]], np.eye(3))
    assert got.ptr.tolist() == [0, 3] and got.verts.tolist() == [0, 2, 1] and got.flags.tolist() == [0]
    assert got.new_tris.tolist() == [[0, 2, 1]] and got.stats.tolist() == [3, 1, 1, 0, 0, 0, 0, 0]
    assert got.area[0] == R.area(np.eye(3)[0], np.eye(3)[2], np.eye(3)[1])


@pytest.mark.parametrize("shape", ["icosphere", "torus"])
def test_restatement_closes_what_was_cut(shape):
    verts, tris = R.icosphere(1) if shape == "icosphere" else R.torus(12, 8)
    assert (edge_counts(tris)[0] == 2).all()
    fan = np.nonzero((tris == 5).any(axis=1))[0]            # the triangles around vertex 5
    far = np.nonzero(~np.isin(tris, np.unique(tris[fan])).any(axis=1))[0][:1]   # and one triangle away from them
    cut = np.delete(tris, np.concatenate([far, fan]), axis=0)
    got = R.fill(cut, verts)
    assert got.stats[1] >= 1 and got.stats[2] == got.stats[1] and got.stats[5] == 0
    und, directed = edge_counts(np.concatenate([cut, got.new_tris]))
    assert (und == 2).all() and (directed == 1).all()       # closed, and every edge once each way
    assert sorted(len(got.loop(i)) for i in range(len(got.flags))) == sorted(np.diff(got.ptr).tolist())
    for i in range(len(got.flags)):
        assert got.loop(i)[0] == got.loop(i).min()
    assert (np.diff([got.loop(i)[0] for i in range(len(got.flags))]) >= 0).all()


def test_pinch_and_open_chain_in_the_restatement():
    # two triangles that touch at vertex 0 only: the rotation stays inside a fan, so two loops that both
    # start at 0, ordered by the half-edge that leaves it, both filled
    bow = [[0, 1, 2], [0, 3, 4]]
    got = R.fill(bow, np.random.default_rng(1).random((5, 3)))
    assert got.flags.tolist() == [0, 0] and got.verts.tolist() == [0, 2, 1, 0, 4, 3]
    assert got.new_tris.tolist() == [[0, 2, 1], [0, 4, 3]] and got.stats.tolist()[:6] == [6, 2, 2, 0, 0, 0]
    # two holes of a sheet that touch diagonally at a vertex: the fans between them lead from one rim to
    # the other, one loop that visits the vertex twice, flag 1, left open; the outer rim is filled
    verts, tris = R.grid_surface(4, 4, False, False, lambda i, j: (i, j, 0.1 * i * j))
    cut = np.delete(tris, [2 * 5, 2 * 5 + 1, 2 * 10, 2 * 10 + 1], axis=0)
    got = R.fill(cut, verts)
    assert sorted(np.diff(got.ptr).tolist()) == [8, 16] and sorted(got.flags.tolist()) == [0, 1]
    pinched = got.loop(int(np.nonzero(got.flags)[0][0])).tolist()
    assert pinched.count(12) == 2 and len(set(pinched)) == 7 and len(got.new_tris) == 14
    # three triangles on edge (0, 1): the walks into it stop, every boundary half-edge lies on an open chain
    book = [[0, 1, 2], [0, 1, 3], [0, 1, 4]]
    got = R.fill(book, np.random.default_rng(2).random((5, 3)))
    assert got.stats.tolist()[:6] == [6, 0, 0, 0, 0, 6]


def test_holes_check_equals_the_restatement(tmp_path):
    """holes_exact.hpp as a stand-alone host program under ASan and UBSan (csrc/Makefile: holes_check): host
    code only, built and run on the CPU. Totals, split tables and rows are the restatement's, bit for bit."""
    if _lib.device_count() > 0:
        pytest.skip("sanitizer runs belong on machines without a GPU")
    loops = [saddle_loop(L, s) for L in (3, 4, 5, 9, 17, 32, 33, 64) for s in range(2)] + [lattice_octagon()]
    a = 2 * np.pi * np.arange(32) / 32
    loops.append(np.stack([np.cos(a), np.sin(a), 0 * a], axis=1))              # near-ties that rounding decides
    path = tmp_path / "loops.txt"
    with open(path, "w") as f:
        for p in loops:
            f.write(f"{len(p)}\n")
            for row in p:
                f.write(" ".join(float(x).hex() for x in row) + "\n")
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "pyqsm_amd", "csrc"), "holes_check", f"LOOPS={path}"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"holes_check: ok {len(loops)} loops" in out.stdout
    lines = re.findall(r"^loop (\d+) ([0-9a-f]{16}) ([0-9a-f]+)((?: \d+\.\d+\.\d+)+)$", out.stdout, flags=re.M)
    assert len(lines) == len(loops)
    for p, (L, bits, table, rows) in zip(loops, lines):
        L = int(L)
        W, split = R.min_area_table(p)
        assert L == len(p) and bits == "%016x" % np.float64(W[0, L - 1]).view(np.uint64)
        want = "".join("%02x" % (split[(i, i + d)] if d > 1 else 0) for d in range(1, L) for i in range(L - d))
        assert table == want
        assert [tuple(int(x) for x in r.split(".")) for r in rows.split()] == R.rows_of(L, split)


def test_constants_and_registration():
    text = open(os.path.join(ROOT, "include", "pyqsm_hip.h")).read()
    for macro, value in (("PYQSM_FILL_MAX_LOOP", hip.FILL_MAX_LOOP), ("PYQSM_FILL_WAVE_MAX", hip.FILL_WAVE_MAX)):
        assert re.search(rf"#define {macro} {value}\b", text), macro
    assert hip.FILL_MAX_LOOP == R.FILL_MAX_LOOP == 128 and 3 <= hip.FILL_WAVE_MAX < hip.FILL_MAX_LOOP
    assert "meshfix" in _shadow.HOT_FUNCTIONS["geometry.surf_recon"] and callable(surf_recon.meshfix)
    assert callable(mp.fill_small_boundaries)
    src = open(os.path.join(ROOT, "pyqsm_amd", "geometry", "surf_recon.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(pymeshfix|pyvista|open3d)\b", src, flags=re.M)
    with pytest.raises(ValueError):
        surf_recon.meshfix(TriangleMesh(np.zeros((3, 3)), [[0, 1, 2]]), algo="fast")


def test_no_triangles_touch_no_device():
    """n_tris == 0 is answered on the host, also without a GPU."""
    loops = hip.mesh_boundary_loops(np.zeros((0, 3), np.int32), 4)
    assert loops.ptr.tolist() == [0] and loops.verts.shape == (0,) and set(loops.stats.values()) == {0}
    got = hip.mesh_fill_holes(np.zeros((0, 3), np.int32), np.zeros((4, 3)))
    assert got.ptr.tolist() == [0] and got.new_tris.shape == (0, 3) and got.flags.shape == (0,)
    assert got.area.shape == (0,) and got.new_loop.shape == (0,) and set(got.stats.values()) == {0}
    mesh = TriangleMesh(np.zeros((4, 3)), np.zeros((0, 3), np.int64))
    assert mesh.get_boundary_loops() == [] and len(mesh.fill_holes().triangles) == 0
    filled, n = mp.fill_small_boundaries(mesh)
    assert n == 0 and len(filled.triangles) == 0


def test_refusals_come_before_any_device():
    tri, verts = np.array([[0, 1, 2]], np.int32), np.eye(3)
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.mesh_fill_holes(tri, verts, max_edges=129)
    assert e.value.code == -1
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.mesh_fill_holes(np.array([[0, 1, 3]], np.int32), verts)
    assert e.value.code == -1
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.mesh_boundary_loops(np.array([[0, 1, 1]], np.int32), 3)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        hip.mesh_fill_holes(tri, np.zeros((3, 2)))
