"""pyqsm_mesh_topology and pyqsm_mesh_self_intersections on the GPU against the CPU statement of
their contract (tests/mesh_restatement.py, itself pinned to SciPy and to exact rationals by
tests/test_mesh_host.py). Everything is compared as integers; the cluster areas follow the two
contracts of the header: per-triangle bits, and |sum - fsum| <= (n + 4) 2^-52 fsum."""
import math

import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry import mesh_processing as mp
from pyqsm_amd.geometry.cloud import TriangleMesh
from tests import mesh_restatement as R

pytestmark = pytest.mark.gpu

ROWS = hip.MESH_TILE_ROWS
CAP = 10 ** 8                          # max_tests for the sweeps below: far above their T (T - 1) / 2
M = R.MAX_EXTENT


# ---------------------------------------------------------------- topology

def assert_topology(top, ref, with_area):
    assert np.array_equal(top.edges, ref["edges"])
    assert np.array_equal(top.edge_count, ref["edge_count"])
    assert np.array_equal(top.edge_flags, ref["edge_flags"])
    assert np.array_equal(top.tri_cluster, ref["tri_cluster"])
    assert np.array_equal(top.cluster_n, ref["cluster_n"])
    assert np.array_equal(top.vertex_flags, ref["vertex_flags"])
    assert list(top.summary.values()) == ref["summary"].tolist()
    assert top.edges.dtype == np.int32 and top.edge_flags.dtype == np.uint8 and top.cluster_n.dtype == np.int64
    if not with_area:
        assert top.cluster_area is None
        return
    exact, n = ref["cluster_area"], ref["cluster_n"]
    err = np.abs(top.cluster_area - exact)
    print("cluster area: max |sum - fsum| / fsum =", float((err / exact).max()) if len(exact) else 0.0)
    assert (err <= (n + 4) * 2.0 ** -52 * exact).all()
    single = np.nonzero(n == 1)[0]                   # one triangle: the sum is that triangle's area, bit for bit
    for c in single:
        t = int(np.nonzero(ref["tri_cluster"] == c)[0][0])
        assert top.cluster_area[c] == ref["tri_area"][t]


@pytest.mark.parametrize("name", sorted(R.NAMED))
def test_named_meshes(gpu, name):
    verts, tris = R.NAMED[name]()
    ref = R.topology(tris, len(verts), verts)
    assert_topology(hip.mesh_topology(tris, len(verts), verts), ref, True)
    assert_topology(hip.mesh_topology(tris, len(verts)), ref, False)


def test_one_two_and_no_triangles(gpu):
    verts = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [3, 4, 1], [9, 9, 9], [10, 9, 9], [9, 11, 9.5]], float)
    for tris in ([[0, 1, 2]], [[0, 1, 2], [2, 1, 3]], [[0, 1, 2], [4, 5, 6]], [[0, 1, 2], [0, 1, 2]]):
        tris = np.array(tris, np.int32)
        assert_topology(hip.mesh_topology(tris, len(verts), verts), R.topology(tris, len(verts), verts), True)
    none = np.zeros((0, 3), np.int32)
    top = hip.mesh_topology(none, len(verts), verts)
    assert_topology(top, R.topology(none, len(verts), verts), True)
    assert top.summary["isolated_vertices"] == len(verts) and top.summary["orientable"] == 1
    assert len(top.cluster_area) == 0
    assert hip.mesh_topology(none, 0).summary["edges"] == 0


def test_bad_indices_are_refused(gpu):
    for tris in ([[0, 1, 4]], [[0, 1, -1]], [[0, 1, 2], [2, 3, 2]]):
        with pytest.raises(_lib.PyQSMHipError) as e:
            hip.mesh_topology(np.array(tris, np.int32), 4)
        assert e.value.code == -1


# ---------------------------------------------------------------- self-intersection

def assert_intersections(ijk, tris, want_pairs=None):
    ref_pairs, ref_hit, ref_stats = R.self_intersections(ijk, tris)
    got = hip.mesh_self_intersections(ijk, tris, max_tests=CAP)
    assert got.pairs.dtype == np.int32 and np.array_equal(got.pairs, ref_pairs)
    assert got.n_pairs == len(ref_pairs)
    assert np.array_equal(got.tri_hit, ref_hit)
    assert list(got.stats.values()) == ref_stats.tolist()
    count_only = hip.mesh_self_intersections(ijk, tris, return_pairs=False, max_tests=CAP)
    assert count_only.pairs is None and count_only.n_pairs == len(ref_pairs)
    assert np.array_equal(count_only.tri_hit, ref_hit) and count_only.stats == got.stats
    if want_pairs is not None:
        assert got.pairs.tolist() == want_pairs
    return got


def soup(n=1500, seed=21):
    """Random small triangles in a [0, 64)^3 lattice: many hits, touches, shared indices and
    degenerate triangles."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 56, (n, 1, 3))
    ijk = (base + rng.integers(0, 9, (n, 3, 3))).reshape(-1, 3)
    tris = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    tris[1:600:2, 0] = tris[0:600:2, 1]              # 300 pairs of triangles that share an edge by index
    tris[1:600:2, 1] = tris[0:600:2, 0]
    ijk[tris[600:640, 2]] = ijk[tris[600:640, 0]]    # two vertices on one node
    ijk[tris[640:680, 2]] = 2 * ijk[tris[640:680, 1]] - ijk[tris[640:680, 0]]   # three on a line
    return np.clip(ijk, 0, 63).astype(np.int32), tris


def test_random_soup(gpu):
    ijk, tris = soup()
    got = assert_intersections(ijk, tris)
    s = got.stats
    assert s["pairs_reported"] > 1000 and s["shared_index_skipped"] >= 300 and s["degenerate_triangles"] >= 40
    assert s["box_survivors"] > s["exact_tests"] > s["pairs_reported"]


def seam_mesh(n, pair):
    """n small triangles far apart along x; triangle pair[1] is moved to pierce triangle pair[0]."""
    t = np.arange(n)
    zero = np.zeros(n, np.int64)
    tri = np.stack([np.stack([10 * t, zero, zero], 1), np.stack([10 * t + 4, zero, zero], 1),
                    np.stack([10 * t, zero + 4, zero], 1)], axis=1)
    i, j = pair
    tri[j] = [[10 * i + 1, 1, -1], [10 * i + 1, 1, 1], [10 * i + 3, 3, 1]]
    tri[:, :, 2] += 1
    return tri.reshape(-1, 3).astype(np.int32), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


@pytest.mark.parametrize("n", [ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 3])
def test_tile_seams(gpu, n):
    for pair in ((0, n - 1), (ROWS - 1, ROWS), (n - 2, n - 1)):
        if pair[1] >= n:
            continue
        ijk, tris = seam_mesh(n, pair)
        assert_intersections(ijk, tris, [list(pair)])


def pierced_pairs(p, seed=5):
    """p pairs of small triangles far apart along x, the second of a pair piercing the first, the 2 p
    triangles in shuffled order: p intersecting pairs whose (i, j) are spread over [0, 2 p)."""
    x = 20 * np.arange(p)[:, None, None] * np.array([1, 0, 0])
    flat = np.array([[0, 0, 1], [4, 0, 1], [0, 4, 1]]) + x
    spike = np.array([[1, 1, 0], [1, 1, 2], [3, 3, 2]]) + x
    tri = np.concatenate([flat, spike])[np.random.default_rng(seed).permutation(2 * p)]
    return tri.reshape(-1, 3).astype(np.int32), np.arange(6 * p, dtype=np.int32).reshape(2 * p, 3)


@pytest.mark.parametrize("p", [100, 2049])
def test_pair_list_sizes(gpu, p):
    """The pair list's two sort passes by (i, j): 100 pairs of 200 triangles (ids of one 8-bit digit),
    and 2049 pairs (one radix tile of 2048 and one row) of 4098 triangles (two digits). One pair, which
    the sort returns as it is, is test_catalogue and test_tile_seams; two digits also test_random_soup."""
    ijk, tris = pierced_pairs(p)
    got = assert_intersections(ijk, tris)
    assert got.n_pairs == p and got.tri_hit.all()


BASE = [[0, 0, 0], [8, 0, 0], [0, 8, 0]]
CATALOGUE = {
    "vertex_on_face": ([[2, 2, 0], [2, 2, 6], [5, 2, 6]], True),
    "edges_cross_at_a_point": ([[4, -2, -2], [4, 2, 2], [4, -2, 2]], True),
    "coplanar_overlap": ([[2, 2, 0], [12, 2, 0], [2, 12, 0]], True),
    "coplanar_inside": ([[1, 1, 0], [3, 1, 0], [1, 3, 0]], True),
    "coplanar_disjoint": ([[9, 9, 0], [12, 9, 0], [9, 12, 0]], False),
    "collinear_edges_touching": ([[8, 0, 0], [14, 0, 0], [11, -5, 0]], True),
    "collinear_edges_apart_by_one": ([[9, 0, 0], [14, 0, 0], [11, -5, 0]], False),
    "near_miss_above_by_one": ([[2, 2, 1], [2, 2, 6], [5, 2, 6]], False),
    "near_miss_beside_by_one": ([[5, 4, -3], [5, 4, 3], [9, 9, 3]], False),
    "pierced": ([[2, 2, -3], [2, 2, 3], [9, 9, 3]], True),
}


@pytest.mark.parametrize("name", sorted(CATALOGUE))
def test_catalogue(gpu, name):
    other, hit = CATALOGUE[name]
    ijk = np.array(BASE + other, np.int32)
    ijk -= ijk.min(axis=0)
    tris = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    got = assert_intersections(ijk, tris, [[0, 1]] if hit else [])
    assert got.stats["shared_index_skipped"] == 0
    assert_intersections(ijk, tris[::-1].copy(), [[0, 1]] if hit else [])


def test_shared_index_is_skipped_and_counted(gpu):
    ijk = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0], [8, 8, 0], [1, 3, 0]], np.int32)
    tris = np.array([[0, 1, 2], [0, 3, 4]], np.int32)            # coplanar, overlapping, one common index
    got = assert_intersections(ijk, tris, [])
    assert got.stats["shared_index_skipped"] == 1 and got.stats["exact_tests"] == 0
    assert not got.tri_hit.any()


@pytest.mark.parametrize("apex,hit", [((M // 2, M // 2, M), True), ((M // 2 + 1, M // 2, M), False),
                                      ((M // 2 - 8, M // 2 - 8, M), True)])
def test_full_extent(gpu, apex, hit):
    """Two triangles that span 2^20 on every axis: the apex of the second touches an edge of the
    first, misses it by one unit, or reaches through it. A determinant that overflowed would flip
    one of these."""
    ijk = np.array([[0, 0, 0], [M, 0, M], [0, M, M], [0, M, 0], [M, 0, 0], list(apex)], np.int32)
    tris = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    assert_intersections(ijk, tris, [[0, 1]] if hit else [])


def test_refusals(gpu):
    tris = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.mesh_self_intersections(np.array([[0, 0, 0], [M + 1, 0, 0], [0, 1, 0]], np.int32), tris, max_tests=CAP)
    assert e.value.code == -1
    ijk, many = seam_mesh(100, (0, 1))
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.mesh_self_intersections(ijk, many, max_tests=10)
    assert e.value.code == -4
    assert not any(e.value.stats.values())           # nothing ran
    assert hip.mesh_self_intersections(ijk, many, max_tests=100 * 99 // 2).n_pairs == 1
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.mesh_self_intersections(ijk, np.array([[0, 1, 300]], np.int32), max_tests=CAP)
    assert e.value.code == -1
    assert hip.mesh_self_intersections(ijk, np.zeros((0, 3), np.int32), max_tests=CAP).n_pairs == 0


def test_default_cap_follows_the_header(gpu):
    """max_tests <= 0 means PYQSM_MESH_DEFAULT_MAX_TESTS; while that is 0 (no measured rate to derive
    it from) there is no default, and the call is refused before anything runs."""
    ijk, tris = seam_mesh(100, (0, 1))
    if hip.MESH_DEFAULT_MAX_TESTS > 0:
        assert hip.mesh_self_intersections(ijk, tris).n_pairs == 1
        return
    for cap in (None, 0, -5):
        with pytest.raises(_lib.PyQSMHipError) as e:
            hip.mesh_self_intersections(ijk, tris, max_tests=cap)
        assert e.value.code == -1 and not any(e.value.stats.values())


# ---------------------------------------------------------------- reproducibility

def test_two_runs_give_the_same_bytes(gpu):
    verts, tris = R.many_tets()
    a, b = hip.mesh_topology(tris, len(verts), verts), hip.mesh_topology(tris, len(verts), verts)
    for x, y in zip(a[:7], b[:7]):
        assert x.tobytes() == y.tobytes()
    assert a.summary == b.summary
    ijk, tris = soup()
    a, b = hip.mesh_self_intersections(ijk, tris, max_tests=CAP), hip.mesh_self_intersections(ijk, tris, max_tests=CAP)
    assert a.pairs.tobytes() == b.pairs.tobytes() and a.tri_hit.tobytes() == b.tri_hit.tobytes()
    assert a.stats == b.stats and a.n_pairs == b.n_pairs


# ---------------------------------------------------------------- wrappers

def pierced_cube():
    verts, tris = R.cube()
    extra = np.array([[0.25, 0.25, 0.5], [0.75, 0.25, 1.5], [0.25, 0.75, 1.5]])
    return np.concatenate([verts, extra]), np.concatenate([tris, [[8, 9, 10]]]).astype(np.int32)


def test_check_properties(gpu):
    cube = mp.check_properties(TriangleMesh(*R.cube()), max_tests=CAP)
    assert cube["watertight"] and cube["orientable"] and cube["edge_manifold_boundary"] and cube["vertex_manifold"]
    assert not cube["self_intersecting"] and len(cube["self_intersecting_pairs"]) == 0
    assert cube["quantum"] == 2.0 ** -20
    sheet = mp.check_properties(TriangleMesh(*R.sheet(7)), max_tests=CAP)
    assert not sheet["watertight"] and sheet["edge_manifold"] and not sheet["edge_manifold_boundary"]
    assert len(sheet["boundary_edges"]) == 28 and not sheet["self_intersecting"]
    verts, tris = pierced_cube()
    mesh = TriangleMesh(verts, tris)
    pierced = mp.check_properties(mesh, max_tests=CAP)
    assert not pierced["watertight"] and pierced["self_intersecting"] and pierced["vertex_manifold"]
    ijk = mp.quantize_mesh(verts)[0]
    assert np.array_equal(pierced["self_intersecting_pairs"], R.self_intersections(ijk, tris)[0])
    assert (pierced["self_intersecting_pairs"][:, 1] == 12).all()
    # the TriangleMesh methods say the same
    assert mesh.is_self_intersecting(max_tests=CAP) and not mesh.is_watertight(max_tests=CAP) and mesh.is_edge_manifold()
    assert not mesh.is_edge_manifold(allow_boundary_edges=False) and mesh.is_vertex_manifold() and mesh.is_orientable()
    assert np.array_equal(mesh.get_self_intersecting_triangles(max_tests=CAP), pierced["self_intersecting_pairs"])
    assert mesh.get_non_manifold_edges(allow_boundary_edges=False).tolist() == [[8, 9], [8, 10], [9, 10]]
    assert TriangleMesh(*R.cube()).is_watertight(max_tests=CAP)
    two = TriangleMesh(*R.two_tets_one_vertex())
    assert two.get_non_manifold_vertices().tolist() == [0] and not two.is_vertex_manifold() and not two.is_watertight(max_tests=CAP)
    assert not TriangleMesh(*R.moebius()).is_orientable()


def test_surface_clusters(gpu):
    """300 tetrahedra (4 triangles each), an octahedron (8) and a cube (12): what stays is what the
    restatement's rule keeps, cluster by cluster."""
    verts, tris = R.many_tets()
    ov, ot = R.octahedron()
    cv, ct = R.cube()
    tris = np.concatenate([tris[:500], ot + len(verts), tris[500:900], ct + len(verts) + len(ov), tris[900:]])
    verts = np.concatenate([verts, ov + 50.0, 3.0 * cv - 60.0])
    tris = tris.astype(np.int32)
    mesh = TriangleMesh(verts, tris)
    ref = R.topology(tris, len(verts), verts)
    octa, cube = ref["tri_cluster"][500], ref["tri_cluster"][908]
    assert ref["cluster_n"][octa] == 8 and ref["cluster_n"][cube] == 12

    def expect(**kw):
        return np.isin(ref["tri_cluster"], R.kept_clusters(ref["cluster_n"].tolist(), ref["cluster_area"].tolist(), **kw))

    for top_n, n_kept in ((1, 12), (2, 20), (3, len(tris)), (None, len(tris))):
        kept, removed, clusters = mp.get_surface_clusters(mesh, top_n_clusters=top_n)
        mask = expect(top_n_clusters=top_n)
        assert mask.sum() == n_kept
        assert np.array_equal(clusters, ref["tri_cluster"])
        assert np.array_equal(kept.triangles, tris[mask]) and np.array_equal(removed.triangles, tris[~mask])
    by_area = np.sort(ref["cluster_area"])
    lo, hi = float(by_area[10] + by_area[11]) / 2, float(by_area[-3] + by_area[-4]) / 2   # between clusters: no sum
    for kw in (dict(min_cluster_area=hi), dict(max_cluster_area=lo), dict(min_cluster_area=lo, max_cluster_area=hi),
               dict(top_n_clusters=2, max_cluster_area=float(ref["cluster_area"][octa]) + 1.0)):   # sits on a bound
        kept, removed, _ = mp.get_surface_clusters(mesh, **{"top_n_clusters": None, **kw})
        mask = expect(**{"top_n_clusters": None, **kw})
        assert 0 < mask.sum() < len(tris)
        assert np.array_equal(kept.triangles, tris[mask]) and np.array_equal(removed.triangles, tris[~mask])
    big = mp.cluster_and_remove_triangles(mesh, min_triangles=5)
    assert np.array_equal(big.triangles, tris[np.isin(ref["tri_cluster"], [octa, cube])])
    assert len(mesh.triangles) == len(tris)
