"""The skeleton graph and the cylinder table on the device (csrc/topology.hip) against
SciPy's minimum spanning tree, the plain-Python chain walk of tests/topology_restatement.py and the
existing host path (extract_skeletal_graph, simplify_graph, skeleton_to_QSM)."""
import math

import numpy as np
import pytest

from pyqsm_amd import _lib, hip, synth
from pyqsm_amd.geometry import skeletonize as sk
from tests import deep_chain
from tests import topology_restatement as tr

pytestmark = pytest.mark.gpu


def _tree_skeleton(n=20_000, seed=3):
    """A contracted tree: the layout of synth.tree_unit (trunk, five branches) with the cylinders
    shrunk to tubes of a few millimetres, coordinates float32-representable like synth's."""
    rng = np.random.default_rng(seed)
    n_trunk = n // 2
    n_branch = (n - n_trunk) // 5
    parts = [synth._cylinder(rng, n_trunk, 0.004, 6.0, 0.001)]
    tilt = np.pi / 2.0 - np.deg2rad(37.0)
    ct, st = np.cos(tilt), np.sin(tilt)
    for b in range(5):
        nb = n_branch if b < 4 else n - n_trunk - 4 * n_branch
        c = synth._cylinder(rng, nb, 0.002, 3.0, 0.0005)
        x, y, z = c[:, 0] * ct + c[:, 2] * st, c[:, 1], -c[:, 0] * st + c[:, 2] * ct
        ca, sa = np.cos(2.0 * np.pi * b / 5.0), np.sin(2.0 * np.pi * b / 5.0)
        parts.append(np.stack([x * ca - y * sa, x * sa + y * ca, z + 2.0 + 0.7 * b], axis=1))
    return np.concatenate(parts).astype(np.float32).astype(np.float64)


def _y_shape():
    rng = np.random.default_rng(2)
    t = np.linspace(0.05, 1.0, 400)
    arms = [np.outer(t, d) for d in ([1, 0, 0.2], [-0.5, 0.8, 0.3], [-0.4, -0.9, 0.1])]
    return np.concatenate(arms) + rng.normal(0, 1e-3, (1200, 3)) + [2.0, 2.0, 2.0]


def _knn_d2_of(P, k, edges, gpu):
    """The kNN's own d2 of every edge (the smaller direction, should both be listed)."""
    idx, d2 = hip.knn(P, k, True, device=gpu)
    table = {}
    for i in range(len(P)):
        for j, w in zip(idx[i], d2[i]):
            if j < len(P):
                key = (min(i, int(j)), max(i, int(j)))
                table[key] = min(table.get(key, np.inf), w)
    return np.array([table[(int(a), int(b))] for a, b in edges])


def _scipy_on_gpu_knn(P, k, gpu):
    """SciPy's tree of the library's own kNN table: what extract_skeletal_graph builds today."""
    n = len(P)
    idx, d2 = hip.knn(P, k, True, device=gpu)
    valid = (idx < n).ravel()
    rows = np.repeat(np.arange(n), k)[valid]
    return tr.forest_from_entries(rows, idx.ravel()[valid], np.sqrt(d2.ravel()[valid]), n)


def _check_layout(edges, n):
    assert edges.dtype == np.int32 and edges.ndim == 2 and edges.shape[1] == 2
    assert (edges[:, 0] < edges[:, 1]).all() and edges.min(initial=0) >= 0 and edges.max(initial=0) < max(n, 1)
    packed = edges[:, 0].astype(np.int64) << 32 | edges[:, 1]
    assert (np.diff(packed) > 0).all()


@pytest.fixture(scope="module")
def tree(gpu):
    P = _tree_skeleton()
    edges, d2, rounds = hip.skeletal_forest(P, 15, return_rounds=True, device=gpu)
    chains = hip.collapse_chains(edges, len(P), device=gpu)
    topo = sk.TopologyArrays(P, np.random.default_rng(8).permutation(len(P)).astype(np.int32), edges,
                             np.sqrt(d2), *chains)
    return {"P": P, "edges": edges, "d2": d2, "rounds": rounds, "chains": chains, "topo": topo}


# ---- forest ---------------------------------------------------------------------------------

def test_forest_uniform_points_equal_scipy(gpu):
    P = np.random.default_rng(0).random((2000, 3))
    edges, d2, rounds = hip.skeletal_forest(P, 8, return_rounds=True, device=gpu)
    _check_layout(edges, 2000)
    want, _ = tr.skeletal_forest(P, 8)
    assert np.array_equal(edges, want)
    assert np.array_equal(d2.view(np.uint64), _knn_d2_of(P, 8, edges, gpu).view(np.uint64))
    assert 1 <= rounds <= math.ceil(math.log2(2000))
    e2, l2 = sk.skeletal_forest(P, 8, device=gpu)
    assert np.array_equal(e2, edges) and np.array_equal(l2, np.sqrt(d2))


def test_forest_tree_skeleton_equal_scipy(gpu, tree):
    P, edges = tree["P"], tree["edges"]
    _check_layout(edges, len(P))
    want, _ = tr.skeletal_forest(P, 15)
    assert np.array_equal(edges, want)
    assert np.array_equal(tree["d2"].view(np.uint64), _knn_d2_of(P, 15, edges, gpu).view(np.uint64))
    assert 2 <= tree["rounds"] <= math.ceil(math.log2(len(P)))
    assert len(edges) == len(P) - tr.n_components(edges, len(P))


def test_forest_all_ties_on_a_lattice(gpu):
    g = np.arange(8, dtype=np.float64)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    edges, d2 = hip.skeletal_forest(P, 6, device=gpu)
    _check_layout(edges, 512)
    assert len(edges) == 511 and tr.n_components(edges, 512) == 1        # acyclic and spanning
    _, w = _scipy_on_gpu_knn(P, 6, gpu)
    assert len(w) == 511 and w.sum() == 511.0
    assert np.array_equal(np.sort(np.sqrt(d2)).view(np.uint64), np.sort(w).view(np.uint64))
    again = hip.skeletal_forest(P, 6, device=gpu)
    assert np.array_equal(again[0], edges) and np.array_equal(again[1].view(np.uint64), d2.view(np.uint64))


def test_forest_disconnected_blobs(gpu):
    rng = np.random.default_rng(4)
    P = np.concatenate([rng.normal(0, 1, (300, 3)), rng.normal(0, 1, (300, 3)) + [50.0, 0, 0]])
    edges, d2 = hip.skeletal_forest(P, 5, device=gpu)
    _check_layout(edges, 600)
    want, _ = tr.skeletal_forest(P, 5)
    assert len(want) == 598                  # each blob's 5-NN graph is connected (SciPy, on the CPU)
    assert len(edges) == 598 and np.array_equal(edges, want)
    assert ((edges[:, 0] < 300) == (edges[:, 1] < 300)).all()            # no edge between the blobs


def test_forest_duplicates(gpu):
    rng = np.random.default_rng(6)
    P = rng.random((500, 3))
    P = np.concatenate([P, P[rng.choice(500, 50, replace=False)]])
    edges, d2 = hip.skeletal_forest(P, 8, device=gpu)
    _check_layout(edges, 550)
    want, w = _scipy_on_gpu_knn(P, 8, gpu)
    assert len(edges) == len(want)
    assert np.array_equal(np.sort(np.sqrt(d2)).view(np.uint64), np.sort(w).view(np.uint64))
    assert (d2 > 0).all()
    assert len(edges) == 550 - tr.n_components(edges, 550)               # acyclic


def test_forest_small_and_invalid_inputs(gpu):
    for m in (0, 1):
        edges, d2, rounds = hip.skeletal_forest(np.zeros((m, 3)), 4, return_rounds=True, device=gpu)
        assert edges.shape == (0, 2) and d2.shape == (0,) and rounds == 0
    edges, d2 = hip.skeletal_forest(np.array([[0.0, 0, 0], [3.0, 4.0, 0]]), 1, device=gpu)
    assert edges.tolist() == [[0, 1]] and d2.tolist() == [25.0]
    edges, d2 = hip.skeletal_forest(np.zeros((2, 3)), 1, device=gpu)       # two coincident points
    assert len(edges) == 0
    P = np.random.default_rng(9).random((5, 3))
    edges, d2 = hip.skeletal_forest(P, 15, device=gpu)                     # padded rows
    want, w = tr.skeletal_forest(P, 15)
    assert np.array_equal(edges, want) and len(edges) == 4
    for k in (0, 193):
        with pytest.raises(_lib.PyQSMHipError) as e:
            hip.skeletal_forest(P, k, device=gpu)
        assert e.value.code == -4


@pytest.mark.parametrize("permuted", [False, True])
def test_forest_single_deep_chain(gpu, permuted):
    """Strictly decreasing gaps along the x axis: the first round hooks all m points into one tree of
    depth m - 2 (tests/deep_chain.py), which the bounded pointer jumping has to flatten."""
    m = 4096
    gaps = 1.0 + (m - np.arange(m - 1)) / m
    x = np.r_[0.0, np.cumsum(gaps)]
    label = deep_chain.relabel(m, permuted, 21)
    a, b = deep_chain.line_graph(x, 2)
    deep_chain.assert_one_chain(a, b, (x[b] - x[a]) ** 2, label)
    P = np.zeros((m, 3))
    P[label, 0] = x
    edges, d2, rounds = hip.skeletal_forest(P, 2, return_rounds=True, device=gpu)
    assert rounds == 1
    _check_layout(edges, m)
    want, _ = tr.skeletal_forest(P, 2)
    assert len(want) == m - 1 and np.array_equal(edges, want)
    if not permuted:
        assert np.array_equal(edges, np.stack([np.arange(m - 1), np.arange(1, m)], axis=1))
    assert np.array_equal(d2.view(np.uint64), _knn_d2_of(P, 2, edges, gpu).view(np.uint64))


# ---- chains ---------------------------------------------------------------------------------

def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_chains_long_path_with_shuffled_labels(gpu):
    rng = np.random.default_rng(11)
    lab = rng.permutation(3000)
    edges = np.stack([lab[:-1], lab[1:]], axis=1)[rng.permutation(2999)]
    kept, ends, ptr, members = hip.collapse_chains(edges, 3000, device=gpu)
    a, b = sorted((int(lab[0]), int(lab[-1])))
    assert kept.tolist() == [a, b] and ends.tolist() == [[a, b]] and ptr.tolist() == [0, 2998]
    walk = lab[1:-1] if lab[0] == a else lab[1:-1][::-1]
    assert np.array_equal(members, walk)
    _same((kept, ends, ptr, members), tr.collapse_chains(edges, 3000))


def test_chains_star_direct_edge_and_isolated_nodes(gpu):
    star = np.array([(0, i) for i in range(1, 50)])
    got = hip.collapse_chains(star, 50, device=gpu)
    assert len(got[1]) == 49 and len(got[3]) == 0 and got[2].tolist() == [0] * 50
    _same(got, tr.collapse_chains(star, 50))
    got = hip.collapse_chains([(1, 0)], 2, device=gpu)
    assert got[0].tolist() == [0, 1] and got[1].tolist() == [[0, 1]] and got[2].tolist() == [0, 0]
    got = hip.collapse_chains(np.zeros((0, 2), np.int32), 10, device=gpu)
    assert got[0].tolist() == list(range(10)) and len(got[1]) == 0 and got[2].tolist() == [0]
    got = hip.collapse_chains(np.zeros((0, 2), np.int32), 0, device=gpu)
    assert len(got[0]) == 0 and got[2].tolist() == [0]
    with pytest.raises(_lib.PyQSMHipError):
        hip.collapse_chains([(0, 7)], 3, device=gpu)                      # a node outside the range


def test_chains_y_shape(gpu):
    topo = sk.extract_topology_arrays(_y_shape(), graph_k_n=8, device=gpu)
    assert len(topo.skeleton_points) == 120 and len(topo.edges) == 119
    assert len(topo.kept) == 4 and len(topo.chain_ends) == 3 and len(topo.members) == 116
    _same((topo.kept, topo.chain_ends, topo.chain_ptr, topo.members), tr.collapse_chains(topo.edges, 120))
    assert topo.topology.points.shape == (4, 3) and topo.topology.lines.shape == (3, 2)
    G = topo.to_networkx()
    assert sorted(d for _, d in G.degree()) == [1, 1, 1, 3]
    assert np.array_equal(_y_shape()[topo.sample_idx], topo.skeleton_points)


def test_chains_end_to_end_equal_simplify_graph(gpu, tree):
    P = tree["P"]
    kept, ends, ptr, members = tree["chains"]
    G, _ = sk.extract_skeletal_graph(P, 15, device=gpu)
    S, _, kept_ref = sk.simplify_graph(G)
    assert sorted(kept_ref) == kept.tolist()
    ref = {(min(a, b), max(a, b)): sorted(d.get("data", [])) for a, b, d in S.edges(data=True)}
    got = {(int(a), int(b)): sorted(members[ptr[c]:ptr[c + 1]].tolist()) for c, (a, b) in enumerate(ends)}
    assert got == ref
    _same((kept, ends, ptr, members), tr.collapse_chains(tree["edges"], len(P)))


# ---- radii ----------------------------------------------------------------------------------

def _radii_close(got, want, ptr):
    n = np.diff(ptr)
    assert got.shape == want.shape
    for g, w, length in zip(got, want, n):
        assert abs(g - w) <= (length + 4) * 2.0 ** -52 * w, (g, w, length)


def test_radii_y_shape_uniform_shift(gpu):
    topo = sk.extract_topology_arrays(_y_shape(), graph_k_n=8, device=gpu)
    shift = np.full((1200, 3), 0.05 / np.sqrt(3))
    for imap in (None, topo.sample_idx):
        r = hip.chain_radii(shift, topo.chain_ptr, topo.members, imap, device=gpu)
        _radii_close(r, tr.chain_radii(shift, topo.chain_ptr, topo.members, imap), topo.chain_ptr)
        assert np.allclose(r, 0.05, rtol=1e-13, atol=0)
    qsm = sk.skeleton_to_QSM_arrays(topo, shift, surfaces=False, device=gpu)
    assert len(qsm["radius"]) == 3 and np.allclose(qsm["radius"], 0.05)
    assert ((0.8 < qsm["height"]) & (qsm["height"] < 1.1)).all()


def test_radii_random_shifts_on_the_tree(gpu, tree):
    topo = tree["topo"]
    shift = np.random.default_rng(12).normal(0, 0.05, (len(tree["P"]), 3))
    for imap in (None, topo.sample_idx):
        r = hip.chain_radii(shift, topo.chain_ptr, topo.members, imap, device=gpu)
        _radii_close(r, tr.chain_radii(shift, topo.chain_ptr, topo.members, imap), topo.chain_ptr)
    with pytest.raises(_lib.PyQSMHipError):
        hip.chain_radii(shift[:100], topo.chain_ptr, topo.members, device=gpu)     # members beyond the table


def test_radii_long_chain(gpu):
    """2 998 members: beyond the 128-term blocks of the summation."""
    shift = np.random.default_rng(14).normal(0, 0.05, (3000, 3))
    ptr, members = np.array([0, 2998]), np.random.default_rng(15).permutation(3000)[:2998].astype(np.int32)
    r = hip.chain_radii(shift, ptr, members, device=gpu)
    _radii_close(r, tr.chain_radii(shift, ptr, members), ptr)


# ---- surfaces -------------------------------------------------------------------------------

def _surfaces_equal_host_path(topo, shift, gpu):
    """Bit-equal surface rows presuppose bit-equal radii: the host path takes np.mean, the kernel
    restates NumPy's pairwise summation order. Should a NumPy release sum differently, the radii
    assertion below fails first and names the cause; the radii contract itself is only the bound."""
    all_pcd, cyls, objs, radii = sk.skeleton_to_QSM(topo.topology, topo.to_networkx(), shift)
    qsm = sk.skeleton_to_QSM_arrays(topo, shift, device=gpu)
    ptr, pts = qsm["surface_ptr"], qsm["surface_points"]
    assert len(cyls) == len(qsm["radius"]) == len(ptr) - 1
    assert np.array_equal(qsm["radius"], np.array(radii)), "radii differ from np.mean in their bits: NumPy sums in another order"
    assert ptr[0] == 0 and ptr[-1] == len(pts) and ptr.dtype == np.int64
    assert np.array_equal(np.diff(ptr), [len(c.points) for c in cyls])
    for i, c in enumerate(cyls):
        got = np.ascontiguousarray(pts[ptr[i]:ptr[i + 1]])
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(c.points).view(np.uint64)), i
    assert np.array_equal(qsm["height"], [o.height for o in objs])
    lengths = np.diff(topo.chain_ptr)[qsm["chain"]]
    _radii_close(qsm["radius"], np.array(radii), np.r_[0, np.cumsum(lengths)])
    return qsm


def test_surfaces_y_shape(gpu):
    topo = sk.extract_topology_arrays(_y_shape(), graph_k_n=8, device=gpu)
    qsm = _surfaces_equal_host_path(topo, np.full((1200, 3), 0.05 / np.sqrt(3)), gpu)
    assert len(qsm["radius"]) == 3 and len(qsm["surface_points"]) > 1000


def test_surfaces_on_the_tree(gpu, tree):
    shift = np.abs(np.random.default_rng(13).normal(0, 0.03, (len(tree["P"]), 3)))
    qsm = _surfaces_equal_host_path(tree["topo"], shift, gpu)
    assert len(qsm["radius"]) > 10


@pytest.mark.parametrize("start,end,radius", [
    ([1.0, 2.0, 3.0], [2.5, 2.0, 3.0], 0.05),             # axis along x: the other helper of _frame
    ([1.0, 2.0, 3.0], [1.0, 2.0, 3.0001], 0.05),          # height 1e-4: the levels collapse
    ([1.0, 2.0, 3.0], [1.3, 2.4, 3.2], 1e-4),             # radius 1e-4: the angles collapse
])
def test_surfaces_single_cylinders(gpu, start, end, radius):
    start, end = np.array(start), np.array(end)
    P = np.stack([start, (start + end) / 2.0, end])
    chains = hip.collapse_chains([(0, 1), (1, 2)], 3, device=gpu)
    topo = sk.TopologyArrays(P, np.arange(3, dtype=np.int32), np.array([[0, 1], [1, 2]], np.int32), None, *chains)
    shift = np.zeros((3, 3))
    shift[1] = [radius, 0, 0]
    qsm = _surfaces_equal_host_path(topo, shift, gpu)
    assert len(qsm["radius"]) == 1 and qsm["radius"][0] == radius
    assert 1 <= len(qsm["surface_points"]) <= 2000
