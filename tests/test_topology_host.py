"""The NumPy / SciPy statement of the skeleton-graph contract (tests/topology_restatement.py) against
hand-made forests and against the existing networkx chain collapse. No GPU."""
import networkx as nx
import numpy as np
import pytest

from pyqsm_amd.geometry import skeletonize as sk
from tests import topology_restatement as tr


def _chains(ends, ptr, members):
    return {(int(a), int(b)): members[ptr[c]:ptr[c + 1]].tolist() for c, (a, b) in enumerate(ends)}


def test_path_with_shuffled_labels():
    rng = np.random.default_rng(0)
    lab = rng.permutation(40)
    edges = np.stack([lab[:-1], lab[1:]], axis=1)[rng.permutation(39)]
    kept, ends, ptr, members = tr.collapse_chains(edges, 40)
    a, b = sorted((lab[0], lab[-1]))
    assert kept.tolist() == [a, b] and ends.tolist() == [[a, b]] and ptr.tolist() == [0, 38]
    walk = lab[1:-1] if lab[0] == a else lab[1:-1][::-1]
    assert members.tolist() == walk.tolist()


def test_star_direct_edges_and_isolated_nodes():
    star = [(0, i) for i in range(1, 50)]
    kept, ends, ptr, members = tr.collapse_chains(star, 50)
    assert kept.tolist() == list(range(50)) and len(ends) == 49 and len(members) == 0
    assert ptr.tolist() == [0] * 50
    kept, ends, ptr, members = tr.collapse_chains([(1, 0)], 2)
    assert kept.tolist() == [0, 1] and ends.tolist() == [[0, 1]] and ptr.tolist() == [0, 0]
    kept, ends, ptr, members = tr.collapse_chains(np.zeros((0, 2), int), 10)
    assert kept.tolist() == list(range(10)) and len(ends) == 0 and ptr.tolist() == [0]


def test_y_shape_by_hand():
    # junction 3, arms 3-1-0, 3-4-5-6, 3-2 ; leaves 0, 6, 2
    edges = [(3, 1), (1, 0), (3, 4), (5, 4), (5, 6), (2, 3)]
    kept, ends, ptr, members = tr.collapse_chains(edges, 7)
    assert kept.tolist() == [0, 2, 3, 6]
    assert _chains(ends, ptr, members) == {(0, 3): [1], (2, 3): [], (3, 6): [4, 5]}
    assert ends.tolist() == [[0, 3], [2, 3], [3, 6]]


def test_matches_simplify_graph_on_a_knn_tree():
    rng = np.random.default_rng(5)
    t = np.linspace(0, 1, 150)
    P = np.concatenate([np.outer(t, d) for d in ([1, 0, 0.3], [-0.6, 0.7, 0.2], [0.1, -0.9, 0.4], [0.2, 0.3, -1])])
    P = P[rng.permutation(len(P))] + rng.normal(0, 2e-3, (len(P), 3))
    edges, w = tr.skeletal_forest(P, 8)
    assert len(edges) == len(P) - tr.n_components(edges, len(P))
    kept, ends, ptr, members = tr.collapse_chains(edges, len(P))
    G = nx.Graph(edges.tolist())
    G.add_nodes_from(range(len(P)))
    for i in range(len(P)):
        G.nodes[i]["pos"] = P[i]
    S, _, kept_ref = sk.simplify_graph(G)
    assert sorted(kept_ref) == kept.tolist()
    ref = {(min(a, b), max(a, b)): sorted(d.get("data", [])) for a, b, d in S.edges(data=True)}
    got = {key: sorted(v) for key, v in _chains(ends, ptr, members).items()}
    assert got == ref
    assert ends.tolist() == sorted(ends.tolist())


def test_forest_never_lists_zero_length_pairs_and_handles_components():
    rng = np.random.default_rng(1)
    P = rng.random((60, 3))
    P = np.concatenate([P, P[:7]])                       # seven exact copies
    edges, w = tr.skeletal_forest(P, 6)
    assert (w > 0).all() and len(edges) == 66 - 7        # a copy is tied to its original by the unlisted edge
    assert len(edges) == len(P) - tr.n_components(edges, len(P))
    Q = np.concatenate([rng.random((30, 3)), rng.random((30, 3)) + 50.0])
    edges, _ = tr.skeletal_forest(Q, 5)
    assert len(edges) == 58 and tr.n_components(edges, 60) == 2


def test_a_ring_is_refused():
    ring = [(i, (i + 1) % 12) for i in range(12)]
    with pytest.raises(ValueError):
        tr.collapse_chains(ring, 12)
    with pytest.raises(ValueError):
        tr.collapse_chains(ring + [(0, 12)], 13)         # a ring through a kept node
    with pytest.raises(ValueError):
        tr.collapse_chains([(0, 5)], 3)


def test_radii_and_surface_restatement():
    shift = np.full((10, 3), 0.05 / np.sqrt(3))
    r = tr.chain_radii(shift, np.array([0, 3, 3]), np.array([1, 2, 3]))
    assert np.allclose(r, [0.05, 0.0])
    imap = np.array([9, 8, 7, 6])
    shift[6:] *= 2
    assert np.allclose(tr.chain_radii(shift, np.array([0, 3]), np.array([1, 2, 3]), imap), 0.1)
    from pyqsm_amd.geometry.cloud import Cylinder
    cyl = Cylinder([1.0, 2.0, 3.0], 0.05, 0.8, [0.3, -0.2, 1.0])
    u, v = cyl._frame()
    pts = tr.cylinder_surface(cyl.center, cyl.axis, u, v, cyl.radius, cyl.height)
    assert 1000 < len(pts) <= 2000 and np.array_equal(pts, np.unique(pts, axis=0))


def test_binding_rejects_bad_k_before_any_device():
    """k outside [1, 192] is refused by the library itself, with or without a GPU."""
    from pyqsm_amd import _lib, hip
    for k in (0, 193):
        with pytest.raises(_lib.PyQSMHipError) as e:
            hip.skeletal_forest(np.zeros((4, 3)), k)
        assert e.value.code == -4
