"""Cluster adjacency without a GPU: the contract's CPU statement against SciPy's own loop and the
stored fixture, and the host logic of pyqsm_amd.cluster_joining with hip.cluster_adjacency replaced
by the restatement."""
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

from pyqsm_amd import cluster_joining as cj
from pyqsm_amd import hip
from pyqsm_amd.geometry.cloud import PointCloud
from tests import adjacency_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adjacency_blocks.npz")


@pytest.fixture(scope="module")
def blocks():
    P, lab = R.block_cloud()
    return R.split_blocks(P, lab)


@pytest.fixture
def restated(monkeypatch):
    monkeypatch.setattr(hip, "cluster_adjacency", R.restated_cluster_adjacency)


@pytest.mark.parametrize("threshold", [0.35, 0.2])
def test_restatement_equals_scipy_loop_on_blocks(blocks, threshold):
    assert R.adjacency(*blocks, threshold) == R.scipy_loop(*blocks, threshold)


def test_restatement_equals_scipy_loop_on_lattice():
    got = R.adjacency(*R.lattice(), 0.25)
    assert got == R.scipy_loop(*R.lattice(), 0.25)
    assert got == {(0, 1): (0.25, 18), (0, 2): (0.25, 18), (0, 7): (0.0, 4)}


def test_golden_fixture_matches_restatement(blocks):
    g = np.load(GOLDEN)
    P = g["block_points"].astype(np.float64)
    assert np.array_equal(np.concatenate([blocks[0], blocks[2]]),
                          np.concatenate(R.split_blocks(P, g["block_labels"].astype(np.int64))[0::2]))
    cases = [(f"block{k}", R.split_blocks(P, g["block_labels"].astype(np.int64)), float(t))
             for k, t in enumerate(g["block_thresholds"])]
    cases.append(("lattice", (g["lattice_src"], g["lattice_src_labels"], g["lattice_tgt"], g["lattice_tgt_labels"]),
                  float(g["lattice_threshold"])))
    for name, clouds, threshold in cases:
        res = R.as_result(R.adjacency(*clouds, threshold))
        assert len(res.a) > 0, name
        assert np.array_equal(np.stack([res.a, res.b], 1), g[f"{name}_ab"]), name
        assert np.array_equal(res.dist, g[f"{name}_dist"]), name
        assert np.array_equal(res.n_pairs, g[f"{name}_pairs"]), name


def test_witness_tie_break_of_the_restatement():
    src = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 0, 0]])
    tgt = np.array([[0.1, 0, 0], [-0.1, 0, 0], [1.1, 0, 0]])
    got = R.adjacency(src, [5, 5, 5], tgt, [9, 9, 9], 0.2, witness=True)
    # (0,0), (0,1), (2,0), (2,1) attain 0.1 exactly; (1,2) is 1.1 - 1.0 > 0.1
    assert got == {(5, 9): (0.1, 5, 0, 0)}


def _clusters():
    """Six small clusters on a line, 0.3 apart edge to edge except 40 (far away); label 0 is a
    cluster too and must never be reported."""
    rng = np.random.default_rng(5)
    base = rng.uniform(0, 0.2, (30, 3))
    at = {10: 0.0, 0: 0.5, 20: 1.0, 30: 1.5, 50: 2.0, 40: 50.0}
    return [(lab, base + [x, 0, 0]) for lab, x in at.items()]


def test_determine_adjacency_exclusions_and_order(restated):
    cl = _clusters()
    adj = cj.determine_adjacency([10, 30, 40], cl, threshold=0.9)
    assert list(adj) == [10, 30, 40]
    # 0 is nearest to 10 but excluded; 30 is in label_list; 20 and 50 in the order of the list
    assert list(adj[10]) == [20]
    assert list(adj[30]) == [20, 50]
    assert adj[40] == {}
    ref = R.scipy_loop(np.concatenate([p for _, p in cl]), np.repeat([l for l, _ in cl], 30),
                       np.concatenate([p for _, p in cl]), np.repeat([l for l, _ in cl], 30), 0.9)
    assert adj[10][20] == ref[(10, 20)][0] and adj[30][50] == ref[(30, 50)][0] and adj[30][20] == ref[(30, 20)][0]
    assert all(isinstance(k, int) for k in adj) and isinstance(adj[10][20], float)


def test_determine_adjacency_order_follows_kdtrees_not_labels(restated):
    cl = _clusters()
    shuffled = [cl[k] for k in (4, 3, 2, 1, 0, 5)]
    adj = cj.determine_adjacency([30], shuffled, threshold=0.9)
    assert list(adj[30]) == [50, 20]


def test_determine_adjacency_separate_sources(restated):
    cl = _clusters()
    src = [(7, cl[0][1]), (8, cl[5][1]), (9, cl[1][1])]       # 9 is not in label_list
    adj = cj.determine_adjacency([7, 8], cl, threshold=0.9, src_kdtrees=src)
    assert list(adj) == [7, 8]
    assert list(adj[7]) == [10, 20] and adj[7][10] == 0.0      # label 0 skipped, 10 is a copy of 7
    assert list(adj[8]) == [40]


def test_determine_adjacency_accepts_trees_arrays_and_clouds(restated):
    cl = _clusters()
    want = cj.determine_adjacency([10, 30], cl, threshold=0.9)
    mixed = [(lab, (cKDTree(p), p.tolist(), PointCloud(p))[k % 3]) for k, (lab, p) in enumerate(cl)]
    assert cj.determine_adjacency([10, 30], mixed, threshold=0.9) == want


def test_determine_adjacency_writes_nothing_unless_asked(restated, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cl = _clusters()
    adj = cj.determine_adjacency([10], cl, threshold=0.9, case_name="x")
    assert os.listdir(tmp_path) == []
    cj.determine_adjacency([10], cl, threshold=0.9, case_name="x", save=True)
    assert os.listdir(tmp_path) == ["adj_x.pkl"]
    import pickle
    with open(tmp_path / "adj_x.pkl", "rb") as f:
        assert pickle.load(f) == adj


def test_duplicate_labels_raise(restated):
    cl = _clusters()
    with pytest.raises(ValueError):
        cj.determine_adjacency([10], cl + [cl[2]])
    with pytest.raises(ValueError):
        cj.determine_adjacency([10], cl, src_kdtrees=[cl[0], cl[0]])


def test_create_kdtrees_sampling():
    rng = np.random.default_rng(2)
    coords = rng.normal(size=(1000, 3))
    labels = rng.integers(0, 7, 1000) * 3
    got = cj.create_kdtrees(coords, labels)
    assert [l for l, _ in got] == list(np.unique(labels))
    for l, pts in got:
        assert np.array_equal(pts, coords[labels == l][::10])
    exact = cj.create_kdtrees(PointCloud(coords), labels, sample_every=1)
    assert sum(len(p) for _, p in exact) == 1000
    with pytest.raises(ValueError):
        cj.create_kdtrees(coords, labels[:-1])


def test_closest_clusters():
    adj = {1: {5: 0.3, 6: 0.1, 7: 0.2, 8: 0.05}, 2: {}}
    assert cj.closest_clusters(adj, 1, 2).tolist() == [8, 6]
    assert cj.closest_clusters(adj, 1, 15).tolist() == [8, 6, 7, 5]
    assert cj.closest_clusters(adj, 2, 3).tolist() == []
    assert cj.closest_clusters(adj, 99, 3).tolist() == []


def test_cluster_adjacency_graph_is_the_same_cloud_form(restated):
    cl = _clusters()
    P = np.concatenate([p for _, p in cl])
    lab = np.repeat([l for l, _ in cl], 30)
    lab[::7] = -1
    res = cj.cluster_adjacency_graph(PointCloud(P), lab, threshold=0.9, return_pairs=True)
    assert R.as_dict(res, witness=True) == R.adjacency(P, lab, P, lab, 0.9, same_cloud=True, witness=True)
    assert np.all(res.a < res.b) and len(res.a) > 0


def test_wrapper_host_paths_need_no_device():
    """Empty and all-ignored inputs return an empty graph, bad arguments raise, before any device is touched."""
    e = hip.cluster_adjacency(np.zeros((0, 3)), np.zeros(0, np.int64), 0.3, return_pairs=True)
    assert len(e.a) == len(e.b) == len(e.dist) == len(e.n_pairs) == len(e.src_idx) == len(e.tgt_idx) == 0
    e = hip.cluster_adjacency(np.zeros((4, 3)), [-1, -1, -5, -1], 0.3, np.zeros((2, 3)), [3, 4])
    assert len(e.a) == 0 and e.src_idx is None
    e = hip.cluster_adjacency(np.zeros((4, 3)), [1, 2, 3, 4], 0.3, np.zeros((0, 3)), [])
    assert len(e.a) == 0
    with pytest.raises(ValueError):
        hip.cluster_adjacency(np.zeros((4, 3)), [1, 2, 3], 0.3)
    with pytest.raises(ValueError):
        hip.cluster_adjacency(np.zeros((4, 3)), [1, 2, 3, 4], 0.3, np.zeros((2, 3)), [1])
    with pytest.raises(hip._lib.PyQSMHipError) as err:
        hip.cluster_adjacency(np.zeros((4, 3)), [1, 2, 3, 4], 0.0)
    assert err.value.code == -1
    bad = np.zeros((4, 3))
    bad[2, 1] = np.nan
    with pytest.raises(hip._lib.PyQSMHipError) as err:
        hip.cluster_adjacency(bad, [1, 2, 3, 4], 0.3)
    assert err.value.code == -1
