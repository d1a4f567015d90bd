"""tests/amg_restatement.py checked against things it was not written from (CPU only): graph
properties of the aggregation, SciPy's triple product, the cycle assembled from explicit matrices and
the spectrum a symmetric V-cycle must have; and the level structure of the cases that
tests/test_gpu_amg.py sends to the device."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from tests import amg_restatement as R

SMALL = ["A", "A96", "C96", "F96"]           # dense matrices of the whole operator are formed for these


def _py_priority(i):
    m = 0xFFFFFFFF
    h = (i * 0x9E3779B1) & m
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m
    h ^= h >> 16
    return ((h >> 1) << 32) | ((i + 1) & m)


def test_priority_wraps_like_uint32():
    idx = [0, 1, 2, 63, 64, 1499, 12399, 2 ** 16, 2 ** 24 + 5, 2 ** 31 - 2, 2 ** 31 - 1]
    got = R.priority(np.array(idx))
    assert [int(v) for v in got] == [_py_priority(i) for i in idx]
    assert len(set(int(v) for v in R.priority(np.arange(100000)))) == 100000      # a strict order
    assert int(got.max()) < 2 ** 64 - 1                                           # below the root mark


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_cases_have_the_stated_level_structure(name):
    _, _, sizes, stop, coarse = R.CASES[name]
    H = R.restated(name)
    assert [L["n"] for L in H["levels"]] == sizes
    assert (H["stop"], H["coarse"]) == (stop, coarse)
    for s in sizes[1:]:
        assert s % 32 != 0                      # no size on a tile boundary of the dense kernels
    if name.startswith("A"):
        assert int((H["levels"][0]["agg"] < 0).sum()) == 3
    if name == "C96":
        assert R.FUSED_TAIL_MAX_ROWS >= sizes[-1] > R.COARSE_MAX
    if name == "D":
        assert sizes[-1] > R.FUSED_TAIL_MAX_ROWS
    if name == "E":                             # most of level 1 is not represented below
        assert int((H["levels"][1]["agg"] < 0).sum()) == 2370
    if name == "F96":                           # the cap stops the SECOND coarsening, above the dense limit
        last = H["levels"][1]
        agg, _, _, nc, _ = R.aggregate(last["indptr"], last["indices"], last["vals"], last["diag"])
        assert 0 < nc <= 0.8 * last["n"] and R.galerkin(last["indptr"], last["indices"], last["vals"], agg, nc) is None
        assert int(np.diff(last["indptr"]).max()) <= R.ROW_CAP
    if name == "G":                             # ... the first
        assert int(np.diff(H["levels"][0]["indptr"]).max()) > R.ROW_CAP


def _strong_graph(L):
    s = R.strong(L["indptr"], L["indices"], L["vals"], L["diag"])
    return sp.csr_matrix((np.ones(int(s.sum())), (R.rows_of(L["indptr"])[s], L["indices"][s])), shape=(L["n"],) * 2)


@pytest.mark.parametrize("name", ["A96", "B96", "C96", "E", "F96"])
def test_roots_are_a_maximal_independent_set_of_the_squared_graph(name):
    H = R.restated(name)
    for L in H["levels"][:-1]:
        S = _strong_graph(L)
        assert (S != S.T).nnz == 0
        S2 = (S + S @ S).tocsr()
        S2.setdiag(0)
        S2.eliminate_zeros()
        roots = L["roots"]
        assert S2[roots][:, roots].nnz == 0                               # no two within two strong steps
        has = np.diff(S.indptr) > 0
        near = np.asarray(S2 @ roots.astype(float)).ravel() > 0
        assert np.array_equal(near | roots, has)                          # maximal; the rest has no strong edge
        agg, nc = L["agg"], H["levels"][H["levels"].index(L) + 1]["n"]
        assert np.array_equal(agg < 0, ~has)
        assert np.array_equal(np.bincount(agg[roots], minlength=nc), np.ones(nc, int))   # one root each
        coo = S.tocoo()
        inside = agg[coo.row] == agg[coo.col]
        G = sp.csr_matrix((np.ones(int(inside.sum())), (coo.row[inside], coo.col[inside])), shape=S.shape)
        ncomp, lab = connected_components(G, directed=False)
        assert ncomp == nc + int((~has).sum())                            # every aggregate is connected
        assert np.array_equal(L["members"], np.lexsort((np.arange(L["n"]), agg))[(agg < 0).sum():])
        assert np.array_equal(np.diff(L["mptr"]), np.bincount(agg[agg >= 0], minlength=nc))


@pytest.mark.parametrize("name", ["A96", "B96", "C96", "E", "F96"])
def test_coarse_matrices_are_the_triple_product(name):
    H = R.restated(name)
    for l, L in enumerate(H["levels"][:-1]):
        C = H["levels"][l + 1]
        P = R.prolongation(L, C["n"])
        ref = (P.T @ R.csr(L) @ P).tocsr()
        ref.sort_indices()
        got = R.csr(C)
        assert np.array_equal(ref.indptr, got.indptr) and np.array_equal(ref.indices, got.indices)
        rowsum = np.asarray(abs(P.T @ abs(R.csr(L)) @ P).sum(axis=1)).ravel()
        assert (np.abs(ref.data - got.data) <= 1e-14 * rowsum[R.rows_of(got.indptr)]).all()
        T = got.T.tocsr()
        T.sort_indices()
        assert np.array_equal(T.indices, got.indices) and np.array_equal(T.data, got.data)    # bitwise symmetric
        d, dinv = R.diag_l1(C["indptr"], C["indices"], C["vals"])
        assert np.array_equal(d, got.diagonal())
        assert np.allclose(1.0 / dinv, np.asarray(abs(got).sum(axis=1)).ravel(), rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", ["A96", "C96"])
def test_ap_table_is_a_times_p(name):
    H = R.restated(name)
    L, C = H["levels"][0], H["levels"][1]
    ptr, idx, val = R.ap_table(L["indptr"], L["indices"], L["vals"], L["agg"])
    AP = (R.csr(L) @ R.prolongation(L, C["n"])).tocsr()
    got = sp.csr_matrix((val.astype(np.float64), idx, ptr), shape=AP.shape)
    assert got.has_canonical_format or len(set(zip(R.rows_of(ptr).tolist(), idx.tolist()))) == len(idx)
    absap = abs(R.csr(L)) @ R.prolongation(L, C["n"])
    assert abs(got - AP).max() <= 16 * 2.0 ** -24 * absap.max()
    for i in (0, 1, L["n"] - 1):                                         # order of first occurrence
        a = L["agg"][L["indices"][L["indptr"][i]:L["indptr"][i + 1]]]
        a = a[a >= 0]
        assert list(idx[ptr[i]:ptr[i + 1]]) == list(dict.fromkeys(a.tolist()))


@pytest.mark.parametrize("name", SMALL)
def test_cycle_is_the_operator_of_explicit_matrices_symmetric_and_contracting(name):
    H = R.restated(name)
    n = H["levels"][0]["n"]
    M = R.cycle_matrix(H)
    b = np.random.default_rng(11).normal(size=(n, 6))
    x = R.cycle(H, b)
    assert np.abs(x - M @ b).max() <= 1e-12 * np.abs(x).max()
    assert np.abs(x - R.cycle(H, b, ap=True)).max() <= 1e-12 * np.abs(x).max()      # k_up_ap's form of the same step
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    B = R.csr(H["levels"][0]).toarray()
    G = np.linalg.cholesky(B)
    lam = np.linalg.eigvalsh(G.T @ (0.5 * (M + M.T)) @ G)                  # the spectrum of M B
    print(f"{name}: eigenvalues of M B in [{lam.min():.4f}, {lam.max():.12f}]")
    assert lam.min() > 0.0 and lam.max() <= 1.0 + 1e-12


@pytest.mark.parametrize("name", SMALL)
def test_fp32_cycle_stays_next_to_the_fp64_cycle(name):
    H = R.restated(name)
    b = R.right_hand_sides(H["levels"][0]["n"])
    for blk in b[[0, 12, 13]]:
        x64, d = R.d32(H, blk)
        assert 0.0 < d <= 1e-5 and np.isfinite(x64).all()
