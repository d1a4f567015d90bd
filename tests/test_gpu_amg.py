"""The multigrid hierarchy and V-cycle of pyqsm_amd/csrc/amg.hip, read out by ``hip.amg_probe``,
against the fp64 restatement of tests/amg_restatement.py (itself checked in tests/test_amg_host.py).

The cases (amg_restatement.CASES; "96" = PYQSM_AMG_DENSE_MAX=96): A / B forests of 1500 / 6000 points
(device inverse of 265 and 1009 rows, padded to 288 and 1024; host Cholesky below one and two middle
levels), C / D cliques whose second coarsening finds nothing (fused tail sweeps at 150 rows, launched
ones at 3100), E a level 1 most of whose rows have no aggregate, F the row cap stopping the second
coarsening (tail sweeps on a strongly connected level), G the cap stopping the first (no hierarchy).
Every test prints the figures it then asserts on.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from pyqsm_amd import hip
from tests import amg_restatement as R

pytestmark = pytest.mark.gpu

HIERARCHIES = ["A", "A96", "B", "B96", "C96", "D", "E", "F96"]
AP_MODES = ["ap", "no_ap"]                       # the default, and PYQSM_AMG_AP=0 (k_up instead of k_up_ap)


@contextlib.contextmanager
def _env(name, mode):
    want = {"PYQSM_AMG_DENSE_MAX": None if R.CASES[name][1] is None else str(R.CASES[name][1]),
            "PYQSM_AMG_AP": "0" if mode == "no_ap" else None}
    old = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _probe(name, mode, gpu):
    """One probe call per hierarchy and mode with the 14 right-hand sides; shared, not modified."""
    L, cw, wh = R.CASES[name][0]()
    with _env(name, mode):
        return hip.amg_probe(L, cw, wh, R.right_hand_sides(L.shape[0]), device=gpu)


@functools.lru_cache(maxsize=None)
def _restated_from_device(name, gpu):
    """The restatement started from the DEVICE's level-0 values."""
    l0 = _probe(name, "ap", gpu)["levels"][0]
    dmax = R.CASES[name][1]
    return R.build(l0["indptr"], l0["indices"], l0["vals"], R.DENSE_MAX if dmax is None else dmax)


@functools.lru_cache(maxsize=None)
def _reference_cycles(name, mode, gpu):
    """Per right-hand side block: (fp64 restated cycle, d32 of the upward step's form in this mode)."""
    H = _restated_from_device(name, gpu)
    return [R.d32(H, b, ap=mode == "ap") for b in R.right_hand_sides(H["levels"][0]["n"])]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("name", ["A", "B", "C96", "D", "E", "F96"])
def test_level0_is_cw_l_plus_wh(gpu, name):
    """k_make_b: off-diagonal values are cw_i L_ij bit for bit; the diagonal lies within 2 spacings of
    cw_i L_ii + wh_i (one rounding or two, should the compiler fuse the multiply-add)."""
    L, cw, wh = R.CASES[name][0]()
    l0 = _probe(name, "ap", gpu)["levels"][0]
    assert np.array_equal(l0["indptr"], L.indptr) and np.array_equal(l0["indices"], L.indices)
    r = R.rows_of(L.indptr)
    off = L.indices != r
    assert np.array_equal(_bits(l0["vals"][off]), _bits((cw[r] * L.data)[off]))
    want = cw[r] * L.data + wh[r]
    assert (np.abs(l0["vals"] - want)[~off] <= 2 * np.spacing(np.abs(want[~off]))).all()
    assert int((~off).sum()) == L.shape[0]


@pytest.mark.parametrize("mode", AP_MODES)
@pytest.mark.parametrize("name", HIERARCHIES)
def test_hierarchy_is_the_restatement_bit_for_bit(gpu, name, mode):
    """From the device's level-0 values the restatement reproduces every level: sizes, the stop rule's
    outcome, agg / mptr / members, the CSR pattern, the fp64 values and diag bit for bit; dinv to 1 ulp
    (a division). Coarse matrices are bitwise symmetric. The A P tables hold the distinct aggregates of
    a row in order of first occurrence with the fp32 sums in the kernel's order, bit for bit; with
    PYQSM_AMG_AP=0 there are none."""
    dev, H = _probe(name, mode, gpu), _restated_from_device(name, gpu)
    _, _, sizes, stop, coarse = R.CASES[name]
    assert dev["n_levels"] == len(sizes) and [l["n"] for l in dev["levels"]] == sizes
    assert [l["n"] for l in H["levels"]] == sizes and (H["stop"], H["coarse"]) == (stop, coarse)
    assert dev["coarse"] == coarse
    for l, (d, h) in enumerate(zip(dev["levels"], H["levels"])):
        assert np.array_equal(d["indptr"], h["indptr"]) and np.array_equal(d["indices"], h["indices"]), l
        assert np.array_equal(_bits(d["vals"]), _bits(h["vals"])), l
        assert np.array_equal(_bits(d["diag"]), _bits(h["diag"])), l
        assert (np.abs(d["dinv"] - h["dinv"]) <= np.spacing(h["dinv"])).all(), l
        if l > 0:
            A = R.csr(d)
            T = A.T.tocsr()
            T.sort_indices()
            assert np.array_equal(T.indices, A.indices) and np.array_equal(_bits(T.data), _bits(A.data)), l
        if l + 1 == len(sizes):
            assert d["agg"] is None and d["mptr"] is None and d["ap_ptr"] is None
            continue
        for k in ("agg", "mptr", "members"):
            assert np.array_equal(d[k], h[k]), (l, k)
        if mode == "no_ap":
            assert d["ap_ptr"] is None and d["ap_idx"] is None and d["ap_val"] is None
            continue
        ptr, idx, val = R.ap_table(d["indptr"], d["indices"], d["vals"], d["agg"])
        assert np.array_equal(d["ap_ptr"], ptr) and np.array_equal(d["ap_idx"], idx), l
        assert np.array_equal(_bits(d["ap_val"]), _bits(val)), l


@pytest.mark.parametrize("name", ["A", "B", "E", "A96", "B96"])
def test_dense_inverse_is_as_good_as_numpys(gpu, name):
    """max |A X - I| of the inverse the hierarchy carries (A, B, E: blocked Gauss-Jordan on the device
    with identity padding; A96, B96: host Cholesky) is at most 16 times that of np.linalg.inv of the same
    level's matrix (another summation order, nothing else), and X is symmetric to the same bound
    relative to max |X|.
    Measured on an MI355X, residual : NumPy's residual (both 2e-16 .. 6e-15): device-made A (265 rows) 0.71,
    B (1009 rows, 32 pivot blocks) 1.00, E (325 rows) 0.50; host-made A96 (53 rows) 1.62, B96 (25 rows) 1.15;
    asymmetry 2e-19 .. 2e-16 of max |X|."""
    dev = _probe(name, "ap", gpu)
    A = R.csr(dev["levels"][-1]).toarray()
    X = dev["inverse"]
    assert X.shape == A.shape and dev["coarse"] == R.CASES[name][4]
    eye = np.eye(len(A))
    res_np = np.abs(A @ np.linalg.inv(A) - eye).max()
    res = np.abs(A @ X - eye).max()
    asym = np.abs(X - X.T).max() / np.abs(X).max()
    print(f"{name} ({dev['coarse']}, {len(A)} rows): residual {res:.3e}, NumPy {res_np:.3e}, ratio {res / res_np:.2f}; "
          f"asymmetry {asym:.3e}")
    assert res <= 16 * res_np
    assert asym <= 16 * res_np


@pytest.mark.parametrize("mode", AP_MODES)
@pytest.mark.parametrize("name", HIERARCHIES)
def test_cycle_matches_the_fp64_restatement(gpu, name, mode):
    """Both interfaces (amg_vcycle on fp64 vectors, amg_vcycle_f32 on their fp32 roundings) lie within
    4 d32 of the restated fp64 cycle, where d32 = max |cycle_f32 - cycle_f64| / max |cycle_f64| of the
    restatement (its upward step in the form of the mode: k_up_ap's r - (A P) xc by default, k_up's b - A y
    with PYQSM_AMG_AP=0) is what fp32 rounding alone costs and the factor 4 covers the kernels' chunked and fused
    summation order; right-hand sides: twelve Gaussian blocks, one scaled by 1e-6, one by 1e6. The
    returned dot is sum b x of the returned x to n 2^-52 sum |b x|.
    Measured on an MI355X (worst block; d32 default / PYQSM_AMG_AP=0): A 1.16e-7 / 1.16e-7, A96 1.37e-7 /
    1.37e-7, B 7.3e-8 / 8.4e-8, B96 8.9e-8 / 1.24e-7, C96 2.17e-7 / 2.69e-7, D 2.29e-7 / 2.29e-7, E 1.96e-7 /
    1.87e-7, F96 1.80e-7 / 1.80e-7; the device's error was 1.00 d32 in every case and mode and for both
    interfaces: the kernels' sums come out as the restatement's sequential fp32 sums do. (Held against the
    k_up form of the restatement, the default mode's k_up_ap reached 6.6 d32 on one block of A96: the two forms
    round differently, which is why d32 takes the form of the mode.)"""
    dev, refs = _probe(name, mode, gpu), _reference_cycles(name, mode, gpu)
    rhs = R.right_hand_sides(dev["levels"][0]["n"])
    n = rhs.shape[1]
    worst = (0.0, 0.0, 0.0)
    for r, (x64, d32) in enumerate(refs):
        scale = np.abs(x64).max()
        e64 = np.abs(dev["x64"][r] - x64).max() / scale
        e32 = np.abs(dev["x32"][r].astype(np.float64) - x64).max() / scale
        worst = max(worst, (max(e64, e32) / d32, d32, max(e64, e32)))
        assert e64 <= 4 * d32 and e32 <= 4 * d32, (r, e64, e32, d32)
        for b, x, dot in ((rhs[r], dev["x64"][r], dev["dot64"][r]),
                          (rhs[r].astype(np.float32).astype(np.float64), dev["x32"][r].astype(np.float64), dev["dot32"][r])):
            p = b.astype(np.longdouble) * x.astype(np.longdouble)
            assert (np.abs(dot - p.sum(axis=0)) <= n * 2.0 ** -52 * np.abs(p).sum(axis=0)).all(), r
    print(f"{name} {mode}: worst block: device error {worst[2]:.3e} = {worst[0]:.2f} d32 (d32 {worst[1]:.3e})")


@pytest.mark.parametrize("name", ["A", "A96"])
def test_whole_operator_is_symmetric_and_contracting(gpu, name):
    """The 1500 unit vectors as 500 right-hand sides in one probe call: column by column M_dev agrees
    with the restated M within the cycle bound (4 d32 of that column), |M_dev - M_dev'| lies within twice
    that bound, and the eigenvalues of the symmetrised M_dev B lie in (0, 1 + bound].
    Measured on an MI355X (both interfaces alike): worst column error 0.25 of the bound (1.00 d32), asymmetry
    0.25 of its bound; eigenvalues in [0.0930, 1 + 6.8e-7] with bound 7.5e-7 (A) and [0.0794, 1 + 4.4e-7] with
    bound 8.7e-7 (A96)."""
    L, cw, wh = R.CASES[name][0]()
    n = L.shape[0]
    with _env(name, "ap"):
        dev = hip.amg_probe(L, cw, wh, np.eye(n).reshape(n, n // 3, 3).transpose(1, 0, 2), device=gpu)
    H = _restated_from_device(name, gpu)
    M64 = R.cycle(H, np.eye(n))
    M32 = R.cycle(H, np.eye(n, dtype=np.float32), np.float32, ap=True).astype(np.float64)
    colmax = np.abs(M64).max(axis=0)
    bound = 4 * np.abs(M32 - M64).max(axis=0)              # 4 d32 max |M[:, j]| per column j
    for key in ("x64", "x32"):
        Md = dev[key].astype(np.float64).transpose(1, 0, 2).reshape(n, n)
        err = np.abs(Md - M64).max(axis=0)
        asym = np.abs(Md - Md.T)
        B = R.csr(dev["levels"][0]).toarray()
        G = np.linalg.cholesky(B)
        lam = np.linalg.eigvalsh(G.T @ (0.5 * (Md + Md.T)) @ G)
        rel = float((bound / colmax).max())
        print(f"{name} {key}: worst column error / bound {float((err / bound).max()):.2f}, asymmetry / bound "
              f"{float((asym / (bound[None, :] + bound[:, None])).max()):.2f}, eigenvalues in [{lam.min():.4f}, "
              f"1 + {lam.max() - 1:.3e}], bound {rel:.3e}")
        assert (err <= bound).all()
        assert (asym <= bound[None, :] + bound[:, None]).all()
        assert lam.min() > 0.0 and lam.max() <= 1.0 + rel


def test_no_right_hand_side_returns_the_hierarchy_alone(gpu):
    L, cw, wh = R.CASES["A"][0]()
    with _env("A", "ap"):
        dev = hip.amg_probe(L, cw, wh, device=gpu)
    full = _probe("A", "ap", gpu)
    assert dev["n_levels"] == 2 and dev["x64"].shape == (0, 1500, 3) and dev["dot32"].shape == (0, 3)
    assert np.array_equal(dev["inverse"], full["inverse"])
    for d, f in zip(dev["levels"], full["levels"]):
        assert all(np.array_equal(d[k], f[k]) for k in d)


def test_row_cap_at_the_first_coarsening_leaves_no_hierarchy(gpu):
    """Case G: the probe reports one level and runs no cycle (the results keep their zeros)."""
    L, cw, wh = R.CASES["G"][0]()
    with _env("G", "ap"):
        dev = hip.amg_probe(L, cw, wh, R.right_hand_sides(L.shape[0])[:2], device=gpu)
    assert dev["n_levels"] == 1 and dev["levels"] == [] and dev["coarse"] is None
    assert "x64" not in dev
    assert R.restated("G")["stop"] == "cap"
