"""The radius graph without a GPU: the CPU statement of the contract (tests/density_restatement.py)
equals SciPy's cKDTree on the point families the GPU tests use, the built library exports the two
entry points with the header's signatures and answers what needs no device, and get_pairs keeps
pyQSM's return shape."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

from pyqsm_amd import _lib, hip
from tests import density_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pyqsm_radius_degrees", "pyqsm_radius_pairs")


def scipy_pairs(P, r):
    p = np.sort(cKDTree(P).query_pairs(r, output_type="ndarray"), 1)
    return p[np.lexsort((p[:, 1], p[:, 0]))].astype(np.int32).reshape(-1, 2)


def scipy_degrees(P, r):
    return (cKDTree(P).query_ball_point(P, r, return_length=True) - 1).astype(np.int32)


def scipy_components(P, r):
    p = scipy_pairs(P, r)
    g = coo_matrix((np.ones(len(p), dtype=np.int8), (p[:, 0], p[:, 1])), shape=(len(P), len(P)))
    return connected_components(g, directed=False)


def check_against_scipy(P, r, n_pairs=None):
    p = R.pairs(P, r)
    assert np.array_equal(p, scipy_pairs(P, r))
    if n_pairs is not None:
        assert len(p) == n_pairs
    deg, cnt = R.degrees(P, [r])
    assert np.array_equal(deg[0], scipy_degrees(P, r))
    assert np.array_equal(deg[0], np.bincount(p.ravel(), minlength=len(P)))
    assert cnt[0] == len(p)
    return p


def test_two_points_on_the_bound():
    P = np.array([[0, 0, 0], [3, 4, 0]], dtype=np.float64) / 64
    assert len(check_against_scipy(P, 5 / 64)) == 1
    assert len(check_against_scipy(P, np.nextafter(5 / 64, 0))) == 0


@pytest.mark.parametrize("r,n_pairs", list(zip(R.LATTICE_RADII, R.LATTICE_PAIRS)))
def test_lattice(r, n_pairs):
    L = R.lattice()
    check_against_scipy(L, r, n_pairs)
    if r == 3 / 64:
        assert R.degrees(L, [r])[0].max() == 122      # an interior point; ties at d2 = 9/4096


def test_lattice_radii_in_one_call():
    L = R.lattice()
    radii = [R.LATTICE_RADII[k] for k in (2, 0, 3, 1, 0)]
    deg, cnt = R.degrees(L, radii)
    for k, r in enumerate(radii):
        assert np.array_equal(deg[k], scipy_degrees(L, r))
    assert cnt.tolist() == [33120, 199572, 33120, 11520, 199572]


@pytest.mark.parametrize("n,r", [(3000, 0.05), (20000, 0.03)])
def test_uniform(n, r):
    check_against_scipy(R.uniform(n), r)


def test_fp32_valued():
    check_against_scipy(R.fp32_valued(), 0.3)


def test_chain():
    C, h = R.chain(), 2.0 ** -5
    p = check_against_scipy(C, h, 1999)
    comp, sizes = R.components(C, h, p)
    assert sizes.tolist() == [2000] and not comp.any()
    assert len(check_against_scipy(C, np.nextafter(h, 0), 0)) == 0
    comp, sizes = R.components(C, np.nextafter(h, 0))
    assert sizes.tolist() == [1] * 2000 and np.array_equal(comp, np.arange(2000))   # ties: smallest member


def test_components_against_scipy_and_ranking():
    P, r = R.small_components()
    comp, sizes = R.components(P, r)
    nc, lab = scipy_components(P, r)
    assert len(sizes) == nc and sizes.sum() == len(P)
    assert sorted(set(sizes.tolist())) == [1, 2, 3]
    # the same partition, sizes descending, ties by smallest member ascending
    assert len(set(zip(comp.tolist(), lab.tolist()))) == nc
    assert np.all(np.diff(sizes) <= 0)
    firsts = np.array([np.flatnonzero(comp == k)[0] for k in range(nc)])
    for s in (1, 2, 3):
        assert np.all(np.diff(firsts[sizes == s]) > 0)
    assert np.array_equal(np.bincount(comp), sizes)


# ---- the built library ------------------------------------------------------------------------

C_TYPES = {"double": ctypes.c_double, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}


def _prototype(name):
    text = open(os.path.join(ROOT, "include", "pyqsm_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/pyqsm_hip.h"
    return [" ".join(a.split()[:-1]) + ("*" if a.split()[-1].startswith("*") else "") for a in m.group(1).split(",")]


def test_symbols_exported_with_the_headers_signatures():
    expected = {
        "pyqsm_radius_degrees": ["const double*", "int64_t", "const double*", "int32_t", "int32_t*", "int64_t*",
                                 "int64_t*", "int32_t"],
        "pyqsm_radius_pairs": ["const double*", "int64_t", "double", "int64_t", "int32_t*", "int64_t*", "int32_t"],
    }
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
        proto = _prototype(name)
        assert proto == expected[name]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(proto)
        for c_type, bound in zip(proto, args):
            if c_type.endswith("*"):
                assert bound is ctypes.c_void_p or issubclass(bound, ctypes._Pointer)
            else:
                assert bound is C_TYPES[c_type]


def test_empty_cloud_needs_no_device():
    E = np.zeros((0, 3))
    deg, cnt = hip.radius_degrees(E, [0.1, 0.2])
    assert deg.shape == (2, 0) and cnt.tolist() == [0, 0]
    assert hip.radius_pairs(E, 0.1).shape == (0, 2)


def test_invalid_arguments():
    P = np.array([[0.0, 0, 0], [1, 0, 0]])
    bad = P.copy()
    bad[1, 2] = np.nan

    def code(call):
        with pytest.raises(_lib.PyQSMHipError) as e:
            call()
        return e.value.code

    EINVAL, ERANGE = -1, -4
    lib = _lib.load()
    for r in (0.0, -1.0, np.inf, np.nan):
        assert code(lambda: hip.radius_degrees(P, [0.1, r])) == EINVAL
        assert code(lambda: hip.radius_pairs(P, r)) == EINVAL
    assert code(lambda: hip.radius_degrees(bad, [0.1])) == EINVAL
    assert code(lambda: hip.radius_pairs(bad, 0.1)) == EINVAL
    assert code(lambda: hip.radius_degrees(P, [])) == ERANGE
    assert code(lambda: hip.radius_degrees(P, [0.1] * 9)) == ERANGE
    # n of 2^31: refused before a coordinate is read
    radii, out, cnt = np.array([0.1]), np.zeros(4, np.int32), ctypes.c_int64(0)
    big = 1 << 31
    assert lib.pyqsm_radius_degrees(hip._p(P), big, hip._p(radii), 1, hip._p(out), hip._p(np.zeros(1, np.int64)), None,
                                    0) == ERANGE
    assert lib.pyqsm_radius_pairs(hip._p(P), big, 0.1, 1, hip._p(out), ctypes.byref(cnt), 0) == ERANGE
    # NULL pointers
    assert lib.pyqsm_radius_degrees(None, 2, hip._p(radii), 1, hip._p(out), hip._p(np.zeros(1, np.int64)), None,
                                    0) == EINVAL
    assert lib.pyqsm_radius_degrees(hip._p(P), 2, None, 1, hip._p(out), hip._p(np.zeros(1, np.int64)), None, 0) == EINVAL
    assert lib.pyqsm_radius_pairs(hip._p(P), 2, 0.1, 1, None, ctypes.byref(cnt), 0) == EINVAL
    assert lib.pyqsm_radius_pairs(hip._p(P), 2, 0.1, 1, hip._p(out), None, 0) == EINVAL


def test_get_pairs_return_shape(monkeypatch):
    """pyQSM's (degrees, cnts, line_set): the degrees from the counting call, the pair list fetched only
    for the line set (the device calls are replaced by the restatement here)."""
    from pyqsm_amd.geometry.skeletonize import LineSet
    from pyqsm_amd.utils import lib_integration as li
    P = R.uniform(400, seed=9)
    calls = []

    def fake_degrees(pts, radii, device=0, stats=None):
        calls.append("degrees")
        return R.degrees(pts, radii)

    def fake_pairs(pts, radius, n_pairs=None, device=0):
        calls.append("pairs")
        p = R.pairs(pts, radius)
        assert n_pairs == len(p)
        return p

    monkeypatch.setattr(hip, "radius_degrees", fake_degrees)
    monkeypatch.setattr(hip, "radius_pairs", fake_pairs)
    deg0, cnts0, pairs0 = R.get_pairs(P, 0.15)
    degrees, cnts, line_set = li.get_pairs(query_pts=P, radius=0.15)
    assert calls == ["degrees"] and line_set is None
    assert len(degrees) == len(P) and np.array_equal(degrees, deg0) and np.array_equal(cnts, cnts0)
    assert cnts.sum() == len(P)
    degrees, cnts, line_set = li.get_pairs(kd_tree=cKDTree(P), radius=0.15, return_line_set=True)
    assert calls == ["degrees", "degrees", "pairs"]
    assert isinstance(line_set, LineSet) and np.array_equal(line_set.points, P)
    assert np.array_equal(line_set.lines, pairs0) and np.array_equal(degrees, deg0)
    with pytest.raises(ValueError):
        li.get_pairs()
