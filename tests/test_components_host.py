"""The ranked components of the radius graph without a GPU: the built library exports
pyqsm_radius_components with the header's argument list and answers what needs no device, and
geometry.density.Components selects what pyQSM's list-of-lists statement selects
(tests/density_restatement.py's components() are pinned to SciPy by tests/test_density_host.py)."""
import ctypes
from itertools import chain

import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry.density import Components
from tests import density_restatement as R
from tests.test_density_host import C_TYPES, _prototype

NAME = "pyqsm_radius_components"
EINVAL, ERANGE = -1, -4


def test_symbol_exported_with_the_headers_signature():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert NAME in _lib.SIGNATURES, f"{NAME} is not in _lib.SIGNATURES"
    assert hasattr(lib, NAME), f"{NAME} is not exported by {_lib.LIB_PATH}"
    proto = _prototype(NAME)
    assert proto == ["const double*", "int64_t", "const double*", "int32_t", "int32_t*", "int32_t*", "int32_t*",
                     "int64_t*", "int32_t"]
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == len(proto)
    for c_type, bound in zip(proto, args):
        if c_type.endswith("*"):
            assert bound is ctypes.c_void_p or issubclass(bound, ctypes._Pointer)
        else:
            assert bound is C_TYPES[c_type]


def test_empty_cloud_needs_no_device():
    E = np.zeros((0, 3))
    comp, sizes = hip.radius_components(E, [0.1, 0.2])
    assert comp.shape == (2, 0) and comp.dtype == np.int32
    assert [s.tolist() for s in sizes] == [[], []]
    comp, sizes, members = hip.radius_components(E, [0.1], members=True)
    assert members.shape == (1, 0) and len(sizes) == 1
    # the count is written, not left as it was
    count = np.full(2, -7, dtype=np.int64)
    radii = np.array([0.1, 0.2])
    assert _lib.load().pyqsm_radius_components(None, 0, hip._p(radii), 2, None, None, None, hip._p(count), 0) == 0
    assert count.tolist() == [0, 0]


def test_invalid_arguments():
    P = np.array([[0.0, 0, 0], [1, 0, 0]])

    def code(call):
        with pytest.raises(_lib.PyQSMHipError) as e:
            call()
        return e.value.code

    for r in (0.0, -1.0, np.inf, -np.inf, np.nan):
        assert code(lambda: hip.radius_components(P, [0.1, r])) == EINVAL
        assert code(lambda: hip.radius_components(P, r)) == EINVAL
    for bad_value in (np.nan, np.inf):
        bad = P.copy()
        bad[1, 2] = bad_value
        assert code(lambda: hip.radius_components(bad, [0.1])) == EINVAL
    assert code(lambda: hip.radius_components(P, [])) == ERANGE
    assert code(lambda: hip.radius_components(P, [0.1] * 9)) == ERANGE
    lib = _lib.load()
    radii, out, cnt = np.array([0.1]), np.zeros(4, np.int32), np.zeros(1, np.int64)
    p = hip._p
    assert lib.pyqsm_radius_components(p(P), -1, p(radii), 1, p(out), p(out), None, p(cnt), 0) == EINVAL
    # n of 2^31: refused before a coordinate is read
    assert lib.pyqsm_radius_components(p(P), 1 << 31, p(radii), 1, p(out), p(out), None, p(cnt), 0) == ERANGE
    # NULL pointers (members alone may be NULL)
    assert lib.pyqsm_radius_components(None, 2, p(radii), 1, p(out), p(out), None, p(cnt), 0) == EINVAL
    assert lib.pyqsm_radius_components(p(P), 2, None, 1, p(out), p(out), None, p(cnt), 0) == EINVAL
    assert lib.pyqsm_radius_components(p(P), 2, p(radii), 1, None, p(out), None, p(cnt), 0) == EINVAL
    assert lib.pyqsm_radius_components(p(P), 2, p(radii), 1, p(out), None, None, p(cnt), 0) == EINVAL
    assert lib.pyqsm_radius_components(p(P), 2, p(radii), 1, p(out), p(out), None, None, 0) == EINVAL
    assert lib.pyqsm_radius_components(p(P), 2, p(radii), 0, p(out), p(out), None, p(cnt), 0) == ERANGE


# ---- Components against pyQSM's statement ---------------------------------------------------------

def conn_comps(component, sizes):
    """sorted(connected_components(g), key=len, reverse=True) as lists of point indices, ties by
    smallest member."""
    out = [np.flatnonzero(component == k).tolist() for k in range(len(sizes))]
    assert [len(x) for x in out] == list(sizes)
    return out


def pyqsm_select(cc, top, min_size, max_size):
    lo = -np.inf if min_size is None else min_size
    hi = np.inf if max_size is None else max_size
    return list(chain.from_iterable(x for x in cc[0:top] if lo < len(x) < hi))


@pytest.fixture(scope="module", params=["small", "uniform"])
def family(request):
    P, r = R.small_components() if request.param == "small" else (R.uniform(20000), 0.032)
    comp, sizes = R.components(P, r)
    return comp, sizes, conn_comps(comp, sizes)


def test_members(family):
    comp, sizes, cc = family
    for c in (Components(comp, sizes), Components(comp, sizes, np.lexsort((np.arange(len(comp)), comp)))):
        assert len(c) == len(cc)
        for k in list(range(min(40, len(cc)))) + [len(cc) - 1]:
            assert c.members(k).tolist() == cc[k]
        for bad in (-1, len(cc)):
            with pytest.raises(IndexError):
                c.members(bad)


def test_select(family):
    comp, sizes, cc = family
    c = Components(comp, sizes)
    big = int(sizes[0])
    cases = [(None, None, None), (500, 100, None), (500, None, 100), (100, None, None), (3, None, None),
             (0, None, None), (len(cc) + 5, 1, 3), (None, 1, None), (None, 2, 3), (None, big, None),
             (None, big - 1, None), (None, None, 2), (None, None, 1), (7, 0, big), (7, 0, big + 1)]
    for top, lo, hi in cases:
        got = c.select(top=top, min_size=lo, max_size=hi)
        assert got.tolist() == pyqsm_select(cc, top, lo, hi), (top, lo, hi)
    assert c.select(top=500, min_size=100).dtype.kind == "i"


def test_select_is_strict_on_both_bounds():
    P, r = R.small_components()
    comp, sizes = R.components(P, r)
    c = Components(comp, sizes)
    assert sizes.tolist() == [3] * 128 + [2] * 128 + [1] * 128
    assert len(c.select(min_size=3)) == 0 and len(c.select(min_size=2)) == 3 * 128
    assert len(c.select(max_size=1)) == 0 and len(c.select(max_size=2)) == 128
    assert len(c.select(min_size=1, max_size=3)) == 2 * 128
    assert len(c.select(top=130, min_size=1, max_size=3)) == 2 * 2
