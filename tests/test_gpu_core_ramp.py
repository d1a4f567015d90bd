"""DBSCAN's core pass counts with two clamped fp32 ramps (dbscan.hip, core_ramp; the constants are
tests/test_core_ramp_constants.py's subject). Here: the device's ramp function, bit for bit against the
emulation (the clamp modifier on a packed fp32 fma is taken on trust nowhere else), and whole clusterings
against the CPU oracle under both radius rules on clouds that aim at the counting: the padding candidate of
an odd count and the wave edges, large and integer-valued sums, distances in the zone where the ramps give
fractions and just outside it, and the two ways out of the ramp form (fp64 records, min_pts above 2^20)."""
import numpy as np
import pytest

import oracle
from pyqsm_amd import hip
from tests import core_ramp_cases as C

pytestmark = pytest.mark.gpu

F32 = np.float32
RULES = (True, False)


def _f32(P):
    return np.ascontiguousarray(P, dtype=np.float64).astype(np.float32).astype(np.float64)


def _check(P, eps, min_pts, gpu):
    """Both radius rules against the oracle; the inclusive rule's core flags."""
    first = None
    for inclusive in RULES:
        lab0, core0 = oracle.dbscan(P, eps, min_pts, radius_inclusive=inclusive)
        lab, core = hip.dbscan(P, eps, min_pts, device=gpu, radius_inclusive=inclusive)
        assert np.array_equal(core, core0), f"core flags, radius_inclusive={inclusive}"
        assert np.array_equal(lab, lab0), f"labels, radius_inclusive={inclusive}"
        if first is None:
            first = core0
    return first


# ---- the ramp function on the device ---------------------------------------------------------------

def _extra(c):
    """0, +inf, far outside on both sides, the format's ends and sub-normal distances."""
    with np.errstate(over="ignore"):
        far = np.array([0.0, np.inf, float(c.lo) / 2, float(c.hi) * 2, float(c.hi) * 1e6, float(c.lo) * 1e-6],
                       dtype=np.float64).astype(np.float32)
    ends = np.array([np.finfo(F32).max, np.finfo(F32).tiny], dtype=np.float32)
    sub = np.array([1, 2, 0x7FFFFF, 0x400000], dtype=np.int32).view(np.float32)
    return np.concatenate([far, ends, sub])


@pytest.mark.parametrize("inclusive", RULES)
def test_probe_equals_emulation(gpu, inclusive):
    for eps in C.eps_values():
        c = hip.core_ramp_constants(eps, inclusive)
        d = np.concatenate([C.probe_distances(eps, inclusive), _extra(c)])
        assert d.size % 2 == 0
        for dd in (d, d[:-1]):                       # (an odd count: the last pair is padded)
            s_in, s_hi = hip.core_ramp_probe(dd, eps, inclusive, device=gpu)
            e_in, e_hi = C.ramp(dd, float(c.K), float(c.A)), C.ramp(dd, float(c.K), float(c.B))
            assert np.array_equal(s_in.view(np.int32), e_in.view(np.int32)), (eps, "s_in")
            assert np.array_equal(s_hi.view(np.int32), e_hi.view(np.int32)), (eps, "s_hi")


def test_probe_refuses_an_eps_without_ramps(gpu):
    with pytest.raises(hip._lib.PyQSMHipError):
        hip.core_ramp_probe(np.zeros(2, dtype=np.float32), 1e20, device=gpu)


# ---- tiny clouds: the padding candidate, the wave edges --------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129])
@pytest.mark.parametrize("min_pts", [1, 3])
def test_tiny_clouds(gpu, n, min_pts):
    P = _f32(np.random.default_rng(n).uniform(0.0, 0.3, (n, 3)))
    core0 = _check(P, 0.1, min_pts, gpu)
    if min_pts == 1:
        assert core0.all()


# ---- a dense blob: more chunks per wave, large sums --------------------------------------------------

BLOB = _f32(np.random.default_rng(3).normal(0.0, 0.12, (4000, 3)))


@pytest.mark.parametrize("min_pts", [1, 2, 64, 300])
def test_dense_blob(gpu, min_pts):
    core0 = _check(BLOB, 0.1, min_pts, gpu)
    if min_pts == 300:
        assert 0.05 < core0.mean() < 0.95             # the verdicts do hinge on counts near 300
    if min_pts == 1:
        assert core0.all()


# ---- integer-valued sums ---------------------------------------------------------------------------

@pytest.mark.parametrize("min_pts", [2, 5, 64, 200])
def test_groups_of_exactly_min_pts_and_one_fewer(gpu, min_pts):
    # Groups three eps apart, every point of a group within 0.25 eps of its centre: all of a group's distances
    # are at most 0.5 eps, where both ramps give exactly 1, and a point has exactly as many neighbours as its
    # group has points: min_pts (core) in the even groups, min_pts - 1 (not core) in the odd ones.
    eps = 0.1
    rng = np.random.default_rng(min_pts)
    side = 4
    pts, want = [], []
    for g in range(side ** 3):
        k = min_pts - g % 2
        centre = 3 * eps * np.array([g % side, g // side % side, g // side ** 2], dtype=np.float64)
        v = rng.normal(size=(k, 3))
        v *= (0.25 * eps * rng.uniform(0.0, 1.0, (k, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1)[:, None]
        pts.append(centre + v)
        want.append(np.full(k, g % 2 == 0))
    P, want = _f32(np.concatenate(pts)), np.concatenate(want)
    perm = rng.permutation(len(P))
    core0 = _check(P[perm], eps, min_pts, gpu)
    assert np.array_equal(core0, want[perm])


# ---- shells inside and just outside the zone of fractions ------------------------------------------

def _d2_f32(A, B):
    """The kernel's fp32 chain for the pairs (A[i], B[i]) (tests/test_gpu_dbscan_core_band.py)."""
    a, b = A.astype(np.float32), B.astype(np.float32)
    d = (a - b).astype(np.float32).astype(np.float64)
    s = np.float32(d[:, 0] * d[:, 0])
    s = np.float32(d[:, 1] * d[:, 1] + np.float64(s))
    s = np.float32(d[:, 2] * d[:, 2] + np.float64(s))
    return s


def _zones(d32, c):
    """Where a fp32 squared distance falls: 0 within and counted as 1, 1 within and counted as a fraction of
    acc_in (lo - 1/K, lo], 2 the band (lo, hi], 3 without and counted as a fraction of acc_hi (hi, hi + 1/K),
    4 without and counted as 0."""
    d, w = d32.astype(np.float64), 1.0 / float(c.K)
    return np.searchsorted([float(c.lo) - w, float(c.lo), float(c.hi)], d, side="left") + (d >= float(c.hi) + w)


def _shells(eps, min_pts, zones, centres=200, shell=24, seed=0):
    """Centres in a 2 m box; around each, `shell` points at about eps, and min_pts - 1 - j fillers at 0.3 eps
    (j = centre index mod min_pts): a centre is core iff at least j of its shell points are within. Rounding
    to fp32 moves a squared distance by several 2^-20 of eps^2 here, so the shell points are chosen among
    400 drawn within eps^2 (1 +- 8 * 2^-20), by the kernel's fp32 chain: as many from each of `zones`
    (_zones; 0 and 4 no further than 6 * 2^-20). Returns the cloud and the index pairs (centre, shell point)."""
    c = hip.core_ramp_constants(eps)
    rng = np.random.default_rng(seed)
    Cn = _f32(rng.uniform(0.0, 2.0, (centres, 3)))
    pts, pairs = [Cn], []
    n = centres
    for i in range(centres):
        d = rng.normal(size=(400, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        rad = eps * np.sqrt(1.0 + rng.uniform(-8.0, 8.0, 400) * 2.0 ** -20)
        S = _f32(Cn[i] + rad[:, None] * d)
        d32 = _d2_f32(np.broadcast_to(Cn[i], S.shape), S)
        z = _zones(d32, c)
        near = np.abs(d32.astype(np.float64) / (eps * eps) - 1.0) < 6.0 * 2.0 ** -20
        pick = np.concatenate([np.flatnonzero((z == k) & near)[: shell // len(zones)] for k in zones])
        assert pick.size == shell
        pts.append(S[pick])
        pairs.append(np.stack([np.full(shell, i), n + np.arange(shell)], 1))
        n += shell
        k = min_pts - 1 - i % min_pts
        d = rng.normal(size=(k, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        pts.append(_f32(Cn[i] + 0.3 * eps * d))
        n += k
    return np.concatenate(pts), np.concatenate(pairs)


@pytest.mark.parametrize("zones", [(1, 3), (0, 4), (0, 1, 3, 4), (0, 1, 2, 3)])
def test_shells_around_the_zone(gpu, zones):
    # shells inside the zone where the ramps give fractions (about eps^2 (1 +- 2 * 2^-20)), just outside it
    # (about eps^2 (1 +- 4 * 2^-20)), both, and with the band
    eps, min_pts = 0.1, 25
    P, pairs = _shells(eps, min_pts, zones, seed=len(zones) + zones[0])
    z = _zones(_d2_f32(P[pairs[:, 0]], P[pairs[:, 1]]), hip.core_ramp_constants(eps))
    assert all((z == k).sum() == len(z) // len(zones) for k in zones)
    perm = np.random.default_rng(7).permutation(P.shape[0])
    core0 = _check(P[perm], eps, min_pts, gpu)
    centre_core = core0[np.argsort(perm)][:200]
    assert 20 <= centre_core.sum() <= 180             # the centres' flags do hinge on the shells


# ---- outside the ramp form: the fp64 kernel ----------------------------------------------------------

def _band_lanes(P, eps, min_pts, gpu):
    hip.prof_enable(2, gpu)
    try:
        hip.prof_reset(gpu)
        lab, core = hip.dbscan(P, eps, min_pts, device=gpu)
        lanes = hip.prof_get("core_band_lanes", gpu)[1]
    finally:
        hip.prof_enable(False, gpu)
    return lab, core, lanes


def test_fp64_records(gpu, monkeypatch):
    monkeypatch.setenv("PYQSM_COORD_F32", "0")
    P, _ = _shells(0.1, 25, (1, 2, 3), centres=40)
    _check(P, 0.1, 25, gpu)
    _check(BLOB, 0.1, 64, gpu)


def test_min_pts_above_two_to_the_twenty(gpu):
    # 2^20 + 1 is still a float, but the ramp form is not taken there: no lane is ever handed on for the band
    P = _f32(np.random.default_rng(9).uniform(0.0, 0.3, (300, 3)))
    min_pts = 2 ** 20 + 1
    core0 = _check(P, 0.1, min_pts, gpu)
    assert not core0.any()
    lab, core, lanes = _band_lanes(P, 0.1, min_pts, gpu)
    assert lanes == 0 and not core.any() and (lab == -1).all()
    _check(P, 0.1, 2 ** 20, gpu)                      # (2^20 itself: the ramp form)
