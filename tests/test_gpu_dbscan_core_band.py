"""DBSCAN's core pass decides its pairs in fp32 where the grid keeps fp32 records (dbscan.hip, core_band):
a pair counts when its fp32 squared distance is <= lo, does not when it is > hi, and only a point whose
verdict hangs on a distance between the two (the band, 2^-20 of eps^2 to either side) is left to the fp64
pass. The clouds here put distances into that band on purpose: shells at exactly eps, lattices whose spacing
is eps, a coarse fp32 grid with many equal distances, millimetre-quantised scans; and they leave the fp32
decision altogether (eps too small or too large for fp32). Labels and core flags are compared with the CPU
oracle for exact equality, under both radius rules."""
import numpy as np
import pytest

import oracle
from pyqsm_amd import hip, synth

pytestmark = pytest.mark.gpu


def _f32(P):
    return np.ascontiguousarray(P, dtype=np.float64).astype(np.float32).astype(np.float64)


def _check(P, eps, min_pts, gpu, rules=(True, False)):
    """Both radius rules against the oracle; the core flags of the inclusive rule (of the first rule asked for)."""
    first = None
    for inclusive in rules:
        lab0, core0 = oracle.dbscan(P, eps, min_pts, radius_inclusive=inclusive)
        lab, core = hip.dbscan(P, eps, min_pts, device=gpu, radius_inclusive=inclusive)
        assert np.array_equal(core, core0), f"core flags, radius_inclusive={inclusive}"
        assert np.array_equal(lab, lab0), f"labels, radius_inclusive={inclusive}"
        if first is None:
            first = core0
    return first


def _band_lanes(P, eps, min_pts, gpu, inclusive=True):
    """core_band_lanes of one call at profiling level 2 (the call's result is checked as well)."""
    hip.prof_enable(2, gpu)
    try:
        hip.prof_reset(gpu)
        lab, core = hip.dbscan(P, eps, min_pts, device=gpu, radius_inclusive=inclusive)
        lanes = hip.prof_get("core_band_lanes", gpu)[1]
        tests = hip.prof_get("core_pair_tests", gpu)[1]
    finally:
        hip.prof_enable(False, gpu)
    lab0, core0 = oracle.dbscan(P, eps, min_pts, radius_inclusive=inclusive)
    assert np.array_equal(core, core0) and np.array_equal(lab, lab0)
    assert tests > 0
    return lanes


def _thresholds(eps):
    """(lo, hi) as float32: the largest float <= r2 (1 - 2^-20), the smallest float >= r2 (1 + 2^-20)."""
    r2 = eps * eps
    a, b = r2 * (1.0 - 2.0 ** -20), r2 * (1.0 + 2.0 ** -20)
    lo, hi = np.float32(a), np.float32(b)
    if float(lo) > a:
        lo = np.nextafter(lo, np.float32(-np.inf))
    if float(hi) < b:
        hi = np.nextafter(hi, np.float32(np.inf))
    return lo, hi


def _d2_f32(A, B):
    """The kernel's fp32 chain for the pairs (A[i], B[i]) of fp32-exact points: rounded differences, one
    rounded product, two fused multiply-adds (a product of two floats is exact in fp64, and the sum of
    two such terms rounds to float from fp64 as it would from the exact value but for a vanishing share of
    double roundings, which moves no count here by more than a few pairs)."""
    a, b = A.astype(np.float32), B.astype(np.float32)
    d = (a - b).astype(np.float32).astype(np.float64)
    s = np.float32(d[:, 0] * d[:, 0])
    s = np.float32(d[:, 1] * d[:, 1] + np.float64(s))
    s = np.float32(d[:, 2] * d[:, 2] + np.float64(s))
    return s


def _d2_f64(A, B):
    d = A - B
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


# ---- shells at eps -------------------------------------------------------------------------------

def _shells(eps, min_pts, centres=200, shell=24, seed=0):
    """Centres in a 2 m box; `shell` points at distance eps from each, in random directions, and
    min_pts - 1 - j fillers at 0.3 eps (j = centre index mod min_pts): with itself and its fillers a centre
    has min_pts - j neighbours for certain and is core iff at least j of its shell points are within.
    Returns the cloud (fp32 values), and the index pairs (centre, shell point)."""
    rng = np.random.default_rng(seed)
    C = _f32(rng.uniform(0.0, 2.0, (centres, 3)))
    pts, pairs = [C], []
    n = centres
    for i in range(centres):
        d = rng.normal(size=(shell, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        S = _f32(C[i] + eps * d)
        pairs.append(np.stack([np.full(shell, i), n + np.arange(shell)], 1))
        pts.append(S)
        n += shell
        k = min_pts - 1 - i % min_pts
        d = rng.normal(size=(k, 3))
        d /= np.linalg.norm(d, axis=1)[:, None]
        pts.append(_f32(C[i] + 0.3 * eps * d))
        n += k
    return np.concatenate(pts), np.concatenate(pairs)


@pytest.mark.parametrize("seed", [0, 1])
def test_shells_at_eps(gpu, seed):
    eps, min_pts = 0.1, 25
    P, pairs = _shells(eps, min_pts, seed=seed)
    # the case proves something only if many shell pairs are left to fp64, with verdicts of both kinds
    lo, hi = _thresholds(eps)
    d32 = _d2_f32(P[pairs[:, 0]], P[pairs[:, 1]])
    d64 = _d2_f64(P[pairs[:, 0]], P[pairs[:, 1]])
    in_band = (d32 > lo) & (d32 <= hi)
    assert (in_band & (d64 <= eps * eps)).sum() >= 100
    assert (in_band & (d64 > eps * eps)).sum() >= 100
    # ... and no pair outside the band is decided wrongly by the emulated chain
    assert not ((d32 <= lo) & (d64 > eps * eps)).any() and not ((d32 > hi) & (d64 <= eps * eps)).any()
    perm = np.random.default_rng(seed + 10).permutation(P.shape[0])
    core0 = _check(P[perm], eps, min_pts, gpu)
    centre_core = core0[np.argsort(perm)][:200]
    assert 20 <= centre_core.sum() <= 180       # the centres' flags do hinge on the shells


# ---- lattices whose spacing is eps ---------------------------------------------------------------

def _lattice(side, pitch):
    return np.stack(np.meshgrid(*[np.arange(side) * pitch] * 3, indexing="ij"), -1).reshape(-1, 3)


@pytest.mark.parametrize("side", [17, 41])
@pytest.mark.parametrize("min_pts", [7, 8])
def test_lattice_spacing_equal_to_eps(gpu, side, min_pts):
    # The six face neighbours are at exactly eps: with itself an interior point has 7 neighbours under the
    # inclusive rule and 1 under the strict one, and every one of these distances lies in the band: fp32
    # decides no point of the cloud, all of it goes through the straggler list (its capacity) and fp64.
    eps = 0.125
    P = _lattice(side, eps)
    assert np.array_equal(_f32(P), P)
    core0 = _check(P, eps, min_pts, gpu)
    assert core0.sum() == ((side - 2) ** 3 if min_pts == 7 else 0)
    assert _band_lanes(P, eps, min_pts, gpu) > 0
    Q = P[np.random.default_rng(side).permutation(P.shape[0])]
    _check(Q, eps, min_pts, gpu)


@pytest.mark.parametrize("side", [4, 5, 6])
@pytest.mark.parametrize("min_pts", [4, 5, 7])
def test_small_lattice_ends_its_tile(gpu, side, min_pts):
    # A wave of the large lattices hands its lanes on after a few chunks, short of everything. Here a tile is
    # one to four chunks: the waves see all of it, through the last chunk or through empty trailing runs, and
    # lanes that straddle then (a corner has 4 neighbours within hi and 1 within lo, an edge 5, a face 6, an
    # interior point 7) must still reach the fp64 pass: decided there and then they would all be non-core.
    eps = 0.125
    P = _lattice(side, eps)
    core0 = _check(P, eps, min_pts, gpu)
    assert core0.sum() == {4: side ** 3, 5: side ** 3 - 8, 7: (side - 2) ** 3}[min_pts]
    assert _band_lanes(P, eps, min_pts, gpu) > 0


# ---- many exactly equal distances ----------------------------------------------------------------

def test_coarse_fp32_grid(gpu):
    # at 4096 the fp32 ulp is 4.9e-4: the coordinates lie on a lattice of that pitch
    rng = np.random.default_rng(5)
    P = _f32(rng.uniform(0.0, 3.0, (50_000, 3)) + 4096.0)
    core0 = _check(P, 0.1, 8, gpu)
    assert 0.2 < core0.mean() < 0.8


def test_mm_quantised_forest(gpu):
    P = _f32(np.round(synth.forest(100_000), 3))
    core0 = _check(P, 0.1, 10, gpu)
    assert core0.any() and not core0.all()


# ---- outside the fp32 decision ---------------------------------------------------------------------

def test_eps_too_small_and_too_large_for_fp32(gpu):
    rng = np.random.default_rng(8)
    U = rng.uniform(0.0, 6.0, (100, 3))
    eps = 2.0 ** -51                                  # eps^2 = 2^-102 <= 2^-100: lo is not above 2^-100
    assert float(_thresholds(eps)[0]) <= 2.0 ** -100
    P = _f32(U * eps)
    core0 = _check(P, eps, 3, gpu)
    assert core0.any() and not core0.all()
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.float32(1e20 * 1e20))   # eps = 1e20: hi is not finite
    core0 = _check(_f32(U), 1e20, 3, gpu)
    assert core0.all()
    assert _band_lanes(_f32(U), 1e20, 3, gpu) == 0


# ---- smooth data stays on the fast path ------------------------------------------------------------

def test_smooth_data_stays_in_fp32(gpu):
    n = 200_000
    P = synth.forest(n)
    assert np.array_equal(_f32(P), P)                 # fp32 records
    assert _band_lanes(P, 0.1, 10, gpu) <= n // 1000
    assert _band_lanes(P, 0.1, 10, gpu, inclusive=False) <= n // 1000
