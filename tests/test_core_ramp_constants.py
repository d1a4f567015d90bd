"""The constants of the two clamped ramps DBSCAN's core pass counts with (dbscan.hip, core_ramp), as
pyqsm_core_ramp_constants reports them; no GPU. With d a pair's fp32 squared distance,
    s_in = sat(fma(d, -K, A)),    s_hi = sat(fma(d, -K, B)),
K a power of two with 1/K in [r2 2^-20, r2 2^-19), A the largest float <= K lo, B the smallest float
>= 1 + K hi, and lo, hi the thresholds of the fp32 decision. What the kernel's counting relies on:
s_in > 0 only where d <= lo, s_hi == 1 wherever d <= hi. The ramps are emulated in float64 and rounded
once to float32, which is what the fma does: K d is exact (a power of two), and near the thresholds the
difference of two values of this size is exact in a double."""
import numpy as np
import pytest

from pyqsm_amd import hip
from tests.core_ramp_cases import eps_values, probe_distances, r2_of, ramp

F32 = np.float32


def check_constants(eps, inclusive):
    r2 = r2_of(eps, inclusive)
    c = hip.core_ramp_constants(eps, inclusive)
    assert c.usable, (eps, inclusive)
    lo, hi, K, A, B = (float(v) for v in c[:5])
    # lo, hi: the largest float <= r2 (1 - 2^-20), the smallest float >= r2 (1 + 2^-20)
    a, b = r2 * (1.0 - 2.0 ** -20), r2 * (1.0 + 2.0 ** -20)
    assert lo <= a < float(np.nextafter(c.lo, F32(np.inf)))
    assert float(np.nextafter(c.hi, F32(-np.inf))) < b <= hi
    # K: a power of two, 1/K in [r2 2^-20, r2 2^-19)
    assert np.frexp(K)[0] == 0.5
    assert r2 * 2.0 ** -20 <= 1.0 / K < r2 * 2.0 ** -19
    # A: the largest float <= K lo; B: the smallest float >= 1 + K hi (both products and the sum exact)
    assert A <= K * lo < float(np.nextafter(c.A, F32(np.inf)))
    assert float(np.nextafter(c.B, F32(-np.inf))) < 1.0 + K * hi <= B
    d = probe_distances(eps, inclusive)
    s_in, s_hi = ramp(d, K, A), ramp(d, K, B)
    d64 = d.astype(np.float64)
    assert (d64[s_in > 0] <= lo).all(), (eps, inclusive)
    assert (s_hi[d64 <= hi] == 1).all(), (eps, inclusive)
    assert (s_in[d64 <= r2 * (1.0 - 3.0 * 2.0 ** -20)] == 1).all(), (eps, inclusive)
    assert (s_hi[d64 >= r2 * (1.0 + 3.0 * 2.0 ** -20)] == 0).all(), (eps, inclusive)
    # both sides of every claim were met
    assert (s_in > 0).any() and (s_in == 0).any() and (s_hi == 1).any() and (s_hi < 1).any()
    inf = np.array([np.inf], dtype=np.float32)
    assert ramp(inf, K, A)[0] == 0 and ramp(inf, K, B)[0] == 0


@pytest.mark.parametrize("inclusive", [True, False])
def test_ramp_constants(inclusive):
    for eps in eps_values():
        check_constants(eps, inclusive)


@pytest.mark.parametrize("inclusive", [True, False])
@pytest.mark.parametrize("eps", [2.0 ** -51, 1e20])
def test_not_usable_outside_fp32(eps, inclusive):
    assert not hip.core_ramp_constants(eps, inclusive).usable
