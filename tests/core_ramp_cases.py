"""What the CPU and the GPU test of the core pass's ramps share: the eps values, the floats around the ramps'
thresholds, and the emulation of a ramp: sat(fma(d, -K, C)) computed in float64 and rounded once to float32,
which is what the fma does here (K d is exact, K being a power of two, and near the thresholds the
difference of two values of this size is exact in a double; far from them the clamp hides the rest)."""
import numpy as np

from pyqsm_amd import hip

F32 = np.float32


def eps_values():
    rng = np.random.default_rng(20)
    vals = [0.1, 0.125, 1e-3, 1e3]
    vals += [2.0 ** k for k in range(-40, 41, 4)]
    vals += list(2.0 ** rng.uniform(-40.0, 40.0, 1000 - len(vals)))
    return vals


def r2_of(eps, inclusive):
    return eps * eps if inclusive else np.nextafter(eps * eps, 0.0)


def ramp(d, K, C):
    """sat(fma(d, -K, C)) for float32 d: the exact value, rounded once."""
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.float64(C) - np.float64(K) * d.astype(np.float64)
        return np.clip(v.astype(np.float32), F32(0.0), F32(1.0))


def around(x, ulps=64):
    """The floats within `ulps` ulps of the float nearest to x (positive, away from the format's ends)."""
    c = np.array([x], dtype=np.float32).view(np.int32)[0]
    return (c + np.arange(-ulps, ulps + 1, dtype=np.int32)).astype(np.int32).view(np.float32)


def probe_distances(eps, inclusive):
    """The floats the ramps are checked on at one eps: around A/K, (B-1)/K, lo and hi."""
    c = hip.core_ramp_constants(eps, inclusive)
    K = float(c.K)
    return np.concatenate([around(float(c.A) / K), around((float(c.B) - 1.0) / K), around(float(c.lo)),
                           around(float(c.hi))])
