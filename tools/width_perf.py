"""Stem width: pyqsm_pdist_select on the points of a noisy ring, with the seven order
statistics width_at_height asks for (two each for p90, p95 and the median, one for the maximum). Per
case: median and quartiles of the wall time of the whole call (host clock, host arrays in and out), the
HIP-event time of the passes from a separate set of repeats, and from it the pair evaluations per
second (passes x pairs over the device time). Cases: one segment of every --n; --segs segments of
--seg-n points in one call and as one call each; scipy's pdist + np.percentile on the first --n as the
CPU baseline, with a check that both give the same bits. One JSON line per case, appended to --out.

    python tools/width_perf.py [--n points ...] [--segs s] [--seg-n p] [--reps r] [--out file]
                               (default: 16384 50000 100000; 1000; 600; 5; profiles/width_perf.jsonl)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import hip  # noqa: E402
from pyqsm_amd.geometry import stem_width as sw  # noqa: E402

PHASES = ("pdist_max_passes", "pdist_passes")
QS = [50, 90, 95]


def _quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, dtype=np.float64), [25, 50, 75])
    return {"q1": round(float(q1), 3), "median": round(float(med), 3), "q3": round(float(q3), 3), "n": len(v)}


def _wall(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def ring(n, seed=0, radius=0.15, sigma=0.005):
    """The xy of a stem slab: a circle of the given radius with Gaussian noise on the radius."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, n)
    r = radius + rng.normal(0, sigma, n)
    return np.ascontiguousarray(np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1))


def width_ranks(m):
    lo, hi, _ = sw.percentile_ranks(m, [90, 95])
    return np.array([lo[0], hi[0], lo[1], hi[1], *sw.middle_ranks(m), m - 1], np.int64)


def _device_ms(fn, reps):
    per = []
    hip.prof_enable(True)
    for _ in range(reps):
        hip.prof_reset()
        fn()
        per.append(sum(hip.prof_get(p)[0] for p in PHASES))
    hip.prof_enable(False)
    return per


def _rate(res, device_ms):
    med = _quartiles(device_ms)["median"]
    return round(res.stats["pair_evaluations"] / (med * 1e-3), 1) if med > 0 else None


def single(n, reps):
    P = ring(n)
    m = n * (n - 1) // 2
    ranks = width_ranks(m)
    call = lambda: hip.pdist_select(P, None, ranks)     # noqa: E731
    res, first_ms = _wall(call)
    walls = [_wall(call)[1] for _ in range(reps)]
    dev = _device_ms(call, reps)
    return dict(case="single", n=n, dim=2, pairs=m, ranks=len(ranks), passes=res.stats["passes"],
                pair_evaluations=res.stats["pair_evaluations"], first_call_ms=round(first_ms, 3),
                wall_ms=_quartiles(walls), device_ms=_quartiles(dev), pair_evaluations_per_s=_rate(res, dev),
                max_width=float(res.values[0, 6]), p95=float(sw.pairwise_distance_quantiles(P, 95)))


def batch(segs, seg_n, reps):
    P = ring(segs * seg_n, seed=1)
    seg = np.arange(segs + 1, dtype=np.int64) * seg_n
    ranks = np.tile(width_ranks(seg_n * (seg_n - 1) // 2), (segs, 1))
    one_call = lambda: hip.pdist_select(P, seg, ranks)                                         # noqa: E731
    many = lambda: [hip.pdist_select(P[seg[s]:seg[s + 1]], None, ranks[s]) for s in range(segs)]    # noqa: E731
    res, _ = _wall(one_call)
    parts, _ = _wall(many)
    equal = all(np.array_equal(res.values[s], parts[s].values[0]) and np.array_equal(res.max_pair[s], parts[s].max_pair[0])
                for s in range(segs))
    walls = {"one_call": [_wall(one_call)[1] for _ in range(reps)], "one_call_each": [_wall(many)[1] for _ in range(reps)]}
    dev = _device_ms(one_call, reps)
    return dict(case="batch", segments=segs, n_per_segment=seg_n, dim=2, pairs=res.stats["pairs"],
                passes=res.stats["passes"], wall_ms={k: _quartiles(v) for k, v in walls.items()},
                one_call_device_ms=_quartiles(dev), one_call_pair_evaluations_per_s=_rate(res, dev), same_results=equal)


def baseline(n):
    from scipy.spatial.distance import pdist
    P = ring(n)
    (d, want), ms = _wall(lambda: (lambda d: (d, np.percentile(d, QS)))(pdist(P)))
    got, gpu_ms = _wall(lambda: sw.pairwise_distance_quantiles(P, QS))
    return dict(case="scipy_baseline", n=n, pairs=len(d), percentiles=QS, cpus=os.cpu_count(),
                scipy_pdist_percentile_ms=round(ms, 1), pairwise_distance_quantiles_ms=round(gpu_ms, 3),
                same_bits=bool(np.array_equal(got, want)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[16384, 50000, 100000])
    ap.add_argument("--segs", type=int, default=1000)
    ap.add_argument("--seg-n", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "width_perf.jsonl"))
    a = ap.parse_args()
    hip.pdist_select(ring(1000), None, width_ranks(499500))     # loads the code objects
    cases = [lambda n=n: single(n, a.reps) for n in a.n]
    if a.segs:
        cases.append(lambda: batch(a.segs, a.seg_n, a.reps))
    if a.n and not a.no_baseline:
        cases.append(lambda: baseline(a.n[0]))
    for run in cases:
        line = json.dumps(run())
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
