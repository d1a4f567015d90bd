"""Plane segmentation on a synth.forest cloud plus a ground sheet: pyqsm_segment_planes with
H hypotheses of m samples and P planes, and pyqsm_segment_plane on the whole cloud. Per case: median and
quartiles of the wall time of the whole call (host clock, host arrays in and out: the finite check, PCIe
and the device), the HIP-event time of every phase from a separate set of repeats (their sum is the call
without PCIe and host work), the count's unfused fp64 operations per second (8 per point and valid
hypothesis) as a share of the 78.6 TFLOP/s fp64 vector peak of the data sheet (which counts a fused
multiply-add as two, so unfused operations reach half of it at most), and the NumPy restatement's count
of one round on the host as the CPU baseline. One JSON line per case, appended to --out.

    python tools/plane_perf.py [--n points] [--H h] [--m m ...] [--P p] [--reps r] [--out file]
                               (default: 1000000; 1000; 3 10; 4; 5; profiles/plane_perf.jsonl)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import hip, synth  # noqa: E402
from pyqsm_amd.math_utils import fit  # noqa: E402
from tests import plane_restatement as R  # noqa: E402

PHASES = ("plane_compact", "plane_models", "plane_count", "plane_flag", "plane_refit")
FP64_PEAK = 78.6e12
THRESH = 0.05


def _quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, dtype=np.float64), [25, 50, 75])
    return {"q1": round(float(q1), 3), "median": round(float(med), 3), "q3": round(float(q3), 3), "n": len(v)}


def _wall(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def cloud(n, seed=0):
    """Half a forest, half a gently sloping ground sheet under it."""
    trees = np.asarray(synth.forest(n // 2), dtype=np.float64)
    rng = np.random.default_rng(seed)
    lo, hi = trees.min(axis=0), trees.max(axis=0)
    g = n - len(trees)
    x, y = rng.uniform(lo[0], hi[0], g), rng.uniform(lo[1], hi[1], g)
    sheet = np.stack([x, y, lo[2] + 0.03 * (x - lo[0]) - 0.01 * (y - lo[1]) + rng.normal(0, 0.01, g)], axis=1)
    return np.ascontiguousarray(np.concatenate([trees, sheet])[rng.permutation(n)])


def _phases(fn, reps):
    per = {p: [] for p in PHASES}
    launches = {}
    hip.prof_enable(True)
    for _ in range(reps):
        hip.prof_reset()
        fn()
        for p in PHASES:
            ms, k = hip.prof_get(p)
            per[p].append(ms)
            launches[p] = int(k)
    hip.prof_enable(False)
    return per, launches


def case(P, H, m, planes, reps, baseline):
    n = len(P)
    draws = fit.draw_u64((planes, H, m), seed=1)
    samples = fit.draw_plane_samples(n, H, m, seed=1)
    peel = lambda: hip.segment_planes(P, draws, THRESH, min_inliers=n // 100)   # noqa: E731
    one = lambda: hip.segment_plane(P, samples, THRESH)                        # noqa: E731
    seg, _ = _wall(peel)  # warm-up
    one()
    walls = {"segment_planes": [], "segment_plane": []}
    for _ in range(reps):
        walls["segment_planes"].append(_wall(peel)[1])
        walls["segment_plane"].append(_wall(one)[1])
    per, launches = _phases(peel, reps)
    per1, _ = _phases(one, reps)
    # the count of the single call: every valid hypothesis against every point, 8 unfused operations a pair
    valid = int((hip.plane_models(P, samples) != 0).any(axis=1).sum())
    count_ms = _quartiles(per1["plane_count"])["median"]
    ops = 8.0 * n * valid
    rec = dict(n=n, H=H, m=m, P=planes, thresh=THRESH, planes_found=len(seg), counts=[int(c) for c in seg.counts],
               used=[int(u) for u in seg.used],
               wall_ms={k: _quartiles(v) for k, v in walls.items()},
               segment_planes_device_ms={p: _quartiles(v) for p, v in per.items()},
               segment_planes_launch_scopes=launches,
               segment_planes_device_sum_ms=round(sum(_quartiles(v)["median"] for v in per.values()), 3),
               segment_plane_device_ms={p: _quartiles(v) for p, v in per1.items()},
               segment_plane_device_sum_ms=round(sum(_quartiles(v)["median"] for v in per1.values()), 3),
               count_valid_hypotheses=valid, count_fp64_ops=ops,
               count_tera_ops_per_s=round(ops / (count_ms * 1e-3) / 1e12, 3) if count_ms > 0 else None,
               count_share_of_fp64_peak=round(ops / (count_ms * 1e-3) / FP64_PEAK, 4) if count_ms > 0 else None)
    if baseline:
        pl = hip.plane_models(P, samples)
        got, ms = _wall(lambda: R.count(P, pl, THRESH))
        rec["numpy_count_ms"] = round(ms, 1)
        rec["numpy_count_equal"] = bool(np.array_equal(got, hip.plane_count(P, pl, THRESH)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--H", type=int, default=1000)
    ap.add_argument("--m", type=int, nargs="*", default=[3, 10])
    ap.add_argument("--P", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "plane_perf.jsonl"))
    a = ap.parse_args()
    P = cloud(a.n)
    for i, m in enumerate(a.m):
        line = json.dumps(case(P, a.H, m, a.P, a.reps, baseline=not a.no_baseline and i == 0))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
