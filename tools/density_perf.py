"""Radius-graph degrees and pair list on synth.forest: for every radius alone and for all
of them in one call, the HIP-event time of the "radius_degrees" scope (the cell-run kernels only),
the wall time of the call (upload, grid build, run lists and download included), median and min of
REPS runs after a warm-up, and distance tests per second from the call's statistics; the pair list at
the smallest radius ("radius_pairs": count pass, fill pass and the two sorts). The yardstick, which
is also the answer the degrees are compared with, is SciPy's
cKDTree.query_ball_point(P, r, return_length=True, workers=W) - 1 on the same cloud (--scipy-radii
picks for which radii: the large ones take minutes on the host). One JSON line per case, appended to
--out as well.

    python tools/density_perf.py [--n 1000000] [--radii 0.05 0.1 0.3] [--scipy-radii ...] [--workers 16]
                                 [--out profiles/density_perf.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import hip, synth  # noqa: E402

REPS = 10


def _median_min(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4)}


def _timed(fn, scope):
    fn()
    walls, dev = [], []
    hip.prof_enable(True)
    for _ in range(REPS):
        hip.prof_reset()
        t = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t) * 1e3)
        dev.append(hip.prof_get(scope)[0])
    hip.prof_enable(False)
    return out, _median_min(walls), _median_min(dev)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def degrees_case(P, radii):
    (deg, n_pairs), wall, dev = _timed(lambda: hip.radius_degrees(P, radii), "radius_degrees")
    stats = {}
    hip.radius_degrees(P, radii, stats=stats)
    k_ms = dev["median"]
    rec = dict(case="degrees", radii=list(radii), n_pairs=[int(v) for v in n_pairs],
               mean_degree=[round(float(d.mean()), 2) for d in deg], max_degree=[int(d.max()) for d in deg],
               kernel_ms=dev, wall_ms=wall, distance_tests=stats["distance_tests"],
               candidates_staged=stats["candidates_staged"],
               distance_tests_per_s=round(stats["distance_tests"] / (k_ms * 1e-3), 1) if k_ms > 0 else None)
    return rec, deg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--radii", type=float, nargs="*", default=[0.05, 0.1, 0.3])
    ap.add_argument("--scipy-radii", type=float, nargs="*", default=None, help="default: all of --radii")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P = np.ascontiguousarray(synth.forest(a.n), dtype=np.float64)
    head = {"n": a.n, "cloud": "synth.forest"}
    single = {}
    for r in a.radii:
        rec, deg = degrees_case(P, [r])
        single[r] = deg[0]
        emit({**head, **rec}, a.out)
    if len(a.radii) > 1:
        rec, deg = degrees_case(P, a.radii)
        rec["rows_equal_single_calls"] = all(np.array_equal(deg[k], single[r]) for k, r in enumerate(a.radii))
        emit({**head, **rec}, a.out)
    r0 = min(a.radii)
    n_pairs = int(single[r0].astype(np.int64).sum() // 2)
    pairs, wall, dev = _timed(lambda: hip.radius_pairs(P, r0, n_pairs), "radius_pairs")
    emit({**head, "case": "pairs", "radius": r0, "rows": len(pairs), "kernel_and_sort_ms": dev, "wall_ms": wall,
          "degrees_from_rows_equal": bool(np.array_equal(np.bincount(pairs.ravel(), minlength=len(P)), single[r0]))},
         a.out)
    from scipy.spatial import cKDTree
    t = time.perf_counter()
    tree = cKDTree(P)
    build = time.perf_counter() - t
    for r in (a.radii if a.scipy_radii is None else a.scipy_radii):
        t = time.perf_counter()
        d = tree.query_ball_point(P, r, return_length=True, workers=a.workers) - 1
        q = time.perf_counter() - t
        emit({**head, "case": "scipy_query_ball_point", "radius": r, "workers": a.workers,
              "kdtree_build_s": round(build, 3), "query_s": round(q, 3),
              "equals_gpu_degrees": bool(np.array_equal(d, single[r])) if r in single else None}, a.out)


if __name__ == "__main__":
    main()
