"""Geometric features and neighbour smoothing on synth.forest clouds: wall time (PCIe
included) and HIP-event time per phase, min and median of 5 runs after a warm-up; candidate pair
tests and in-ball pairs with the share of the fp64 vector peak (78.6 TFLOP/s, 8 flops per pair
test); CPU baselines on sampled queries (the restatement: cKDTree with 16 workers) and the
reference's sklearn NearestNeighbors call for the smoothing. One JSON line per case.

    python tools/features_perf.py [--sizes n ...] [--radii r ...] [--ks k ...] [--no-cpu]
                                                  (default: 1000000 5000000; 0.1 0.3 0.6; 25 50 100)
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import hip, synth  # noqa: E402
from tests import features_restatement as R  # noqa: E402

REPS = 5
PEAK_FP64 = 78.6e12
FOUR = ["planarity", "linearity", "verticality", "surface_variation"]
F_PHASES = ("features_grid", "features_moments", "features_finish")
S_PHASES = ("smooth_knn", "smooth_reduce")


def _digest(*arrays):
    """SHA-256 over the arrays' bytes (the first 24 hex digits): equal digests, equal bits."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:24]


def _runs(fn, phases):
    fn()
    walls, per = [], {k: [] for k in phases}
    hip.prof_enable(True)
    for _ in range(REPS):
        hip.prof_reset()
        t = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t) * 1e3)
        for k in phases:
            per[k].append(hip.prof_get(k)[0])
    hip.prof_enable(False)
    stat = {k: {"min": round(min(v), 4), "median": round(float(np.median(v)), 4)} for k, v in per.items()}
    return out, {"wall_ms_min": round(min(walls), 3), "wall_ms_median": round(float(np.median(walls)), 3),
                 "phase_ms": stat}


def candidate_tests(P, radius):
    """Pair tests the kernel makes: every point against the 27 cells of edge ~radius around it."""
    cell = radius * (1.0 + 1.0 / 1048576.0)
    c = np.floor((P - P.min(0)) / cell).astype(np.int64)
    key = (c[:, 2] * (c[:, 1].max() + 3) + c[:, 1]) * (c[:, 0].max() + 3) + c[:, 0]
    uk, cnt = np.unique(key, return_counts=True)
    lookup = dict(zip(uk.tolist(), cnt.tolist()))
    nx, ny = c[:, 0].max() + 3, c[:, 1].max() + 3
    tot = 0
    for k, n in lookup.items():
        s = 0
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    s += lookup.get(k + (dz * ny + dy) * nx + dx, 0)
        tot += n * s
    return tot


def features_case(P, radius, names, cpu):
    (out, cnt), rep = _runs(lambda: hip.geometric_features(P, radius, names, return_counts=True), F_PHASES)
    tests = candidate_tests(P, radius)
    mom = rep["phase_ms"]["features_moments"]["min"] * 1e-3
    rep.update(n=len(P), radius=radius, features=len(names), in_ball_pairs=int(cnt.astype(np.int64).sum()),
               pair_tests=int(tests), fp64_peak_share=round(tests * 8 / mom / PEAK_FP64, 4) if mom > 0 else None,
               nan_rows=int(np.isnan(out[:, 0]).sum()), sha256=_digest(out, cnt))
    if cpu:
        q = np.random.default_rng(0).choice(len(P), 2000, replace=False)
        t = time.perf_counter()
        R.compute_features(P, radius, names, qidx=q)
        per_q = (time.perf_counter() - t) / len(q)
        rep["cpu_restatement_s_per_1M_points_extrapolated_from_2000_queries"] = round(per_q * 1e6, 2)
    return rep


def smooth_case(P, k, cpu):
    V = np.random.default_rng(1).normal(size=len(P))
    out, rep = _runs(lambda: hip.smooth_values(P, V, k, "mean"), S_PHASES)
    rep.update(n=len(P), k=k, sha256=_digest(out))
    if cpu and len(P) <= 1_000_000:
        from sklearn.neighbors import NearestNeighbors
        t = time.perf_counter()
        nb = NearestNeighbors(n_neighbors=k, n_jobs=16).fit(P)
        np.mean(V[nb.kneighbors(P[:100_000])[1]], axis=1)
        rep["cpu_sklearn_s_per_1M_queries_extrapolated_from_100k"] = round((time.perf_counter() - t) * 10, 2)
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 5_000_000])
    ap.add_argument("--radii", type=float, nargs="*", default=[0.1, 0.3, 0.6])
    ap.add_argument("--ks", type=int, nargs="*", default=[25, 50, 100])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-smooth", action="store_true")
    a = ap.parse_args()
    for n in a.sizes:
        P = synth.forest(n)
        for r in a.radii:
            for names in (FOUR, list(hip.FEATURE_NAMES)):
                print(json.dumps({"case": "features", **features_case(P, r, names, not a.no_cpu and n == a.sizes[0])}),
                      flush=True)
        if not a.no_smooth:
            for k in a.ks:
                print(json.dumps({"case": "smooth", **smooth_case(P, k, not a.no_cpu)}), flush=True)


if __name__ == "__main__":
    main()
