"""Tree-ensemble inference: 201 unrestricted trees fitted by scikit-learn on 32 000
rows of 7 features in 3 overlapping Gaussian classes; prediction (probabilities and labels) of
1 M and 5 M rows. Kernel time (HIP events around the walk kernel) and wall time with the PCIe
transfers, min and median of 5 runs after a warm-up, for every staged depth; node visits per
second (the visits counted on the host from the leaves' depths of a 50 000-row sample); and
scikit-learn's predict_proba of the same forest on the same machine (1 M rows with n_jobs=16,
200 000 rows with n_jobs=1), per million rows. One JSON line per case.

    python tools/forest_perf.py [--sizes n ...] [--staged s ...] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import hip  # noqa: E402
from pyqsm_amd.math_utils.forest import GPUForest  # noqa: E402
from tests import forest_restatement as R  # noqa: E402

REPS = 5


def _runs(fn):
    fn()
    walls, kern = [], []
    hip.prof_enable(True)
    for _ in range(REPS):
        hip.prof_reset()
        t = time.perf_counter()
        fn()
        walls.append((time.perf_counter() - t) * 1e3)
        kern.append(hip.prof_get("forest_walk")[0])
    hip.prof_enable(False)
    return {"wall_ms_min": round(min(walls), 3), "wall_ms_median": round(float(np.median(walls)), 3),
            "kernel_ms_min": round(min(kern), 3), "kernel_ms_median": round(float(np.median(kern)), 3)}


def node_depths(trees):
    """Per tree the depth of every node (root 0)."""
    out = []
    for left, right, *_ in trees:
        d = np.zeros(len(left), np.int64)
        for i in range(len(left)):              # scikit-learn numbers parents before children
            if left[i] != -1:
                d[left[i]] = d[right[i]] = d[i] + 1
        out.append(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 5_000_000])
    ap.add_argument("--staged", type=int, nargs="*", default=list(hip.FOREST_STAGED))
    ap.add_argument("--trees", type=int, default=201)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    from sklearn.ensemble import RandomForestClassifier
    Xt, yt = R.gaussian_classes(32_000, 7, 3, seed=5, spread=0.5)
    rf = RandomForestClassifier(n_estimators=a.trees, random_state=42, n_jobs=16).fit(Xt, yt)
    forest = GPUForest.from_sklearn(rf)
    dev = forest.device_forest()
    info = dev.info()
    print(json.dumps({"case": "forest", **info}), flush=True)
    trees = R.trees_of(rf)
    depths = node_depths(trees)
    for n in a.sizes:
        X, _ = R.gaussian_classes(n, 7, 3, seed=6, spread=0.5)
        sample = X[np.random.default_rng(0).choice(n, 50_000, replace=False)]
        leaves = dev.apply(sample)
        # records read per row: every node on the path, the leaf's included
        visits_per_row = float(np.mean(sum(depths[k][leaves[:, k]] + 1 for k in range(len(trees)))))
        below = {s: float(np.mean(sum(np.maximum(0, depths[k][leaves[:, k]] + 1 - max(1, int(np.log2(s + 1))))
                                      for k in range(len(trees))))) if s > 0 else visits_per_row
                 for s in a.staged}
        for s in a.staged:
            dev.stage(s)
            rep = _runs(lambda: dev.predict(X, True, True, False))
            k = rep["kernel_ms_min"] * 1e-3
            rep.update(case="predict", n=n, trees=len(trees), staged_nodes=s,
                       visits_per_row=round(visits_per_row, 1),
                       visits_below_full_staged_levels_per_row=round(below[s], 1),
                       node_visits_per_s=round(visits_per_row * n / k, 0) if k > 0 else None)
            print(json.dumps(rep), flush=True)
        dev.stage(info['staged_nodes'])
    if not a.no_cpu:
        X, _ = R.gaussian_classes(1_000_000, 7, 3, seed=6, spread=0.5)
        for jobs, rows in ((16, 1_000_000), (1, 200_000)):
            rf.n_jobs = jobs
            t = time.perf_counter()
            rf.predict_proba(X[:rows])
            s = time.perf_counter() - t
            print(json.dumps({"case": "sklearn_predict_proba", "n_jobs": jobs, "rows": rows, "seconds": round(s, 3),
                              "seconds_per_1M_rows": round(s * 1e6 / rows, 3)}), flush=True)
    forest.free()


if __name__ == "__main__":
    main()
