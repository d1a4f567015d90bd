"""Branch tracing: the silhouette kernel at m = 5 k, 20 k, 50 k against sklearn's
silhouette_score (its BLAS on the host threads), with its share of the fp64 bound; and
branch_tracing.sphere_step over one synthetic tree (synth.tree_unit) from its trunk seed band:
time per step and for the whole trace, against a CPU composition of the same steps (one cKDTree
of the cloud, scipy kmeans2 + sklearn silhouette_score, sklearn DBSCAN). RANSAC runs on the GPU
in both, so the comparison is of the stages this module moves. One JSON line per measurement.

    python tools/sphere_perf.py [--sizes 5000 20000 50000] [--tree 50000] [--reps 5]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import _lib, branch_tracing, hip, synth  # noqa: E402
from pyqsm_amd.math_utils import clustering  # noqa: E402
from pyqsm_amd.set_config import config  # noqa: E402

# fp64 work per pair: 3 sub, 3 mul, 2 add for d2, 1 sqrt, 1 add into the sum = 10 operations;
# MI355X fp64 vector peak 78.6 TFLOP/s counts an FMA as 2, so 39.3 T non-FMA operations per second
FP64_OPS_PER_PAIR = 10
FP64_OPS_PEAK = 39.3e12


def _cloud(m, k=3, seed=0):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-1, 1, (k, 3))
    lab = rng.integers(0, k, m)
    return centers[lab] + rng.normal(0, 0.25, (m, 3)), lab


def silhouette(m, reps, cpu=True):
    from sklearn.metrics import silhouette_score
    P, lab = _cloud(m)
    hip.silhouette(P, lab, 3)                                    # warm-up
    walls, kern = [], []
    hip.prof_enable(True)
    for _ in range(reps):
        hip.prof_reset()
        t = time.perf_counter()
        score, _ = hip.silhouette(P, lab, 3)
        walls.append((time.perf_counter() - t) * 1e3)
        kern.append(hip.prof_get("silhouette")[0])
    hip.prof_enable(False)
    t = time.perf_counter()
    want = silhouette_score(P, lab) if cpu else np.nan
    cpu_ms = (time.perf_counter() - t) * 1e3 if cpu else np.nan
    k_ms = float(np.median(kern))
    bound_ms = m * m * FP64_OPS_PER_PAIR / FP64_OPS_PEAK * 1e3
    return {"what": "silhouette", "m": m, "gpu_wall_ms_median": round(float(np.median(walls)), 3),
            "gpu_kernel_ms_median": round(k_ms, 3), "fp64_bound_ms": round(bound_ms, 3),
            "fp64_bound_share": round(bound_ms / k_ms, 3), "sklearn_ms": round(cpu_ms, 1),
            "speedup_wall": round(cpu_ms / float(np.median(walls)), 1), "abs_diff_vs_sklearn": abs(score - want)}


class CpuTracer:
    """SphereTracer's interface on the CPU libraries (one cKDTree for the whole trace)."""

    def __init__(self, pts, total_found=(), device=0):
        from scipy.spatial import cKDTree
        self.pts = np.asarray(pts)
        self.device = device
        self.found = np.zeros(len(pts), bool)
        self.mark(total_found)
        self.tree = cKDTree(self.pts)

    def mark(self, idx):
        self.found[np.asarray(idx, dtype=np.int64)] = True

    def ball(self, center, radius):
        idx = np.array(sorted(self.tree.query_ball_point(center, radius)), dtype=np.int64)
        return idx[~self.found[idx]] if len(idx) else idx

    def cluster(self, nn, cluster_type, rng):
        from scipy.cluster.vq import kmeans2
        from sklearn.cluster import DBSCAN
        from sklearn.metrics import silhouette_score
        pts = self.pts[nn]
        returned = []
        if cluster_type == "kmeans":
            ks = clustering.candidate_ks(1)
            labs, scores, present = [], [], []
            for k in ks:
                init = clustering.krandinit(pts[:, :2], k, rng)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    _, book = kmeans2(pts[:, :2], init, minit="matrix")
                labs.append(book)
                n_lab = len(np.unique(book))
                present.append(n_lab)
                scores.append(silhouette_score(pts, book) if 2 <= n_lab <= len(pts) - 1 else 0.0)
            labels, local = clustering.select(ks, labs, scores, present, len(pts))
            returned = [nn[c] for c in local]
        if cluster_type != "kmeans" or len(returned) < 2:
            fit = DBSCAN(eps=config["dbscan"]["epsilon"], min_samples=config["dbscan"]["min_neighbors"]).fit(pts)
            core = np.zeros(len(pts), bool)
            core[fit.core_sample_indices_] = True
            from pyqsm_amd.math_utils.fit import _group_labels
            labels, returned, _ = _group_labels(fit.labels_.astype(np.int64), core, nn)
        return labels, returned

    def free(self):
        pass


def trace(n, reps, cpu=True):
    P = synth.tree_unit(0, n)
    r = np.hypot(P[:, 0], P[:, 1])
    seed_idx = np.flatnonzero((P[:, 2] < 0.3) & (r < 0.5))

    def run(tracer_cls=None):
        spheres = []
        kw = {}
        if tracer_cls is not None:
            kw["tracer"] = tracer_cls(P, list(seed_idx))
        t = time.perf_counter()
        out = branch_tracing.sphere_step(P[seed_idx].copy(), 0.3, P, seed_idx, total_found=list(seed_idx),
                                         spheres=spheres, seed=1, **kw)
        return (time.perf_counter() - t) * 1e3, len(spheres), out

    run()                                                        # warm-up
    hip.prof_enable(True)
    hip.prof_reset()
    gpu = [run() for _ in range(reps)]
    phases = {k: round(hip.prof_get(k)[0] / reps, 3) for k in
              ("ball_excl", "kmeans_select", "kmeans_lloyd", "silhouette_group", "silhouette", "dbscan_total")}
    hip.prof_enable(False)
    walls = [g[0] for g in gpu]
    steps = gpu[0][1]
    found = len(gpu[0][2][0][0]) if gpu[0][2] != [] else 0
    cpu_ms, cpu_steps, _ = run(CpuTracer) if cpu else (np.nan, 0, None)
    med = float(np.median(walls))
    return {"what": "sphere_step", "n": n, "steps": steps, "found": found, "gpu_trace_ms_median": round(med, 1),
            "gpu_trace_ms_min": round(min(walls), 1), "gpu_ms_per_step": round(med / max(steps, 1), 3),
            "device_ms_per_trace": phases, "cpu_trace_ms": round(cpu_ms, 1), "cpu_steps": cpu_steps,
            "cpu_ms_per_step": round(cpu_ms / max(cpu_steps, 1), 3), "speedup": round(cpu_ms / med, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[5000, 20_000, 50_000])
    ap.add_argument("--tree", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baselines (profiler runs)")
    a = ap.parse_args()
    _lib.require_gpu(0)
    for m in a.sizes:
        print(json.dumps(silhouette(m, a.reps, not a.no_cpu)), flush=True)
    if a.tree:
        print(json.dumps(trace(a.tree, a.reps, not a.no_cpu)), flush=True)


if __name__ == "__main__":
    main()
