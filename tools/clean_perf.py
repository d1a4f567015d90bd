"""clean_cloud at the config defaults (voxel 0.04, neighbors 2, ratio 4, iters 3) on synth.forest
clouds: wall time of the fused call (PCIe included), HIP-event time per phase, the time of every
statistical round, output sizes, and the CPU restatement (cKDTree with 16 workers) as baseline.

    python tools/clean_perf.py [n ...]        (default: 1000000 5000000)
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import _lib, hip, synth  # noqa: E402
from tests import clean_restatement as R  # noqa: E402

VOXEL, NEIGHBORS, RATIO, ITERS = 0.04, 2, 4.0, 3
PHASES = ("clean_bbox", "clean_keys", "clean_sort", "clean_segments", "clean_means", "clean_knn",
          "clean_reduce", "clean_compact")
ROUND_PHASES = ("clean_knn", "clean_reduce", "clean_compact")


def _prof(names):
    return {k: round(hip.prof_get(k)[0], 4) for k in names}


def measure(n, reps=5):
    P = synth.forest(n)
    out = hip.clean_cloud(P, VOXEL, NEIGHBORS, RATIO, ITERS)        # warm-up of every shape
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        out = hip.clean_cloud(P, VOXEL, NEIGHBORS, RATIO, ITERS)
        walls.append((time.perf_counter() - t) * 1e3)
    hip.prof_enable(True)
    hip.prof_reset()
    hip.clean_cloud(P, VOXEL, NEIGHBORS, RATIO, ITERS)
    phases = _prof(PHASES)
    # the rounds one by one (the same kernels through pyqsm_stat_outlier), on the clouds the loop sees
    down, _ = hip.voxel_down_sample(P, VOXEL)
    rounds, cur, nb, r = [], down, NEIGHBORS, RATIO
    for _ in range(ITERS):
        hip.stat_outlier(cur, int(nb), r)                            # warm-up
        hip.prof_reset()
        keep = hip.stat_outlier(cur, int(nb), r)
        rounds.append({"k": int(nb), "n_in": len(cur), "n_out": len(keep), **_prof(ROUND_PHASES)})
        cur, nb, r = cur[keep], nb * 2, r / 1.5
    hip.prof_enable(False)
    assert np.array_equal(cur, out)
    t = time.perf_counter()
    ref = R.clean_cloud(P, VOXEL, NEIGHBORS, RATIO, ITERS, workers=16)
    cpu_ms = (time.perf_counter() - t) * 1e3
    return {"n": n, "voxels": len(down), "out": len(out), "wall_ms_min": round(min(walls), 2),
            "wall_ms_median": round(float(np.median(walls)), 2), "phase_ms": phases, "rounds": rounds,
            "cpu_restatement_ms": round(cpu_ms, 1), "same_as_restatement": bool(np.array_equal(ref, out))}


def main():
    _lib.require_gpu(0)
    sizes = [int(a) for a in sys.argv[1:]] or [1_000_000, 5_000_000]
    for n in sizes:
        print(json.dumps(measure(n)), flush=True)


if __name__ == "__main__":
    main()
