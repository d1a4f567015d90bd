"""Epiphyte split: the three device stages of identify_epiphytes' tail on a synthetic
tree of --n points (synth.tree_unit). One JSON line per case, appended to --out.

  kmeans   hip.kmeans_pp, k = --k, d = 3: HIP-event time of the phases (centring, seeding, Lloyd, the
           final pass; median of --reps) and, from a run of its own, of the single kernels summed over
           the call (the Lloyd ones include the no-ops queued behind the "done" word), the wall time of the whole call with the upload, the iteration
           count, the Lloyd time per iteration and what it is of the bytes one iteration must read
           (n * d * 8) at the 6.3 TB/s a streaming kernel reaches on this part.
  sklearn  sklearn.cluster.KMeans on the same points and threads as the machine gives (skipped when
           scikit-learn is missing), and whether the labels agree.
  shift    hip.shift_components on --n shift vectors against the NumPy formulation of the reference
           (row norms, two np.percentile, np.where), with a check that both give the same partition.
  tail     geometry.epiphytes.identify_epiphytes on one cloud: splits -> clumps -> areas, wall time.

    python tools/epiphyte_perf.py [--n points] [--k clusters] [--reps r] [--out file]
                                  (default: 1000000; 20; 5; profiles/epiphyte_perf.jsonl)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import hip, synth  # noqa: E402
from pyqsm_amd.geometry import epiphytes  # noqa: E402
from pyqsm_amd.geometry.cloud import PointCloud  # noqa: E402
from pyqsm_amd.math_utils.clustering import kmeanspp_draws  # noqa: E402

KMEANS_PHASES = ("kmeanspp_centre", "kmeanspp_seed", "kmeanspp_lloyd", "kmeanspp_final")
KMEANS_KERNELS = ("kmeanspp_closest", "kmeanspp_pick", "kmeanspp_trial", "kmeanspp_choose", "kmeanspp_assign",
                  "kmeanspp_colsums")
SHIFT_PHASES = ("select_passes", "shift_split", "shift_labels")
STREAM_BYTES_PER_S = 6.3e12


def _quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, dtype=np.float64), [25, 50, 75])
    return {"q1": round(float(q1), 3), "median": round(float(med), 3), "q3": round(float(q3), 3), "n": len(v)}


def _wall(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def _device_ms(fn, reps, phases, level=1):
    per = {p: [] for p in phases}
    hip.prof_enable(level)
    for _ in range(reps):
        hip.prof_reset()
        fn()
        for p in phases:
            per[p].append(hip.prof_get(p)[0])
    hip.prof_enable(False)
    return per


def shift_field(n, seed=0):
    rng = np.random.default_rng(seed)
    s = rng.normal(0, 0.02, (n, 3))
    big = rng.random(n) < 0.5
    s[big] += rng.normal(0, 0.3, (int(big.sum()), 3)) + np.array([0, 0, -0.1])
    return s


def kmeans_case(x, k, reps):
    n, d = x.shape
    first, u = kmeanspp_draws(n, k, 0)
    call = lambda: hip.kmeans_pp(x, k, first, u)     # noqa: E731
    res, first_ms = _wall(call)
    walls = [_wall(call)[1] for _ in range(reps)]
    dev = _device_ms(call, reps, KMEANS_PHASES)
    kernels = _device_ms(call, reps, KMEANS_KERNELS, level=2)     # events around single kernels: a run of its own
    lloyd = _quartiles(dev["kmeanspp_lloyd"])["median"]
    per_iter_us = lloyd * 1e3 / res.n_iter
    model_us = n * d * 8 / STREAM_BYTES_PER_S * 1e6
    return res, dict(case="kmeans", n=n, d=d, k=k, n_iter=res.n_iter, n_empty=res.n_empty, inertia=res.inertia,
                     first_call_ms=round(first_ms, 3), wall_ms=_quartiles(walls),
                     device_ms={p: _quartiles(v) for p, v in dev.items()},
                     kernel_ms={p: _quartiles(v)["median"] for p, v in kernels.items()},
                     device_total_ms=round(sum(_quartiles(v)["median"] for v in dev.values()), 3),
                     lloyd_us_per_iteration=round(per_iter_us, 2), byte_model_us_per_iteration=round(model_us, 2),
                     fraction_of_stream_rate=round(model_us / per_iter_us, 3))


def sklearn_case(x, k, ours):
    try:
        from sklearn.cluster import KMeans
    except ImportError:
        return dict(case="sklearn", skipped="scikit-learn is not installed")
    km, ms = _wall(lambda: KMeans(n_clusters=k, random_state=0, n_init="auto").fit(x))
    return dict(case="sklearn", n=len(x), k=k, cpus=len(os.sched_getaffinity(0)),
                threads=os.environ.get("OMP_NUM_THREADS"), fit_ms=round(ms, 1), n_iter=int(km.n_iter_),
                labels_equal=bool(np.array_equal(km.labels_, ours.labels)),
                labels_differing=int((km.labels_ != ours.labels).sum()),
                inertia_relative_difference=abs(km.inertia_ - ours.inertia) / km.inertia_)


def shift_case(n, reps):
    shift = shift_field(n)
    call = lambda: hip.shift_components(shift)     # noqa: E731
    res, first_ms = _wall(call)
    walls = [_wall(call)[1] for _ in range(reps)]
    dev = _device_ms(call, reps, SHIFT_PHASES)

    def numpy_form():
        mag = np.linalg.norm(shift, axis=1)
        high = np.where(mag > np.percentile(mag, 65))[0]
        z = shift[high, 2]
        return high, high[np.where(z > np.percentile(z, 60))[0]]

    (high, leaves), np_ms = _wall(numpy_form)
    same = np.array_equal(np.nonzero(res.labels > 0)[0], high) and np.array_equal(np.nonzero(res.labels == 1)[0], leaves)
    return dict(case="shift", n=n, counts=res.counts.tolist(), first_call_ms=round(first_ms, 3),
                wall_ms=_quartiles(walls), device_ms={p: _quartiles(v) for p, v in dev.items()},
                numpy_ms=round(np_ms, 3), same_partition=bool(same))


def tail_case(x, reps):
    content = {"seed": 0, "src": None, "clean_pcd": PointCloud(x), "shift_one": shift_field(len(x), seed=1)}
    call = lambda: epiphytes.identify_epiphytes(content, voxel_size=0.1, alpha=0.4)     # noqa: E731
    out, first_ms = _wall(call)
    walls = [_wall(call)[1] for _ in range(reps)]
    return dict(case="tail", n=len(x), counts=out["counts"].tolist(), first_call_ms=round(first_ms, 3),
                wall_ms=_quartiles(walls), metrics={k: float(v) for k, v in out["metrics"][0].items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--no-tail", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "epiphyte_perf.jsonl"))
    a = ap.parse_args()
    x = synth.tree_unit(seed=0, n=a.n)
    hip.kmeans_pp(x[:5000], a.k, *kmeanspp_draws(5000, a.k, 0))     # loads the code objects
    hip.shift_components(shift_field(5000))
    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")

    ours, line = kmeans_case(x, a.k, a.reps)
    emit(line)
    emit(shift_case(len(x), a.reps))
    if not a.no_tail:
        emit(tail_case(x, max(1, a.reps // 2)))
    if not a.no_sklearn:
        emit(sklearn_case(x, a.k, ours))


if __name__ == "__main__":
    main()
