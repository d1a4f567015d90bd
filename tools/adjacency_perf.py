"""Cluster adjacency on block-labelled synth.forest clouds at threshold 0.35: wall time
(PCIe and host label handling included) and HIP-event time of the "cluster_adjacency" scope, median
and min of 10 runs after a warm-up; distance tests per second; pairs of table atomics per source
point with and without the per-lane accumulation; the time of the closest-pair pass. Two yardsticks,
neither of them the code under test: (a) the reference's method on the CPU, one
cKDTree.sparse_distance_matrix per cluster pair, on every tenth point as the reference samples and
unsampled (--cpu, needs no GPU; above --cpu-pairs cluster pairs a spread of source clusters is timed
and the total extrapolated, which the record says); (b) pyqsm_radius_mark over the same sources and
targets at the same radius with k too large to cut anything: the same candidate walk with no table.
One JSON line per case.

    python tools/adjacency_perf.py [--sizes n ...] [--edges e ...] [--threshold t]     (GPU cases)
    python tools/adjacency_perf.py --cpu [--sizes n ...] [--edges e ...]               (yardstick a)
                                                 (default: 1000000 5000000; 0.8 2.0; 0.35)
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


def block_labels(P, edge):
    """Index of each point's block of edge `edge` among the occupied blocks, in the order
    np.unique(floor(P / edge), axis=0) gives them (x, then y, then z)."""
    c = np.floor(P / edge).astype(np.int64)
    c -= c.min(0)
    ext = c.max(0) + 1
    key = (c[:, 0] * ext[1] + c[:, 1]) * ext[2] + c[:, 2]
    _, lab = np.unique(key, return_inverse=True)
    return lab.reshape(-1).astype(np.int64)


def forms(P, lab):
    """(name, source points, labels, target points, labels); targets None: the same-cloud form."""
    s = lab % 3 == 0
    return [("same_cloud", P, lab, None, None), ("bipartite", P[s], lab[s], P[~s], lab[~s])]


def _median_min(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4)}


def _timed(fn, scopes):
    fn()
    walls, per = [], {k: [] for k in scopes}
    hip.prof_enable(True)
    for _ in range(REPS):
        hip.prof_reset()
        t = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t) * 1e3)
        for k in scopes:
            per[k].append(hip.prof_get(k)[0])
    hip.prof_enable(False)
    return out, _median_min(walls), {k: _median_min(v) for k, v in per.items()}


def gpu_case(name, s, sl, t, tl, threshold):
    call = lambda **kw: hip.cluster_adjacency(s, sl, threshold, t, tl, **kw)  # noqa: E731
    res, wall, dev = _timed(call, ("cluster_adjacency",))
    _, wall_w, dev_w = _timed(lambda: call(return_pairs=True), ("cluster_adjacency", "cluster_adjacency_witness"))
    with_cache, without = {}, {}
    call(stats=with_cache)
    call(stats=without, cache=False)
    hip.prof_enable(True)
    hip.prof_reset()
    call(cache=False)
    no_cache_ms = hip.prof_get("cluster_adjacency")[0]
    hip.prof_enable(False)
    n_src = int((np.asarray(sl) >= 0).sum())
    kernel_ms = dev["cluster_adjacency"]["median"]
    rep = dict(form=name, sources=len(s), targets=len(s) if t is None else len(t),
               source_clusters=len(np.unique(sl)), target_clusters=len(np.unique(sl if t is None else tl)),
               cluster_pairs=len(res.a), point_pairs=int(res.n_pairs.sum()),
               wall_ms=wall, kernel_ms=dev["cluster_adjacency"],
               wall_ms_with_closest_pair=wall_w, kernel_ms_with_closest_pair=dev_w["cluster_adjacency"],
               closest_pair_pass_ms=dev_w["cluster_adjacency_witness"],
               distance_tests=with_cache["distance_tests"],
               distance_tests_per_s=round(with_cache["distance_tests"] / (kernel_ms * 1e-3), 1) if kernel_ms > 0 else None,
               atomic_pairs_per_source_point=round(with_cache["atomic_pairs"] / n_src, 3),
               atomic_pairs_per_source_point_no_cache=round(without["atomic_pairs"] / n_src, 3),
               kernel_ms_no_cache=round(no_cache_ms, 4))
    # yardstick (b): the same walk with no table (strict bound there, inclusive here: same candidates)
    src, qry = (s, s) if t is None else (t, s)
    _, _, dev_m = _timed(lambda: hip.radius_mark(src, qry, threshold, k=2**31 - 1), ("radius_mark",))
    rep["radius_mark_kernel_ms"] = dev_m["radius_mark"]
    if dev_m["radius_mark"]["median"] > 0:
        rep["kernel_ms_over_radius_mark"] = round(kernel_ms / dev_m["radius_mark"]["median"], 3)
    return rep


def cpu_case(name, s, sl, t, tl, threshold, max_pairs):
    """The reference's loop: a cKDTree per cluster, sparse_distance_matrix per cluster pair."""
    from scipy.spatial import cKDTree
    same = t is None
    if same:
        t, tl = s, sl
    t0 = time.perf_counter()
    s_trees = [(int(l), cKDTree(s[sl == l])) for l in np.unique(sl)]
    t_trees = s_trees if same else [(int(l), cKDTree(t[tl == l])) for l in np.unique(tl)]
    build = time.perf_counter() - t0
    total = len(s_trees) * len(t_trees)
    step = max(1, -(-total // max_pairs))
    t0 = time.perf_counter()
    found = 0
    for a, ta in s_trees[::step]:
        for b, tb in t_trees:
            if same and not a < b:
                continue
            m = ta.sparse_distance_matrix(tb, threshold, output_type="ndarray")
            if m.shape[0] > 0:
                m["v"].min()
                found += 1
    loop = time.perf_counter() - t0
    served = len(s_trees[::step])
    return dict(form=name, sources=len(s), targets=len(t), source_clusters=len(s_trees),
                target_clusters=len(t_trees), kdtree_build_s=round(build, 3), source_clusters_timed=served,
                loop_s_timed=round(loop, 3), loop_s=round(loop * len(s_trees) / served, 3),
                extrapolated=served != len(s_trees), cluster_pairs_found_in_timed_part=found)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 5_000_000])
    ap.add_argument("--edges", type=float, nargs="*", default=[0.8, 2.0])
    ap.add_argument("--threshold", type=float, default=0.35)
    ap.add_argument("--cpu", action="store_true", help="yardstick (a) only; needs no GPU")
    ap.add_argument("--cpu-pairs", type=int, default=2_000_000, help="cluster pairs timed before extrapolating")
    a = ap.parse_args()
    for n in a.sizes:
        P = np.ascontiguousarray(synth.forest(n), dtype=np.float64)
        for edge in a.edges:
            lab = block_labels(P, edge)
            for name, s, sl, t, tl in forms(P, lab):
                head = {"n": n, "block_edge": edge, "threshold": a.threshold}
                if not a.cpu:
                    print(json.dumps({"case": "gpu", **head, **gpu_case(name, s, sl, t, tl, a.threshold)}), flush=True)
                    continue
                if n > 1_000_000:
                    continue
                for every in (10, 1):
                    # the reference samples each cluster [::10]; in a cloud sorted by label that is every tenth point
                    o = np.argsort(sl, kind="stable")[::every]
                    ot = None if t is None else np.argsort(tl, kind="stable")[::every]
                    rep = cpu_case(name, s[o], sl[o], None if t is None else t[ot], None if t is None else tl[ot],
                                   a.threshold, a.cpu_pairs)
                    print(json.dumps({"case": "cpu_scipy_loop", **head, "sample_every": every, **rep}), flush=True)


if __name__ == "__main__":
    main()
