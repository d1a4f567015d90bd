"""Radius-graph degrees and pair list on synth.forest: for every radius alone and for all
of them in one call, the HIP-event time of the "radius_degrees" scope (the cell-run kernels only),
the wall time of the call (upload, grid build, run lists and download included), median and min of
REPS runs after a warm-up, and distance tests per second from the call's statistics; the pair list at
the smallest radius ("radius_pairs": count pass, fill pass and the two sorts). The yardstick, which
is also the answer the degrees are compared with, is SciPy's
cKDTree.query_ball_point(P, r, return_length=True, workers=W) - 1 on the same cloud (--scipy-radii
picks for which radii: the large ones take minutes on the host). One JSON line per case, appended to
--out as well.

--cases components: the components ranked by size (hip.radius_components) at every radius alone and the
--sweep radii as one call: kernel = the "radius_components_union" scope (init, the two union launches,
flatten) and the "radius_components_rank" scope (sizes, compaction, sort, labels), wall = the whole call.
Next to each record its baseline, what the library offered before for the same answer, in the same
process: hip.dbscan(P, r, 1) and rank_components in NumPy on the host (one dbscan call per radius for the
sweep); at the smallest radius also the pair-list route, hip.radius_pairs and SciPy's
connected_components. Every baseline's answer is compared with the call's.

    python tools/density_perf.py [--n 1000000] [--radii 0.05 0.1 0.3] [--scipy-radii ...] [--workers 16]
                                 [--cases degrees components] [--sweep .06 .07 .08 .09]
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


def _timed(fn, *scopes):
    """(result, wall, device time of scope 0, of scope 1, ...): median and min of REPS after a warm-up."""
    fn()
    walls, dev = [], [[] for _ in scopes]
    hip.prof_enable(bool(scopes))
    for _ in range(REPS):
        hip.prof_reset()
        t = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t) * 1e3)
        for d, scope in zip(dev, scopes):
            d.append(hip.prof_get(scope)[0])
    hip.prof_enable(False)
    return (out, _median_min(walls)) + tuple(_median_min(d) for d in dev)


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


def rank_components(labels):
    """(component, sizes) from any labelling: ranks by (size descending, smallest member ascending);
    tests/density_restatement.py's statement."""
    _, first, inv, counts = np.unique(labels, return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((first, -counts))
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    return rank[inv].astype(np.int32), counts[order].astype(np.int32)


def components_case(P, radii, head, out, pair_route=False):
    (comp, sizes), wall, union, rank = _timed(lambda: hip.radius_components(P, radii), "radius_components_union",
                                              "radius_components_rank")
    emit({**head, "case": "components", "radii": list(radii), "n_components": [len(s) for s in sizes],
          "largest": [int(s[0]) for s in sizes], "union_kernel_ms": union, "rank_kernel_ms": rank,
          "wall_ms": wall}, out)

    def dbscan_route():
        return [rank_components(hip.dbscan(P, r, 1)[0]) for r in radii]

    ref, wall = _timed(dbscan_route)
    _, dbscan_wall = _timed(lambda: [hip.dbscan(P, r, 1) for r in radii])
    same = all(np.array_equal(c0, c1) and np.array_equal(s0, s1) for (c0, s0), c1, s1 in zip(ref, comp, sizes))
    emit({**head, "case": "components_baseline_dbscan_min_pts_1_host_rank", "radii": list(radii), "wall_ms": wall,
          "dbscan_calls_wall_ms": dbscan_wall, "equals_components": bool(same)}, out)
    if pair_route:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components

        def pairs_route():
            p = hip.radius_pairs(P, radii[0])
            g = coo_matrix((np.ones(len(p), dtype=np.int8), (p[:, 0], p[:, 1])), shape=(len(P), len(P)))
            return rank_components(connected_components(g, directed=False)[1])

        (c0, s0), wall = _timed(pairs_route)
        emit({**head, "case": "components_baseline_radius_pairs_scipy", "radii": list(radii), "wall_ms": wall,
              "equals_components": bool(np.array_equal(c0, comp[0]) and np.array_equal(s0, sizes[0]))}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--radii", type=float, nargs="*", default=[0.05, 0.1, 0.3])
    ap.add_argument("--scipy-radii", type=float, nargs="*", default=None, help="default: all of --radii")
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", nargs="*", default=["degrees", "components"], choices=["degrees", "components"])
    ap.add_argument("--sweep", type=float, nargs="*", default=[.06, .07, .08, .09])
    a = ap.parse_args()
    P = np.ascontiguousarray(synth.forest(a.n), dtype=np.float64)
    head = {"n": a.n, "cloud": "synth.forest"}
    if "components" in a.cases:
        for r in a.radii:
            components_case(P, [r], head, a.out, pair_route=(r == min(a.radii)))
        if a.sweep:
            components_case(P, a.sweep, head, a.out)
    if "degrees" not in a.cases:
        return
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
