"""Region growing: extend_seed_clusters with the host engine (one pyqsm_radius_label call
per cycle) against the device engine (one pyqsm_grow_clusters call) on synth.forest clouds, seeds = the
DBSCAN clusters (eps 0.1, 10 points) of the slice below z = 0.3, pyQSM's defaults k = 200, radius 0.1,
150 cycles. Both engines run in the same process, alternating, after a warm-up: median and quartiles
of the wall time of the whole call (host clock; every call ends in a synchronise) and of the device
engine's growing alone (grow_seed_clusters, without the clouds' reconstruction on the host). From a
separate set of repeats the HIP-event time of the device engine's phases. The two engines' outputs are
compared on the spot. For scale, hip.radius_mark with the largest frontier of the run as queries. One
JSON line per size, appended to --out.

    python tools/grow_perf.py [--sizes n ...] [--reps r] [--cycles c] [--out file]
                                        (default: 1000000 5000000; 5; 150; profiles/grow_perf.jsonl)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import hip, synth  # noqa: E402
from pyqsm_amd.tree_isolation import extend_seed_clusters, grow_seed_clusters  # noqa: E402

PHASES = ("grow_walk", "grow_commit", "grow_frontier")


def _quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, dtype=np.float64), [25, 50, 75])
    return {"q1": round(float(q1), 3), "median": round(float(med), 3), "q3": round(float(q3), 3), "n": len(v)}


def _wall(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def case(n, reps, cycles, k=200, radius=0.1):
    P = np.ascontiguousarray(synth.forest(n), dtype=np.float64)
    low = P[P[:, 2] < 0.3]
    lab, _ = hip.dbscan(low, 0.1, 10)
    seeds = [(int(c), low[lab == c]) for c in range(int(lab.max()) + 1)]
    kw = dict(k=k, max_distance=radius, cycles=cycles)
    host = lambda: extend_seed_clusters(seeds, P, engine="host", **kw)      # noqa: E731
    dev = lambda: extend_seed_clusters(seeds, P, engine="device", **kw)     # noqa: E731
    grow = lambda: grow_seed_clusters(seeds, P, **kw)                       # noqa: E731
    (h_pcds, h_nbrs), _ = _wall(host)                                       # warm-up, and the comparison
    (d_pcds, d_nbrs), _ = _wall(dev)
    same = (len(h_pcds) == len(d_pcds) and all(np.array_equal(a.points, b.points) for a, b in zip(h_pcds, d_pcds))
            and h_nbrs == d_nbrs)
    walls = {"host": [], "device": [], "device_growing_only": []}
    for _ in range(reps):
        walls["host"].append(_wall(host)[1])
        walls["device"].append(_wall(dev)[1])
        res, ms = _wall(grow)
        walls["device_growing_only"].append(ms)
    per = {p: [] for p in PHASES}
    hip.prof_enable(True)
    for _ in range(reps):
        hip.prof_reset()
        grow()
        for p in PHASES:
            per[p].append(hip.prof_get(p)[0])
    # the walk for scale: radius_mark with the largest frontier as queries (frontier c + 1 = the points of cycle c)
    acquired = np.bincount(res.cycle[res.cycle >= 0], minlength=1)
    frontiers = [int(sum(len(s) for _, s in seeds))] + acquired.tolist()
    big = int(np.argmax(acquired))
    q = res.src_points[res.cycle == big]
    mark_ms = []
    for _ in range(reps + 1):
        hip.prof_reset()
        hip.radius_mark(P, q, radius, k=k)
        mark_ms.append(hip.prof_get("radius_mark")[0])
    hip.prof_enable(False)
    stats = [int(v) for v in res.stats]
    walk = _quartiles(per["grow_walk"])
    mark = _quartiles(mark_ms[1:])
    rec = dict(n=n, seeds=len(seeds), seed_points=frontiers[0], k=k, radius=radius, cycles=cycles, outputs_equal=bool(same),
               cycles_run=stats[0], queries_served=stats[1], points_acquired=stats[2], largest_frontier=stats[3],
               finished=[int(v) for v in res.finished], frontier_per_cycle=frontiers[:stats[0]],
               wall_ms={name: _quartiles(v) for name, v in walls.items()},
               host_q1_over_device_median=round(_quartiles(walls["host"])["q1"] / _quartiles(walls["device"])["median"], 2),
               device_ms={p: _quartiles(v) for p, v in per.items()},
               device_ms_per_cycle={p: round(_quartiles(v)["median"] / max(stats[0], 1), 4) for p, v in per.items()},
               grow_walk_us_per_query=round(walk["median"] * 1e3 / max(stats[1], 1), 4),
               radius_mark_ms_largest_frontier=mark, radius_mark_queries=len(q),
               radius_mark_us_per_query=round(mark["median"] * 1e3 / max(len(q), 1), 4))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 5_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=150)
    ap.add_argument("--out", default=os.path.join("profiles", "grow_perf.jsonl"))
    a = ap.parse_args()
    for n in a.sizes:
        line = json.dumps(case(n, a.reps, a.cycles))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
