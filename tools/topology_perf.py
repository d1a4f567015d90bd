"""Skeleton graph and cylinder table: the host stages of the existing wrappers against the
device stages, in one process on one sample. One JSON line per stage.

A `--points` synth forest (default 1 M) is contracted with extract_skeleton (`--iters` steps),
the artefact filter and the existing farthest-point sampling of extract_topology take it to a tenth,
and from that sample both paths are timed:

  host   extract_skeletal_graph + simplify_and_update (kNN on the device, SciPy's spanning tree,
         networkx chain collapse), then skeleton_to_QSM (Python loop over the cylinders);
  device hip.skeletal_forest + hip.collapse_chains through the *_dev entry points with the sample
         resident (what extract_topology_arrays does after its sampling), then skeleton_to_QSM_arrays.

Every figure is a host clock around a call that ends in a device synchronise (every entry point
synchronises before it returns), after one warm-up call of each path; `--reps` warm repeats, the two
paths alternating; median and quartiles. The per-phase device times (`*_ms`) are HIP-event times of the
library's profiling scopes, taken in a separate set of repeats with profiling on, so the wall times
are free of it. The two paths' outputs are compared on the spot: kept nodes, chain ends, member sets,
and every cylinder's surface rows bit for bit.

Per kernel: the same script under the profiler, in a run of its own (tracing slows the host, so
its wall times are not used), e.g.
    rocprofv3 --kernel-trace --stats -d out -o topo -- python tools/topology_perf.py --reps 2 --out ''
profiles/topology_kernel_stats.csv holds the calls and durations of this file's kernels from such a run.

    python tools/topology_perf.py [--points 1000000] [--iters 5] [--reps 5] [--out file]   (default profiles/topology_perf.jsonl)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import _lib, hip, synth  # noqa: E402
from pyqsm_amd.geometry import skeletonize as sk  # noqa: E402

PHASES = ("topo_knn", "topo_forest", "topo_forest_sort", "topo_chains", "topo_radii", "topo_surfaces")


def _stats(v):
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "q1_ms": round(float(q1), 3), "q3_ms": round(float(q3), 3),
            "runs": len(v)}


def _timed(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def device_topology(sample, k):
    """extract_topology_arrays from its sampling on: upload, forest, collapse, download."""
    m = len(sample)
    bufs = [hip.DeviceBuffer.from_array(sample)]
    try:
        for nbytes in (8 * (m - 1), 8 * (m - 1), 4 * m, 8 * (m - 1), 8 * m, 4 * m):
            bufs.append(hip.DeviceBuffer(nbytes))
        xyz, d_edges, d_d2, d_kept, d_ends, d_ptr, d_mem = bufs
        ne, rounds = hip.skeletal_forest_dev(xyz.ptr, m, k, d_edges.ptr, d_d2.ptr)
        nk, nc, nm = hip.collapse_chains_dev(d_edges.ptr, ne, m, d_kept.ptr, d_ends.ptr, d_ptr.ptr, d_mem.ptr)
        topo = sk.TopologyArrays(sample, np.arange(m, dtype=np.int32), d_edges.download((ne, 2), np.int32),
                                 np.sqrt(d_d2.download((ne,), np.float64)), d_kept.download((nk,), np.int32),
                                 d_ends.download((nc, 2), np.int32), d_ptr.download((nc + 1,), np.int64),
                                 d_mem.download((nm,), np.int32))
    finally:
        for b in bufs:
            b.free()
    return topo, rounds


def host_topology(sample, k):
    graph, _ = sk.extract_skeletal_graph(sample, k)
    tgraph, tpoints, mapping = sk.simplify_and_update(graph)
    return sk.LineSet(tpoints, list(tgraph.edges())), tgraph, graph


def compare(topo, host, shift):
    """The two paths on the same sample: same kept nodes, chain ends and member sets; and, from the
    device path's own topology, the same surface rows from both cylinder stages."""
    _, _, graph = host
    simp, _, kept_ref = sk.simplify_graph(graph)
    ref = {(min(a, b), max(a, b)): sorted(d.get("data", [])) for a, b, d in simp.edges(data=True)}
    got = {(int(a), int(b)): sorted(topo.members[topo.chain_ptr[c]:topo.chain_ptr[c + 1]].tolist())
           for c, (a, b) in enumerate(topo.chain_ends)}
    same_graph = sorted(kept_ref) == topo.kept.tolist() and got == ref
    _, cyls, _, radii = sk.skeleton_to_QSM(topo.topology, topo.to_networkx(), shift)
    qsm = sk.skeleton_to_QSM_arrays(topo, shift)
    ptr, pts = qsm["surface_ptr"], qsm["surface_points"]
    same_rows = len(cyls) == len(ptr) - 1 and all(
        np.array_equal(np.ascontiguousarray(pts[ptr[i]:ptr[i + 1]]).view(np.uint64),
                       np.ascontiguousarray(c.points).view(np.uint64)) for i, c in enumerate(cyls))
    rel = float(np.max(np.abs(qsm["radius"] - np.array(radii)) / np.array(radii))) if len(radii) else 0.0
    return {"same_kept_ends_members": bool(same_graph), "same_surface_rows": bool(same_rows),
            "max_rel_radius_difference": rel, "cylinders": len(cyls), "surface_points": int(len(pts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "topology_perf.jsonl"),
                    help="the JSON lines are appended to this file as well ('' for none)")
    a = ap.parse_args()
    _lib.require_gpu(0)                                   # no device, no measurement
    k = int(sk._SK["graph_k_n"])
    contracted, total, _ = sk.extract_skeleton(synth.forest(a.points, seed=0), max_iter=a.iters,
                                               termination_ratio=0.0)
    pts = sk.as_points(contracted)
    norms = np.linalg.norm(pts, axis=1)
    near = int(np.argmin(norms))
    if norms[near] <= 0.01:
        pts = pts[np.linalg.norm(pts - pts[near], axis=1) > 0.01]
    n_sample = min(max(int(len(pts) * 0.1), 15), len(pts))
    t_fps, (_, sample) = _timed(lambda: sk.farthest_point_down_sample(pts, n_sample))
    sample = np.ascontiguousarray(sample)
    lines = [{"case": "setup", "points": a.points, "contraction_steps": a.iters, "sample": len(sample),
              "graph_k_n": k, "fps_wall_ms": round(t_fps, 1)}]

    host = host_topology(sample, k)                       # warm-up of both paths
    topo, rounds = device_topology(sample, k)
    lines.append({"case": "parity", "boruvka_rounds": rounds, "forest_edges": int(len(topo.edges)),
                  "kept": int(len(topo.kept)), "chains": int(len(topo.chain_ends)), **compare(topo, host, total)})
    sk.skeleton_to_QSM(host[0], host[1], total)

    walls = {key: [] for key in ("host_graph", "device_graph", "host_qsm", "device_qsm", "device_qsm_no_surfaces")}
    for _ in range(a.reps):                               # alternating, profiling off
        walls["host_graph"].append(_timed(lambda: host_topology(sample, k))[0])
        walls["device_graph"].append(_timed(lambda: device_topology(sample, k))[0])
        walls["host_qsm"].append(_timed(lambda: sk.skeleton_to_QSM(host[0], host[1], total))[0])
        walls["device_qsm"].append(_timed(lambda: sk.skeleton_to_QSM_arrays(topo, total))[0])
        walls["device_qsm_no_surfaces"].append(
            _timed(lambda: sk.skeleton_to_QSM_arrays(topo, total, surfaces=False))[0])
    notes = {"host_graph": "extract_skeletal_graph + simplify_and_update",
             "device_graph": "upload + pyqsm_skeletal_forest_dev + pyqsm_collapse_chains_dev + download",
             "host_qsm": "skeleton_to_QSM", "device_qsm": "skeleton_to_QSM_arrays",
             "device_qsm_no_surfaces": "skeleton_to_QSM_arrays(surfaces=False)"}
    for key, v in walls.items():
        lines.append({"case": "wall", "stage": key, "what": notes[key], **_stats(v)})
    lines.append({"case": "ratio", "host_over_device_graph": round(
        float(np.median(walls["host_graph"]) / np.median(walls["device_graph"])), 2),
        "host_over_device_qsm": round(float(np.median(walls["host_qsm"]) / np.median(walls["device_qsm"])), 2)})

    phase = {p: [] for p in PHASES}
    hip.prof_enable(True)                                 # a separate set of repeats, event-timed
    for _ in range(a.reps):
        hip.prof_reset()
        device_topology(sample, k)
        sk.skeleton_to_QSM_arrays(topo, total)
        for p in PHASES:
            phase[p].append(hip.prof_get(p)[0])
    hip.prof_enable(False)
    for p in PHASES:
        lines.append({"case": "device_phase", "phase": p, **_stats(phase[p])})

    text = "\n".join(json.dumps(line) for line in lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
