"""Convex hull and points in boxes at the project's sizes. Hull inputs: the synthetic
forest of --points points as one cloud, the same split into its trees as one batched call, and a
100 000-point shell (points rounded from a sphere: nearly every one a hull vertex, the worst case).
Per input: wall time of hip.convex_hull on the lattice points (upload and host passes included) and
HIP-event time of the scopes "hull_prefilter", "hull_rounds" and "hull_sort", median and min of 3 runs
after a warm-up; candidates, rounds, facets, orient tests and tests per second of the "hull_rounds"
scope; beside them, on the same machine, the path the contraction loop takes today,
skeletonize.oriented_bounds(pts, device=0) (two fp64 filters and Qhull on the survivors), the device
path oriented_bounds(pts, device=0, hull="device") and plain scipy.spatial.ConvexHull(pts).
Boxes: hip.points_in_boxes for 1 and 256 boxes over --box-points points already in HBM, wall time and the
scopes "boxes_count" and "boxes_fill", GB/s of the 24 B-per-point stream (two passes). One JSON line per
case, printed and appended to --out (default profiles/hull_perf.jsonl; "-" prints only).

    python tools/hull_perf.py [--points n] [--box-points n] [--out path]
    python tools/hull_perf.py --resource-usage      (no GPU: hipcc's kernel-resource-usage remarks for
                                                    convex_hull.hip and boxes.hip -> profiles/hull_resource_usage.txt)
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import hip, synth  # noqa: E402
from pyqsm_amd.geometry import skeletonize  # noqa: E402
from pyqsm_amd.geometry.mesh_processing import quantize_mesh  # noqa: E402

REPS = 3
HULL_SCOPES = ("hull_prefilter", "hull_rounds", "hull_sort")
BOX_SCOPES = ("boxes_count", "boxes_fill")


def _median_min(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4)}


def _timed(fn, scopes=()):
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


def hull_case(name, pts, seg=None, host_paths=True):
    from scipy.spatial import ConvexHull
    ijk, q, _ = quantize_mesh(pts)
    r, wall, dev = _timed(lambda: hip.convex_hull(ijk, seg), HULL_SCOPES)
    rounds_ms = dev["hull_rounds"]["median"]       # both wraps; the prefilter's is a few dozen points per segment
    rec = dict(input=name, points=len(pts), segments=1 if seg is None else len(seg) - 1, quantum=q,
               triangles=int(r.tri_ptr[-1]), vertices=int(len(np.unique(r.tris))), stats=r.stats,
               hull_wall_ms=wall, hull_scopes_ms=dev,
               tests_per_s=round(r.stats["tests"] / (rounds_ms * 1e-3), 1) if rounds_ms > 0 else None)
    if host_paths:
        _, rec["filtered_qhull_wall_ms"], _ = _timed(lambda: skeletonize.oriented_bounds(pts, device=0))
        _, rec["device_bounds_wall_ms"], _ = _timed(lambda: skeletonize.oriented_bounds(pts, device=0, hull="device"))
        _, rec["qhull_wall_ms"], _ = _timed(lambda: ConvexHull(pts))
    return rec


def box_case(buf, n, boxes):
    (ptr, _), wall, dev = _timed(lambda: hip.points_in_boxes(buf, boxes), BOX_SCOPES)
    dev_ms = dev["boxes_count"]["median"] + dev["boxes_fill"]["median"]
    return dict(input="boxes", points=n, boxes=len(boxes), members=int(ptr[-1]), wall_ms=wall, scopes_ms=dev,
                stream_gb_per_s=round(2 * 24 * n * -(-len(boxes) // max(1, min(256, 0x7FFFFF00 // n))) / (dev_ms * 1e-3) / 1e9, 1)
                if dev_ms > 0 else None)


def resource_usage(path):
    """hipcc's -Rpass-analysis=kernel-resource-usage remarks for the two files, one block per kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "pyqsm_amd", "csrc")
    keep = re.compile(r"remark: (?:\S+ )?\s*(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize|Occupancy|SGPRs Spill|"
                      r"VGPRs Spill|LDS Size)(.*?)(?:\s*\[-Rpass.*)?$")
    with open(path, "w") as f:
        for name in ("convex_hull.hip", "boxes.hip"):
            cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                   "-munsafe-fp-atomics", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
                   name, "-o", os.devnull]
            err = subprocess.run(cmd, cwd=src, check=True, capture_output=True, text=True).stderr
            for line in err.splitlines():
                m = keep.search(line)
                if m:
                    f.write(("Name" if m.group(1) == "Function Name" else m.group(1)) + m.group(2).rstrip() + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--box-points", type=int, default=20_000_000)
    ap.add_argument("--out", default=os.path.join("profiles", "hull_perf.jsonl"),
                    help="file the records are appended to; - for none")
    ap.add_argument("--resource-usage", action="store_true",
                    help="write profiles/hull_resource_usage.txt from the compiler's remarks and stop")
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(os.path.join("profiles", "hull_resource_usage.txt"))
        return

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out != "-":
            with open(a.out, "a") as f:
                f.write(line + "\n")

    forest = synth.forest(a.points)
    units = max(1, int(round(a.points / synth.TREE_UNIT)))
    seg = np.minimum(np.arange(units + 1, dtype=np.int64) * (len(forest) // units), len(forest))
    seg[-1] = len(forest)
    emit(hull_case("forest", forest))
    emit(hull_case("forest_by_tree", forest, seg, host_paths=False))
    v = np.random.default_rng(7).normal(size=(100_000, 3))
    emit(hull_case("shell", np.rint(v / np.linalg.norm(v, axis=1)[:, None] * float(1 << 19))))
    rng = np.random.default_rng(8)
    n = a.box_points
    cloud = rng.uniform(-50.0, 50.0, (n, 3))
    boxes = np.zeros((256, 15))
    boxes[:, :3] = rng.uniform(-45.0, 45.0, (256, 3))
    for k in range(256):
        qm, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        boxes[k, 3:12] = qm.ravel()
    boxes[:, 12:] = rng.uniform(0.5, 3.0, (256, 3))
    buf = hip.DeviceBuffer.from_array(cloud)
    try:
        emit(box_case(buf, n, boxes[:1]))
        emit(box_case(buf, n, boxes))
    finally:
        buf.free()


if __name__ == "__main__":
    main()
