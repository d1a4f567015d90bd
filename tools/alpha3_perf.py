"""The 3-D alpha shape at the project's cloud size: synth.forest(n) after clean_cloud at the config
defaults (voxel 0.04, neighbors 2, ratio 4, iters 3), at alpha = 2 and 4 mean nearest-neighbour distances, as one
segment and with one segment per tree unit (the points sorted by the forest's grid square). Per case: wall time
of geometry.hull.alpha_shapes (snapping and PCIe included) and HIP-event time of the scopes "alpha3_bin",
"alpha3_tris", "alpha3_volume" and "alpha3_sort", median and min of 3 runs after a warm-up; points, rows, volume
and area, the call's counters, and candidates, ball tests and estimated pair tests per second of "alpha3_tris".
Beside each radius, hip.ball_pivot on the same cloud and radius (normals from the 20 nearest within three mean
nearest-neighbour distances, oriented with k = 100): the nearest existing kernel, its "recon_tris" time and
counters. Nobody measured this kernel before and it has no parent: the numbers are a record, none is a pass
criterion. One JSON line per case, printed and appended to --out (default profiles/alpha3_perf.jsonl; "-"
prints only).

    python tools/alpha3_perf.py [--n points] [--out path]        (default: 1000000)
    python tools/alpha3_perf.py --resource-usage     (no GPU: hipcc's kernel-resource-usage remarks for
                                                     alpha3.hip -> profiles/alpha3_resource_usage.txt)
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
from pyqsm_amd.geometry import hull  # noqa: E402
from pyqsm_amd.geometry.cloud import KDTreeSearchParamHybrid, PointCloud, TriangleMesh  # noqa: E402

REPS = 3
SCOPES = ("alpha3_bin", "alpha3_tris", "alpha3_volume", "alpha3_sort")
RECON_SCOPES = ("recon_bin", "recon_tris", "recon_sort")
CAP = 1 << 62                                       # the measurement states its own cap
PITCH = 10.0                                        # synth.forest's grid of tree units


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


def _rates(st, ms):
    if not ms > 0:
        return {}
    return {k + "_per_s": round(st[v] / (ms * 1e-3), 1)
            for k, v in (("candidates", "candidates"), ("ball_tests", "tests"), ("estimated_pair_tests", "estimated_tests"))}


def alpha_case(name, pts, seg, alpha, avg):
    shapes, wall, dev = _timed(lambda: hull.alpha_shapes(pts, seg, alpha, max_tests=CAP), SCOPES)
    st = shapes[0].stats
    return dict(case=name, kernel="alpha_shape3", points=len(pts), segments=len(seg) - 1,
                mean_nn_distance=round(avg, 6), alpha=round(alpha, 6), quantum=shapes[0].quantum, rho2=shapes[0].rho2,
                rows=int(sum(len(s.triangles) for s in shapes)), unresolved_ties=shapes[0].n_unresolved_ties,
                volume=float(sum(s.volume for s in shapes)), area=float(sum(s.area for s in shapes)), stats=st,
                wall_ms=wall, scopes_ms=dev, **_rates(st, dev["alpha3_tris"]["median"]))


def pivot_case(name, cloud, alpha, avg):
    mesh, wall, dev = _timed(lambda: TriangleMesh.create_from_point_cloud_ball_pivoting(cloud, [alpha], max_tests=CAP),
                             RECON_SCOPES)
    st = mesh.stats
    return dict(case=name, kernel="ball_pivot", points=len(cloud.points), mean_nn_distance=round(avg, 6),
                alpha=round(alpha, 6), quantum=mesh.quantum, rows=len(mesh.triangles),
                unresolved_ties=mesh.n_unresolved_ties, stats=st, wall_ms=wall, scopes_ms=dev,
                **_rates(st, dev["recon_tris"]["median"]))


def resource_usage(path):
    """hipcc's -Rpass-analysis=kernel-resource-usage remarks for alpha3.hip, one block per kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "pyqsm_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-munsafe-fp-atomics", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
           "alpha3.hip", "-o", os.devnull]
    err = subprocess.run(cmd, cwd=src, check=True, capture_output=True, text=True).stderr
    keep = re.compile(r"remark: (?:\S+ )?\s*(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize|Occupancy|SGPRs Spill|"
                      r"VGPRs Spill|LDS Size)(.*?)(?:\s*\[-Rpass.*)?$")
    with open(path, "w") as f:
        for line in err.splitlines():
            m = keep.search(line)
            if m:
                f.write(("Name" if m.group(1) == "Function Name" else m.group(1)) + m.group(2).rstrip() + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join("profiles", "alpha3_perf.jsonl"),
                    help="file the records are appended to; - for none")
    ap.add_argument("--resource-usage", action="store_true",
                    help="write profiles/alpha3_resource_usage.txt from the compiler's remarks and stop")
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(os.path.join("profiles", "alpha3_resource_usage.txt"))
        return
    pts = hip.clean_cloud(synth.forest(a.n), 0.04, 2, 4, 3)
    # one segment per tree unit: the points sorted by the square of the forest's grid they stand in
    sq = np.floor(pts[:, :2] / PITCH + 0.5).astype(np.int64)
    tree = (sq[:, 1] - sq[:, 1].min()) * (sq[:, 0].max() - sq[:, 0].min() + 1) + sq[:, 0] - sq[:, 0].min()
    order = np.argsort(tree, kind="stable")
    pts, tree = pts[order], tree[order]
    seg_trees = np.concatenate([[0], np.cumsum(np.bincount(tree))]).astype(np.int64)
    seg_one = np.array([0, len(pts)], np.int64)
    cloud = PointCloud(pts)
    avg = float(np.mean(cloud.compute_nearest_neighbor_distance()))
    cloud.estimate_normals(search_param=KDTreeSearchParamHybrid(radius=3 * avg, max_nn=20))
    cloud.orient_normals_consistent_tangent_plane(100)

    def emit(rec):
        line = json.dumps(dict(rec, forest_points=a.n))
        print(line, flush=True)
        if a.out != "-":
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for k in (2, 4):
        emit(alpha_case(f"alpha_{k}_spacings", pts, seg_one, k * avg, avg))
        emit(alpha_case(f"alpha_{k}_spacings_per_tree", pts, seg_trees, k * avg, avg))
        emit(pivot_case(f"ball_pivot_{k}_spacings", cloud, k * avg, avg))


if __name__ == "__main__":
    main()
