"""Ball pivoting at the project's cloud size: synth.forest(n) after clean_cloud at the config
defaults (voxel 0.04, neighbors 2, ratio 4, iters 3), normals from the 20 nearest within three mean
nearest-neighbour distances, oriented with k = 100, as geometry.surf_recon.pivot_ball_mesh does. Two cases:
rho = 2 mean nearest-neighbour distances alone, and pyQSM's default factor list (eleven radii, 0.1 to 2).
Per case: wall time of TriangleMesh.create_from_point_cloud_ball_pivoting (snapping and PCIe included) and
HIP-event time of the scopes "recon_bin", "recon_tris", "recon_half_edges" and "recon_sort", median and min
of 3 runs after a warm-up; points, triangles, the call's counters, ball tests and estimated pair tests per
second of "recon_tris", and what mesh_topology says about the result. One JSON line per case, printed and
appended to --out (default profiles/recon_perf.jsonl; "-" prints only).

    python tools/recon_perf.py [--n points] [--out path]        (default: 1000000)
    python tools/recon_perf.py --resource-usage     (no GPU: hipcc's kernel-resource-usage remarks for
                                                    recon.hip -> profiles/recon_resource_usage.txt)
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
from pyqsm_amd.geometry.cloud import KDTreeSearchParamHybrid, PointCloud, TriangleMesh  # noqa: E402

REPS = 3
SCOPES = ("recon_bin", "recon_tris", "recon_half_edges", "recon_sort")
FACTORS = [0.1, 0.2, 0.3, 0.4, 0.5, 0.7, 1, 1.2, 1.5, 1.7, 2]


def _median_min(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4)}


def _timed(fn):
    fn()
    walls, per = [], {k: [] for k in SCOPES}
    hip.prof_enable(True)
    for _ in range(REPS):
        hip.prof_reset()
        t = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t) * 1e3)
        for k in SCOPES:
            per[k].append(hip.prof_get(k)[0])
    hip.prof_enable(False)
    return out, _median_min(walls), {k: _median_min(v) for k, v in per.items()}


def case(name, cloud, radii, avg):
    cap = 1 << 62                                   # the measurement states its own cap
    mesh, wall, dev = _timed(lambda: TriangleMesh.create_from_point_cloud_ball_pivoting(cloud, radii, max_tests=cap))
    ms = dev["recon_tris"]["median"]
    top = hip.mesh_topology(mesh.triangles, len(mesh.vertices)).summary
    st = mesh.stats
    return dict(case=name, points=len(cloud.points), mean_nn_distance=round(avg, 6), radii=[round(r, 6) for r in radii],
                quantum=mesh.quantum, triangles=len(mesh.triangles),
                triangles_per_level=np.bincount(mesh.triangle_levels, minlength=len(radii)).tolist(),
                unresolved_ties=mesh.n_unresolved_ties, stats=st, wall_ms=wall, scopes_ms=dev,
                ball_tests_per_s=round(st["tests"] / (ms * 1e-3), 1) if ms > 0 else None,
                estimated_pair_tests_per_s=round(st["estimated_tests"] / (ms * 1e-3), 1) if ms > 0 else None,
                topology={k: top[k] for k in ("edges", "boundary_edges", "over_two_edges", "non_manifold_vertices",
                                              "clusters", "orientable")})


def resource_usage(path):
    """hipcc's -Rpass-analysis=kernel-resource-usage remarks for recon.hip, one block per kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "pyqsm_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-munsafe-fp-atomics", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
           "recon.hip", "-o", os.devnull]
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
    ap.add_argument("--out", default=os.path.join("profiles", "recon_perf.jsonl"),
                    help="file the records are appended to; - for none")
    ap.add_argument("--resource-usage", action="store_true",
                    help="write profiles/recon_resource_usage.txt from the compiler's remarks and stop")
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(os.path.join("profiles", "recon_resource_usage.txt"))
        return
    cloud = PointCloud(hip.clean_cloud(synth.forest(a.n), 0.04, 2, 4, 3))
    avg = float(np.mean(cloud.compute_nearest_neighbor_distance()))
    cloud.estimate_normals(search_param=KDTreeSearchParamHybrid(radius=3 * avg, max_nn=20))
    cloud.orient_normals_consistent_tangent_plane(100)
    for name, radii in (("rho_2_spacings", [2 * avg]), ("factor_list", [f * avg for f in FACTORS])):
        line = json.dumps(dict(case(name, cloud, radii, avg), forest_points=a.n))
        print(line, flush=True)
        if a.out != "-":
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
