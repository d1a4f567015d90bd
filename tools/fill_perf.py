"""Hole filling at the project's mesh size. Two meshes:

  ball_pivot   synth.forest(n) after clean_cloud at the config values, ball-pivoted at two mean
               nearest-neighbour spacings (the mesh of tools/recon_perf.py, about 490 k triangles at
               n = 1 000 000): thousands of short holes, open chains at its non-manifold edges;
  tubes_128    5 000 open tubes with 128-gon rims: 10 000 loops of FILL_MAX_LOOP edges, the long class only.

Per mesh: wall time of hip.mesh_fill_holes (host checks and PCIe included) and HIP-event time of the scopes
"fill_table", "fill_successor", "fill_loops" and "fill_patches", median and min of 3 runs after a warm-up;
the statistics; the loops-per-length histogram. The CPU time is that of the NumPy / Python restatement of
the contract (tests/holes_restatement.py), one run, which is also compared with the device's output; no other
implementation (pymeshfix, Open3D, VTK) is installed here. On tubes_128 the restatement runs on the first
--cpu-tubes tubes only and its time per loop is reported, not extrapolated. One JSON line per mesh, printed
and appended to --out (default profiles/fill_perf.jsonl; "-" prints only).

    python tools/fill_perf.py [--n points] [--tubes count] [--cpu-tubes count] [--out path]
    python tools/fill_perf.py --resource-usage      (no GPU: hipcc's kernel-resource-usage remarks for the
                                                    kernels of holes.hip -> profiles/fill_resource_usage.txt)
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
from tests import holes_restatement as R  # noqa: E402

REPS = 3
SCOPES = ("fill_table", "fill_successor", "fill_loops", "fill_patches")


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


def tubes(count, L=hip.FILL_MAX_LOOP, seed=7):
    """`count` open tubes of two rings of L vertices each, z noisy along the rims: 2 * count loops of L edges."""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(L) / L
    ring = np.stack([np.cos(a), np.sin(a), 0 * a], axis=1)
    verts = np.concatenate([ring, ring * 1.1 + (0, 0, 1)])[None] + np.zeros((count, 1, 1))
    verts[:, :, 2] += 0.3 * rng.standard_normal((count, 2 * L))
    verts[:, :, 0] += 3.0 * np.arange(count)[:, None]
    i = np.arange(L)
    lo, lo1, hi, hi1 = i, (i + 1) % L, L + i, L + (i + 1) % L
    one = np.concatenate([np.stack([lo, lo1, hi1], 1), np.stack([lo, hi1, hi], 1)])
    tris = one[None] + (2 * L * np.arange(count))[:, None, None]
    return verts.reshape(-1, 3), tris.reshape(-1, 3).astype(np.int32)


def same(got, want):
    return bool(np.array_equal(got.ptr, want.ptr) and np.array_equal(got.verts, want.verts)
                and np.array_equal(got.flags, want.flags) and got.area.tobytes() == want.area.tobytes()
                and np.array_equal(got.new_tris, want.new_tris) and np.array_equal(got.new_loop, want.new_loop)
                and [got.stats[k] for k in hip._FILL_STATS] == want.stats.tolist())


def case(name, verts, tris, cpu_tris=None):
    verts = np.ascontiguousarray(verts, dtype=np.float64)
    got, wall, dev = _timed(lambda: hip.mesh_fill_holes(tris, verts))
    lengths = np.diff(got.ptr)
    rec = dict(mesh=name, triangles=len(tris), vertices=len(verts), stats=got.stats, new_rows=len(got.new_tris),
               loops_per_length={int(k): int(v) for k, v in zip(*np.unique(lengths, return_counts=True))},
               wall_ms=wall, scopes_ms=dev)
    sub = tris if cpu_tris is None else cpu_tris
    t = time.perf_counter()
    want = R.fill(sub, verts)
    cpu_ms = (time.perf_counter() - t) * 1e3
    ref = got if cpu_tris is None else hip.mesh_fill_holes(sub, verts)
    rec.update(cpu_restatement=dict(triangles=len(sub), loops=int(want.stats[1]), wall_ms=round(cpu_ms, 1),
                                    ms_per_loop=round(cpu_ms / max(1, int(want.stats[1])), 3)),
               equals_restatement=same(ref, want))
    return rec


def resource_usage(path):
    """hipcc's -Rpass-analysis=kernel-resource-usage remarks for the k_fill_* kernels of holes.hip."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "pyqsm_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-munsafe-fp-atomics", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
           "holes.hip", "-o", os.devnull]
    err = subprocess.run(cmd, cwd=src, check=True, capture_output=True, text=True).stderr
    keep = re.compile(r"remark: (?:\S+ )?\s*(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize|Occupancy|SGPRs Spill|"
                      r"VGPRs Spill|LDS Size)(.*?)(?:\s*\[-Rpass.*)?$")
    with open(path, "w") as f:
        on = False
        for line in err.splitlines():
            m = keep.search(line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                on = "k_fill" in m.group(2)      # not the shared half-edge kernels (profiles/mesh_resource_usage.txt)
            if on:
                f.write(("Name" if m.group(1) == "Function Name" else m.group(1)) + m.group(2).rstrip() + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--tubes", type=int, default=5000)
    ap.add_argument("--cpu-tubes", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "fill_perf.jsonl"),
                    help="file the records are appended to; - for none")
    ap.add_argument("--resource-usage", action="store_true",
                    help="write profiles/fill_resource_usage.txt from the compiler's remarks and stop")
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(os.path.join("profiles", "fill_resource_usage.txt"))
        return

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out != "-":
            with open(a.out, "a") as f:
                f.write(line + "\n")

    cloud = PointCloud(hip.clean_cloud(synth.forest(a.n), 0.04, 2, 4, 3))
    avg = float(np.mean(cloud.compute_nearest_neighbor_distance()))
    cloud.estimate_normals(search_param=KDTreeSearchParamHybrid(radius=3 * avg, max_nn=20))
    cloud.orient_normals_consistent_tangent_plane(100)
    mesh = TriangleMesh.create_from_point_cloud_ball_pivoting(cloud, [2 * avg], max_tests=1 << 62)
    emit(dict(case("ball_pivot", mesh.vertices, mesh.triangles.astype(np.int32)), forest_points=a.n))
    verts, tris = tubes(a.tubes)
    per_tube = 2 * hip.FILL_MAX_LOOP
    emit(case("tubes_128", verts, tris, cpu_tris=tris[:per_tube * min(a.cpu_tubes, a.tubes)]))


if __name__ == "__main__":
    main()
