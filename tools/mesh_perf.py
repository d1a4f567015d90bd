"""Mesh checks at the project's canopy size: synth.canopy_mesh(n), an unwelded soup of
square leaves (every leaf its own four vertices, so n / 2 clusters of two triangles), and one welded
closed surface of about the same number of triangles (a bumpy torus: one cluster, watertight).
Per mesh: wall time of hip.mesh_topology (with areas) and of hip.mesh_self_intersections (host
checks and PCIe included) and HIP-event time of the scopes "mesh_edge_sort", "mesh_union",
"mesh_clusters" and "mesh_sweep", median and min of 3 runs after a warm-up; the sweep's counters and
box tests per second of the "mesh_sweep" scope: one whole sweep of all pairs, the exact tests of the box
survivors included (they run inline); a second sweep after a pair list that did not fit is timed apart
as "mesh_sweep_rerun" and recorded as sweep_passes = 2. One JSON line per mesh, printed and appended to --out
(default profiles/mesh_perf.jsonl; "-" prints only).

    python tools/mesh_perf.py [--tris n] [--out path]           (default: 500000)
    python tools/mesh_perf.py --resource-usage      (no GPU: hipcc's kernel-resource-usage remarks for
                                                    mesh.hip -> profiles/mesh_resource_usage.txt)
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
from pyqsm_amd.geometry import mesh_processing as mp  # noqa: E402

REPS = 3
TOPOLOGY_SCOPES = ("mesh_edge_sort", "mesh_union", "mesh_clusters")
SWEEP_SCOPES = ("mesh_sweep", "mesh_sweep_rerun", "mesh_pair_sort")


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


def torus(n_tris):
    """A welded, closed, bumpy torus of about n_tris triangles (m x m quads)."""
    m = max(3, int(round((n_tris / 2) ** 0.5)))
    u, v = np.meshgrid(2 * np.pi * np.arange(m) / m, 2 * np.pi * np.arange(m) / m, indexing="ij")
    r = 1.5 + 0.1 * np.sin(5 * u) * np.cos(7 * v)
    x, y, z = (4 + r * np.cos(v)) * np.cos(u), (4 + r * np.cos(v)) * np.sin(u), 9 + r * np.sin(v)
    verts = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    a, b = i * m + j, ((i + 1) % m) * m + j
    c, d = ((i + 1) % m) * m + (j + 1) % m, i * m + (j + 1) % m
    tris = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return verts, tris.astype(np.int32)


def case(name, verts, tris):
    verts = np.asarray(verts, dtype=np.float64)
    top, wall_t, dev_t = _timed(lambda: hip.mesh_topology(tris, len(verts), verts), TOPOLOGY_SCOPES)
    ijk, q, _ = mp.quantize_mesh(verts)
    cap = len(tris) * (len(tris) - 1) // 2         # the measurement states its own cap: this many pairs
    hits, wall_s, dev_s = _timed(lambda: hip.mesh_self_intersections(ijk, tris, max_tests=cap), SWEEP_SCOPES)
    sweep_ms = dev_s["mesh_sweep"]["median"]
    considered = hits.stats["pairs_considered"]
    return dict(mesh=name, triangles=len(tris), vertices=len(verts), quantum=q, summary=top.summary,
                topology_wall_ms=wall_t, topology_scopes_ms=dev_t, sweep_wall_ms=wall_s, sweep_scopes_ms=dev_s,
                sweep_stats=hits.stats, sweep_passes=2 if dev_s["mesh_sweep_rerun"]["median"] > 0 else 1,
                box_tests_per_s=round(considered / (sweep_ms * 1e-3), 1) if sweep_ms > 0 else None)


def resource_usage(path):
    """hipcc's -Rpass-analysis=kernel-resource-usage remarks for mesh.hip, one block per kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "pyqsm_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-munsafe-fp-atomics", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
           "mesh.hip", "-o", os.devnull]
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
    ap.add_argument("--tris", type=int, default=500_000)
    ap.add_argument("--out", default=os.path.join("profiles", "mesh_perf.jsonl"),
                    help="file the records are appended to; - for none")
    ap.add_argument("--resource-usage", action="store_true",
                    help="write profiles/mesh_resource_usage.txt from the compiler's remarks and stop")
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(os.path.join("profiles", "mesh_resource_usage.txt"))
        return
    for name, (verts, tris) in (("canopy_soup", synth.canopy_mesh(a.tris)), ("welded_torus", torus(a.tris))):
        line = json.dumps(case(name, verts, tris))
        print(line, flush=True)
        if a.out != "-":
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
