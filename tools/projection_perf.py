"""Projected area on a synthetic crown: synth.forest(n) voxel-down-sampled, projected
onto the ground plane and quantised, at alpha = 2, 4 and 8 mean projected spacings (the mean distance
from a projected point to its nearest other one); project_in_slices and a 20-label project_by_label on
the largest cloud. Per case: wall time (host quantisation, PCIe and the host prelude included) and
HIP-event time of the "alpha_edges" scope (the directed-edge kernel) and the "alpha_bin" scope,
median and min of 3 runs after a warm-up (one more run with the boundary); estimated and executed
tests, tests per second of the edge kernel, the share of comparisons the 128-bit fallback decided,
merged duplicates. A case whose estimate exceeds the default max_tests is recorded as refused, with
the estimate. The CPU yardstick (--cpu; the crown is still down-sampled on the GPU) is
scipy.spatial.Delaunay plus the exact integer circumradius filter (what delaunay_filtered of
tests/alpha_restatement.py does, vectorised) on the same quantised points. pyvista / VTK, whose delaunay_2d the reference calls, is not installed where these
records were taken, so the reference's own time is not among them. One JSON line per case, printed
and appended to --out (default profiles/projection_perf.jsonl; "-" prints only).

    python tools/projection_perf.py [--sizes n ...] [--spacings k ...] [--voxel v]     (GPU cases)
    python tools/projection_perf.py --cpu [--sizes n ...] [--spacings k ...]           (yardstick)
                                                 (default: 100000 1000000; 2 4 8; 0.02)
    python tools/projection_perf.py --resource-usage      (no GPU: hipcc's kernel-resource-usage remarks
                                                 for alpha.hip -> profiles/projection_resource_usage.txt)
    bash tools/prof_kernels.sh projection tools/projection_perf.py --sizes 100000 --out -
                                                 (rocprofv3 --kernel-trace --stats around the 100 k cases
                                                 -> projection_kernel_stats.csv, kept under profiles/)
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
from pyqsm_amd import _lib, hip, synth  # noqa: E402
from pyqsm_amd.viz import projection as pj  # noqa: E402

REPS = 3


def _median_min(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4)}


def _timed(fn, scopes=("alpha_edges", "alpha_bin")):
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


def crown(n, voxel):
    """The cloud a caller would project: synth.forest(n) after voxel down-sampling on the GPU."""
    P = np.ascontiguousarray(synth.forest(n), dtype=np.float64)
    return np.asarray(hip.voxel_down_sample(P, voxel)[0], dtype=np.float64)


def spacing_of(ij):
    """(mean distance from a projected point to its nearest other one in lattice units, live points). The
    projection stacks points: stems are hundreds of times denser than the crown, and the bounding box's
    area per point says nothing about either."""
    from scipy.spatial import cKDTree
    U = np.unique(ij, axis=0).astype(np.float64)
    d, _ = cKDTree(U).query(U, k=2)
    return float(d[:, 1].mean()), len(U)


def gpu_case(pts, k):
    ij, q = pj.quantize_plane(pts)
    sp, live = spacing_of(ij)
    alpha = k * sp * q
    a2 = pj.lattice_a2(alpha, q)
    rep = dict(points=len(pts), live_points=live, quantum=q, mean_spacing=round(sp * q, 6), alpha=round(alpha, 6),
               alpha_spacings=k, A2=a2)
    try:
        res = hip.alpha_area(ij, a2)
    except _lib.PyQSMHipError as e:
        rep.update(refused=True, message=str(e))
        return rep
    st = res.stats
    _, wall, dev = _timed(lambda: pj.projected_area(pts, alpha))
    hip.prof_enable(True)
    hip.prof_reset()
    t = time.perf_counter()
    pj.projected_area(pts, alpha, return_boundary=True)
    wall_b = round((time.perf_counter() - t) * 1e3, 4)
    sort_ms = round(hip.prof_get("alpha_boundary_sort")[0], 4)
    hip.prof_enable(False)
    kernel_ms = dev["alpha_edges"]["median"]
    rep.update(area=res.twice_area[0] * q * q / 2, boundary_edges=int(res.n_boundary[0]), wall_ms=wall,
               kernel_ms=dev["alpha_edges"], bin_ms=dev["alpha_bin"], wall_ms_with_boundary=wall_b,
               boundary_sort_ms=sort_ms, estimated_tests=st["estimated_tests"],
               tests=st["tests"], directed_edges=st["edges"],
               tests_per_s=round(st["tests"] / (kernel_ms * 1e-3), 1) if kernel_ms > 0 else None,
               exact_fallbacks=st["exact_fallbacks"],
               exact_fallback_share=st["exact_fallbacks"] / max(st["tests"], 1),
               merged_duplicates=st["merged_duplicates"])
    return rep


def wrapper_cases(pts, k):
    ij, q = pj.quantize_plane(pts)
    alpha = k * spacing_of(ij)[0] * q
    m, wall, dev = _timed(lambda: pj.project_in_slices(pts, seed=0, alpha=alpha))
    yield dict(wrapper="project_in_slices", points=len(pts), alpha=round(alpha, 6), alpha_spacings=k,
               total_area=m["total_area"], wall_ms=wall, kernel_ms=dev["alpha_edges"], bin_ms=dev["alpha_bin"])
    lab = np.floor((pts[:, 0] - pts[:, 0].min()) / (np.ptp(pts[:, 0]) * (1 + 1e-9)) * 20).astype(np.int64)
    out, wall, dev = _timed(lambda: pj.project_by_label(pts, lab, alpha))
    yield dict(wrapper="project_by_label", labels=len(out["areas"]), points=len(pts), alpha=round(alpha, 6),
               alpha_spacings=k, total_area=out["total_area"], wall_ms=wall, kernel_ms=dev["alpha_edges"],
               bin_ms=dev["alpha_bin"])


def cpu_case(pts, k):
    from scipy.spatial import Delaunay
    ij, q = pj.quantize_plane(pts)
    sp, live = spacing_of(ij)
    a2 = pj.lattice_a2(k * sp * q, q)
    t0 = time.perf_counter()
    Q = np.unique(ij, axis=0).astype(np.int64)
    tri = Delaunay(Q.astype(np.float64)).simplices
    t1 = time.perf_counter()
    A, B, C = Q[tri[:, 0]], Q[tri[:, 1]], Q[tri[:, 2]]
    cr = ((B[:, 0] - A[:, 0]) * (C[:, 1] - A[:, 1]) - (B[:, 1] - A[:, 1]) * (C[:, 0] - A[:, 0])).astype(object)
    la, lb, lc = (((X - Y) ** 2).sum(axis=1).astype(object) for X, Y in ((B, A), (C, B), (A, C)))
    kept = la * lb * lc <= 4 * a2 * cr * cr
    twice = int(abs(cr[kept.astype(bool)]).sum())
    t2 = time.perf_counter()
    return dict(points=len(pts), live_points=live, alpha_spacings=k, A2=a2, area=twice * q * q / 2,
                delaunay_s=round(t1 - t0, 3), filter_s=round(t2 - t1, 3), total_s=round(t2 - t0, 3))


def resource_usage(path):
    """hipcc's -Rpass-analysis=kernel-resource-usage remarks for alpha.hip, one block per kernel."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "pyqsm_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-munsafe-fp-atomics", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
           "alpha.hip", "-o", os.devnull]
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
    ap.add_argument("--sizes", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--spacings", type=float, nargs="*", default=[2, 4, 8])
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--cpu", action="store_true", help="the scipy yardstick only")
    ap.add_argument("--out", default=os.path.join("profiles", "projection_perf.jsonl"),
                    help="file the records are appended to; - for none")
    ap.add_argument("--resource-usage", action="store_true",
                    help="write profiles/projection_resource_usage.txt from the compiler's remarks and stop")
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(os.path.join("profiles", "projection_resource_usage.txt"))
        return

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out != "-":
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for n in a.sizes:
        pts = crown(n, a.voxel)
        for k in a.spacings:
            head = {"n": n, "voxel": a.voxel}
            if a.cpu:
                emit({"case": "cpu_scipy_delaunay_filter", **head, **cpu_case(pts, k)})
            else:
                emit({"case": "gpu", **head, **gpu_case(pts, k)})
        if not a.cpu and n == max(a.sizes):
            for rep in wrapper_cases(pts, min(a.spacings)):
                emit({"case": "gpu_wrapper", "n": n, "voxel": a.voxel, **rep})


if __name__ == "__main__":
    main()
