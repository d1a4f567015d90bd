"""The colour path at the project's sizes: 1 M and 20 M 8-bit colours.
Per size: hip.hsv_segment with and without the member lists (all outputs, and classes only), the
histogram at (20, 1, 1) and (16, 16, 16), the two plain conversions and the white mask. For each the wall
time of the call (upload, download and host check included) and the HIP-event time of its kernel scopes,
median and min of 3 runs after a warm-up; beside them the byte model of each pass (the bytes it has to
read and write), the GB/s that gives over the kernel time and its share of the 6.29 TB/s a copy reaches
on one MI355X. CPU baseline on the same machine: matplotlib's rgb_to_hsv / hsv_to_rgb where it imports,
and the NumPy restatement of the whole segmentation (tests/color_restatement.py). One JSON line per case,
printed and appended to --out (default profiles/color_perf.jsonl; "-" prints only).

    python tools/color_perf.py [--sizes 1000000,20000000] [--out path]
    python tools/color_perf.py --resource-usage      (no GPU: hipcc's kernel-resource-usage remarks for
                                                      color.hip -> profiles/color_resource_usage.txt)
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyqsm_amd import hip  # noqa: E402
from pyqsm_amd.viz import color as vc  # noqa: E402
from tests import color_restatement as R  # noqa: E402

REPS = 3
HBM_COPY_GBS = 6290.0       # measured float4 copy on one MI355X


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


def _cpu(fn):
    t = time.perf_counter()
    fn()
    return round((time.perf_counter() - t) * 1e3, 2)


def case(name, n, fn, passes):
    """passes: {scope: bytes the pass reads and writes}."""
    _, wall, dev = _timed(fn, tuple(passes))
    rec = dict(case=name, colours=n, wall_ms=wall, scopes_ms=dev, model_bytes=passes, gb_per_s={}, hbm_share={})
    for k, b in passes.items():
        ms = dev[k]["median"]
        if ms > 0:
            rec["gb_per_s"][k] = round(b / (ms * 1e-3) / 1e9, 1)
            rec["hbm_share"][k] = round(b / (ms * 1e-3) / 1e9 / HBM_COPY_GBS, 3)
    return rec


def resource_usage(path):
    """hipcc's -Rpass-analysis=kernel-resource-usage remarks for color.hip, one block per kernel."""
    src = os.path.join(ROOT, "pyqsm_amd", "csrc")
    keep = re.compile(r"remark: (?:\S+ )?\s*(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize|Occupancy|SGPRs Spill|"
                      r"VGPRs Spill|LDS Size)(.*?)(?:\s*\[-Rpass.*)?$")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-munsafe-fp-atomics", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage", "-c",
           "color.hip", "-o", os.devnull]
    err = subprocess.run(cmd, cwd=src, check=True, capture_output=True, text=True).stderr
    with open(path, "w") as f:
        for line in err.splitlines():
            m = keep.search(line)
            if m:
                f.write(("Name" if m.group(1) == "Function Name" else m.group(1)) + m.group(2).rstrip() + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,20000000")
    ap.add_argument("--out", default=os.path.join("profiles", "color_perf.jsonl"),
                    help="file the records are appended to; - for none")
    ap.add_argument("--resource-usage", action="store_true",
                    help="write profiles/color_resource_usage.txt from the compiler's remarks and stop")
    a = ap.parse_args()
    if a.resource_usage:
        resource_usage(os.path.join("profiles", "color_resource_usage.txt"))
        return

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out != "-":
            with open(a.out, "a") as f:
                f.write(line + "\n")

    rules, closed = vc._rules(vc.DEFAULT_HUES)
    for n in (int(s) for s in a.sizes.split(",")):
        rgb = np.random.default_rng(7).integers(0, 256, (n, 3)) / 255.0
        row = 24 * n
        emit(case("segment_all_outputs", n, lambda: hip.hsv_segment(rgb, rules, closed),
                  {"hsv_segment": row + n + 2 * row, "hsv_members": n + 8 * n}))
        emit(case("segment_classes_and_members", n,
                  lambda: hip.hsv_segment(rgb, rules, closed, corrected=False, hsv=False),
                  {"hsv_segment": row + n, "hsv_members": n + 8 * n}))
        emit(case("segment_classes_only", n,
                  lambda: hip.hsv_segment(rgb, rules, closed, members=False, corrected=False, hsv=False),
                  {"hsv_segment": row + n}))
        for bins in ((20, 1, 1), (16, 16, 16)):
            emit(case("histogram_%dx%dx%d" % bins, n, lambda: hip.hsv_histogram(rgb, bins), {"hsv_hist": row}))
        emit(case("rgb_to_hsv", n, lambda: hip.rgb_to_hsv(rgb), {"pyqsm_rgb_to_hsv": 2 * row}))
        hsv = hip.rgb_to_hsv(rgb)
        emit(case("hsv_to_rgb", n, lambda: hip.hsv_to_rgb(hsv), {"pyqsm_hsv_to_rgb": 2 * row}))
        emit(case("mask_sum_gt", n, lambda: hip.color_mask(rgb), {"color_flags": row + 4 * n}))
        cpu = dict(case="cpu_baseline", colours=n,
                   restatement_segment_ms=_cpu(lambda: R.segment(rgb, rules, closed)),
                   restatement_rgb_to_hsv_ms=_cpu(lambda: R.rgb_to_hsv(rgb)),
                   histogramdd_16x16x16_ms=_cpu(lambda: np.histogramdd(hsv, (16, 16, 16), range=[(0, 1)] * 3)))
        try:
            from matplotlib.colors import hsv_to_rgb, rgb_to_hsv
            cpu["matplotlib_rgb_to_hsv_ms"] = _cpu(lambda: rgb_to_hsv(rgb))
            cpu["matplotlib_hsv_to_rgb_ms"] = _cpu(lambda: hsv_to_rgb(hsv))
        except ImportError:
            cpu["matplotlib_rgb_to_hsv_ms"] = cpu["matplotlib_hsv_to_rgb_ms"] = None
        emit(cpu)


if __name__ == "__main__":
    main()
