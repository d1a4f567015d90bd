"""A/B timing of the DBSCAN step (HBM-resident input) under environment switches:
    python tools/ab_dbscan.py [n] -- prints per-phase ms for each variant, interleaved.
    python tools/ab_dbscan.py [n] plan -- device-planned against host-planned grid
    (PYQSM_DBSCAN_PLAN=host), each with the profiling scopes on and off: wall ms per step
    over five interleaved rounds, then the median and range of every variant."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import hip, synth, _lib
_lib.require_gpu(0)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
variants = [("bucketed+f32", {}), ("bucketed f64", {"PYQSM_COORD_F32": "0"}), ("atomic  f64", {"PYQSM_DBSCAN_BIN": "atomic"})]
if len(sys.argv) > 2 and sys.argv[2] == "union":   # grid of the two wave-per-sub-cells passes
    variants = [("16,32 per CU", {}), ("bound grid", {"PYQSM_UNION_BLOCKS_PER_CU": "0"}), ("8,8 per CU", {"PYQSM_UNION_BLOCKS_PER_CU": "8"}),
                ("16,64 per CU", {"PYQSM_UNION_BLOCKS_PER_CU": "16,64"})]
if len(sys.argv) > 2 and sys.argv[2] == "plan":
    P = synth.forest(n)
    d_xyz = hip.DeviceBuffer.from_array(P)
    d_lab = hip.DeviceBuffer(n * 8); d_core = hip.DeviceBuffer(n)
    plan_variants = [("device plan, prof on ", {}, True), ("host plan,   prof on ", {"PYQSM_DBSCAN_PLAN": "host"}, True),
                     ("device plan, prof off", {}, False), ("host plan,   prof off", {"PYQSM_DBSCAN_PLAN": "host"}, False)]
    times = {name: [] for name, _, _ in plan_variants}
    ref = None
    for rnd in range(5):
        for name, env, prof in plan_variants:
            os.environ.pop("PYQSM_DBSCAN_PLAN", None)
            os.environ.update(env)
            for _ in range(3):
                hip.dbscan_dev(d_xyz.ptr, n, 0.1, 10, d_lab.ptr, d_core.ptr)
            hip.prof_enable(prof); hip.prof_reset()
            hip.sync()
            t = time.perf_counter()
            for _ in range(20):
                hip.dbscan_dev(d_xyz.ptr, n, 0.1, 10, d_lab.ptr, d_core.ptr)
            hip.sync(); dt = (time.perf_counter() - t) / 20
            hits = hip.prof_get("dbscan_plan_hit")[1] if prof else -1
            hip.prof_enable(False)
            times[name].append(dt * 1e3)
            lab = d_lab.download((n,), np.int64)
            if ref is None:
                ref = lab
            print(f"{name} step {dt*1e3:.4f} ms  plan hits {hits}/20  labels==first: {bool(np.array_equal(lab, ref))}",
                  flush=True)
    for name, v in times.items():
        print(f"{name} median {np.median(v):.4f} ms  range {min(v):.4f} .. {max(v):.4f}")
    sys.exit(0)
P = synth.forest(n)
d_xyz = hip.DeviceBuffer.from_array(P)
d_lab = hip.DeviceBuffer(n * 8); d_core = hip.DeviceBuffer(n)
ref = None
for rnd in range(3):
    for name, env in variants:
        for k in ("PYQSM_DBSCAN_BIN", "PYQSM_COORD_F32", "PYQSM_UNION_BLOCKS_PER_CU"):
            os.environ.pop(k, None)
        os.environ.update(env)
        for _ in range(3):
            hip.dbscan_dev(d_xyz.ptr, n, 0.1, 10, d_lab.ptr, d_core.ptr)
        hip.sync()
        hip.prof_enable(True); hip.prof_reset()
        t = time.perf_counter()
        for _ in range(20):
            hip.dbscan_dev(d_xyz.ptr, n, 0.1, 10, d_lab.ptr, d_core.ptr)
        hip.sync(); dt = (time.perf_counter() - t) / 20
        ph = {k: round(hip.prof_get(k)[0] / 20, 4) for k in ("dbscan_bin", "dbscan_core", "dbscan_union", "dbscan_label",
                                                             "k_core_tiled", "k_hook_sub", "k_union_sub")}
        hip.prof_enable(False)
        lab = d_lab.download((n,), np.int64)
        if ref is None:
            ref = lab
        print(f"{name:13s} step {dt*1e3:.3f} ms  {ph}  labels==first: {bool(np.array_equal(lab, ref))}", flush=True)
