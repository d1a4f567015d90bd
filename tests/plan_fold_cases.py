"""Clouds and calls of tests/test_gpu_dbscan_plan_fold.py. Run as a program (python -m tests.plan_fold_cases, from
the repository's root) it makes the calls that need a context without a shape hint: a process of its own,
because contexts are kept per thread and handed on with their hint when a thread ends, so only a process
that has started no other thread can tell that a thread's context is new. Every size runs in a thread of
its own, kept alive to the end; one JSON line per size."""
import json
import sys
import threading

import numpy as np

EPS, MIN_PTS = 0.1, 10
# around the blocks of k_bbox (256 points a block and sweep), of k_bk_hist (2048 points), and more points
# than one sweep of k_bbox covers (256 threads in twice as many blocks as a MI355X has compute units)
SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 256 * 512 + 257)


def _f32(P):
    return np.ascontiguousarray(P, dtype=np.float64).astype(np.float32).astype(np.float64)


def cloud(n):
    """n points with fp32 values, uniform in a cube with three points per eps^3: about twelve neighbours
    inside, fewer at the faces, so that min_pts = 10 splits the cloud."""
    side = EPS * (n / 3.0) ** (1.0 / 3.0)
    return _f32(np.random.default_rng(n).uniform(0.0, side, (n, 3)))


# three points in one cell: the smallest grid there is (27 cells), for a hint that every larger cloud outgrows
TINY = np.array([[0.0, 0.0, 0.0], [0.0625, 0.0, 0.0], [0.0, 0.0625, 0.0]])


def counted(fn, gpu=0):
    """fn() with the phase counters on: (its result, plan hits, plan misses)."""
    from pyqsm_amd import hip
    hip.prof_enable(True, gpu)
    try:
        hip.prof_reset(gpu)
        out = fn()
        hit = hip.prof_get("dbscan_plan_hit", gpu)[1]
        miss = hip.prof_get("dbscan_plan_miss", gpu)[1]
    finally:
        hip.prof_enable(False, gpu)
    return out, hit, miss


def _fresh(n, results, ready, done):
    import oracle
    from pyqsm_amd import hip
    try:
        P = cloud(n)
        lab0, core0 = oracle.dbscan(P, EPS, MIN_PTS)
        calls = []
        for _ in range(2):
            (lab, core), hit, miss = counted(lambda: hip.dbscan(P, EPS, MIN_PTS))
            calls.append({"hit": hit, "miss": miss,
                          "equal": bool(np.array_equal(lab, lab0) and np.array_equal(core, core0))})
        results[n] = calls
    finally:
        ready.set()
    done.wait()          # the context stays this thread's: the next thread gets a new one


if __name__ == "__main__":
    from pyqsm_amd import _lib
    _lib.require_gpu(0)
    results, done, threads = {}, threading.Event(), []
    for n in SIZES:
        ready = threading.Event()
        t = threading.Thread(target=_fresh, args=(n, results, ready, done))
        t.start()
        threads.append(t)
        ready.wait()
        if n not in results:
            break
        print(json.dumps({"n": n, "calls": results[n]}), flush=True)
    done.set()
    for t in threads:
        t.join()
    sys.exit(0 if len(results) == len(SIZES) else 1)
