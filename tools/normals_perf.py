"""Normals, tangent-plane orientation and the stem stage on synth.forest clouds:
HIP-event time per phase (min and median of 5 runs), the wall time of every entry point (PCIe
included), the Boruvka round count, and CPU baselines: cKDTree (16 workers) plus batched
numpy.linalg.eigh for the normals, SciPy's minimum_spanning_tree for the orientation graph. The
GPU normals are compared with the restatement (tests/normals_restatement.py) at sizes up to
--check-normals points, the orientation and the stem route up to --check-orient points (the
restatement's Kruskal is a Python loop).

    python tools/normals_perf.py [n ...] [--check-normals N] [--check-orient N]
                                                         (default: 1000000 5000000; 1000000; 200000)
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import _lib, hip, synth  # noqa: E402
from tests import normals_restatement as R  # noqa: E402

RADIUS, NN, K, CUTOFF, REPS = 0.1, 30, 100, 10.0, 5
N_PHASES = ("normals_grid", "normals_cov", "normals_eig")
O_PHASES = ("orient_knn", "orient_min_edge", "orient_hook", "orient_jump", "orient_sign")
S_PHASES = ("stem_crop",) + N_PHASES + O_PHASES + ("stem_filter",)


def _digest(*arrays):
    """SHA-256 over the arrays' bytes (the first 24 hex digits): equal digests, equal bits."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:24]


def _runs(fn, phases):
    fn()                                                   # warm-up of every shape
    walls, per = [], {k: [] for k in phases}
    hip.prof_enable(True)
    for _ in range(REPS):
        hip.prof_reset()
        t = time.perf_counter()
        out = fn()
        walls.append((time.perf_counter() - t) * 1e3)
        for k in phases:
            per[k].append(hip.prof_get(k)[0])
    hip.prof_enable(False)
    stat = {k: {"min": round(min(v), 4), "median": round(float(np.median(v)), 4)} for k, v in per.items()}
    return out, {"wall_ms_min": round(min(walls), 3), "wall_ms_median": round(float(np.median(walls)), 3),
                 "phase_ms": stat}


def cpu_normals(P):
    from scipy.spatial import cKDTree
    t = time.perf_counter()
    d, idx = cKDTree(P).query(P, k=NN, distance_upper_bound=RADIUS, workers=16)
    ok = np.isfinite(d)
    idx = np.where(ok, idx, np.arange(len(P))[:, None])
    O = P[idx] - P[:, None, :]
    cnt = ok.sum(1)
    O = np.where(ok[..., None], O, 0.0)
    m = O.sum(1) / cnt[:, None]
    D = np.where(ok[..., None], O - m[:, None, :], 0.0)
    C = np.einsum("nki,nkj->nij", D, D) / cnt[:, None, None]
    np.linalg.eigh(C)
    return (time.perf_counter() - t) * 1e3


def cpu_mst(P, N):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    from scipy.spatial import cKDTree
    t = time.perf_counter()
    _, idx = cKDTree(P).query(P, k=K, workers=16)
    rows = np.repeat(np.arange(len(P)), K)
    cols = idx.reshape(-1)
    ok = rows != cols
    w = 1.0 - np.abs(np.sum(N[rows[ok]] * N[cols[ok]], axis=1)) + 1e-12
    minimum_spanning_tree(coo_matrix((w, (rows[ok], cols[ok])), shape=(len(P), len(P))).tocsr())
    return (time.perf_counter() - t) * 1e3


def measure(n, check_normals, check_orient, mst_max):
    P = synth.forest(n)
    N, nrm = _runs(lambda: hip.estimate_normals(P, RADIUS, NN), N_PHASES)
    rounds = hip.orient_normals_tangent_plane(P, N, K, return_rounds=True)[1]
    O, ori = _runs(lambda: hip.orient_normals_tangent_plane(P, N, K), O_PHASES)
    S, stem = _runs(lambda: hip.stem_cloud(P, RADIUS, NN, K, CUTOFF), S_PHASES)
    res = {"n": n, "estimate_normals": nrm, "orient_k100": dict(ori, boruvka_rounds=rounds),
           "stem_cloud": dict(stem, kept=len(S[0])),
           "sha256": {"normals": _digest(N), "oriented": _digest(O), "stem": _digest(*S)}, "cpu_normals_ms": round(cpu_normals(P), 1)}
    if n <= mst_max:
        res["cpu_scipy_mst_k100_ms"] = round(cpu_mst(P, N), 1)
    if n <= check_normals:
        res["normals_equal_restatement"] = bool(np.array_equal(N, R.estimate_normals(P, RADIUS, NN)))
    if n <= check_orient:
        res["orient_equal_restatement"] = bool(np.array_equal(O, R.orient_tangent_plane(P, N, K)))
        ri, rn = R.stem_route(P, RADIUS, NN, K, CUTOFF)
        res["stem_equal_restatement"] = bool(np.array_equal(S[0], ri) and np.array_equal(S[1], rn))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[1_000_000, 5_000_000])
    ap.add_argument("--check-normals", type=int, default=1_000_000)
    ap.add_argument("--check-orient", type=int, default=200_000)
    ap.add_argument("--mst-max", type=int, default=1_000_000)
    a = ap.parse_args()
    _lib.require_gpu(0)
    for n in a.sizes:
        print(json.dumps(measure(n, a.check_normals, a.check_orient, a.mst_max)), flush=True)


if __name__ == "__main__":
    main()
