"""Detail recovery: voxel-grid occupancy of full-resolution tiles and the fused neighbour
reduction. One JSON line per case.

Occupancy: the grid of one tree of synth.forest (every fourth of its points) at voxel sizes 0.1 and
0.02, queried by tiles of 5 M and 20 M points of the whole forest. Wall time of the host form (the
tile crosses PCIe in chunks; `included` comes back) and HIP-event time of the query kernel, median and
min of 5 runs after a warm-up, queries per second and the bytes a query moves at the least (24 B read,
1 B written) against the kernel's time. A third tile lies wholly inside the tree's box (the tree's
points repeated with 5 cm of jitter): every query reaches the lookup. The records of case
"occupancy_gpu_ab" in profiles/detail_perf.jsonl come from this loop run once per lookup while the
library still held both, the binary search over sorted voxel keys and the block table;
the binary search lost and was removed, so the tool now times the one lookup there is. Yardstick with
--cpu (needs no GPU): the NumPy restatement, sorted keys plus searchsorted. It is not Open3D, whose
check_if_included does one hash lookup per point on one thread.

Transfer: the mean of F = 1 and 8 value columns over the neighbours (k = 500, r = 0.05) of m = 1 M
points of a forest in every fourth of them, by hip.radius_reduce and by the route it replaces:
hip.radius_knn's padded [m, 500] tables brought to the host in chunks and reduced there with NumPy
(over the columns up to the chunk's longest neighbour list only, which favours the yardstick).

    python tools/detail_perf.py [--tiles n ...] [--voxels v ...] [--queries m] [--skip-transfer]
    python tools/detail_perf.py --cpu [--tiles n ...] [--voxels v ...]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyqsm_amd import hip, synth  # noqa: E402

REPS = 5


def _median_min(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4)}


def numpy_grid(comp, size):
    origin = comp.min(axis=0) - size * 0.5
    k3 = np.floor((comp - origin) / size).astype(np.int64)
    dims = k3.max(axis=0) + 1
    return origin, dims, np.unique(k3[:, 0] + dims[0] * (k3[:, 1] + dims[1] * k3[:, 2]))


def numpy_included(origin, dims, keys, size, tile):
    f3 = np.floor((tile - origin) / size)
    box = np.all((f3 >= 0) & (f3 < dims), axis=1)
    k3 = f3[box].astype(np.int64)
    k = k3[:, 0] + dims[0] * (k3[:, 1] + dims[1] * k3[:, 2])
    pos = np.minimum(np.searchsorted(keys, k), len(keys) - 1)
    inc = np.zeros(len(tile), dtype=bool)
    inc[np.flatnonzero(box)[keys[pos] == k]] = True
    return inc, box


def in_box_tile(tree, n):
    """n queries inside one tree's box: its points repeated, each copy jittered by up to 5 cm (the
    search cloud of tree_isolation.py:465-475 is of this kind: the clusters' own surroundings)."""
    rng = np.random.default_rng(7)
    reps = -(-n // len(tree))
    return (np.tile(tree, (reps, 1))[:n] + rng.uniform(-0.05, 0.05, (n, 3))).astype(np.float32).astype(np.float64)


def occupancy_gpu(tile, comp, size, kind="forest"):
    want, box = numpy_included(*numpy_grid(comp, size), size, tile)
    rep = dict(tile=kind, queries=len(tile), grid_points=len(comp), voxel_size=size, included=int(want.sum()),
               in_box_not_included=int((box & ~want).sum()), outside_box=int((~box).sum()))
    with hip.VoxelGrid(comp, size) as g:
        rep.update(voxels=g.n_voxels, dims=g.dims.tolist(), device_bytes=g.device_bytes)
        assert np.array_equal(g.query(tile), want)    # warm-up and check
        walls, kern = [], []
        hip.prof_enable(True)
        for _ in range(REPS):
            hip.prof_reset()
            t = time.perf_counter()
            g.query(tile)
            walls.append((time.perf_counter() - t) * 1e3)
            kern.append(hip.prof_get("voxgrid_query")[0])
        hip.prof_enable(False)
        k_ms = float(np.median(kern))
        rep.update(wall_ms=_median_min(walls), kernel_ms=_median_min(kern),
                   queries_per_s_kernel=round(len(tile) / (k_ms * 1e-3), 1) if k_ms > 0 else None,
                   queries_per_s_wall=round(len(tile) / (float(np.median(walls)) * 1e-3), 1), min_bytes_per_query=25,
                   gb_per_s_at_min_bytes=round(25 * len(tile) / (k_ms * 1e-3) / 1e9, 1) if k_ms > 0 else None)
    return rep


def occupancy_cpu(tile, comp, size):
    t = time.perf_counter()
    grid = numpy_grid(comp, size)
    build = time.perf_counter() - t
    times = []
    for _ in range(3):
        t = time.perf_counter()
        inc, _ = numpy_included(*grid, size, tile)
        times.append((time.perf_counter() - t) * 1e3)
    return dict(queries=len(tile), grid_points=len(comp), voxel_size=size, voxels=len(grid[2]), included=int(inc.sum()),
                build_ms=round(build * 1e3, 3), query_ms=_median_min(times),
                queries_per_s=round(len(tile) / (float(np.median(times)) * 1e-3), 1),
                note="NumPy restatement (sorted keys + searchsorted), not Open3D")


def table_route(src, qry, vals, radius, k, chunk):
    """The route the fused call replaces: padded tables to the host, np.mean over the real entries."""
    n, F = vals.shape
    out = np.empty((len(qry), F))
    for r0 in range(0, len(qry), chunk):
        dist, idx = hip.radius_knn(src, qry[r0:r0 + chunk], radius, k=k)
        real = idx < n
        cnt = real.sum(axis=1)
        kmax = max(int(cnt.max()), 1)
        real, idx = real[:, :kmax], idx[:, :kmax]
        g = vals[np.where(real, idx, 0)] * real[..., None]
        with np.errstate(invalid="ignore", divide="ignore"):
            o = g.sum(axis=1) / cnt[:, None]
        o[cnt == 0] = vals[0]
        out[r0:r0 + chunk] = o
    return out


def transfer_gpu(m, F, radius=0.05, k=500, chunk=100_000):
    qry = synth.forest(m, seed=3)
    src = np.ascontiguousarray(qry[::4])
    vals = np.random.default_rng(F).normal(size=(len(src), F))
    fused, cnt = hip.radius_reduce(src, qry, vals, radius, k=k, return_counts=True)   # warm-up
    walls, kern = [], []
    hip.prof_enable(True)
    for _ in range(3):
        hip.prof_reset()
        t = time.perf_counter()
        hip.radius_reduce(src, qry, vals, radius, k=k)
        walls.append((time.perf_counter() - t) * 1e3)
        kern.append(hip.prof_get("radius_reduce")[0])
    hip.prof_enable(False)
    table_route(src, qry[:chunk], vals, radius, k, chunk)                            # warm-up
    t = time.perf_counter()
    tab = table_route(src, qry, vals, radius, k, chunk)
    table_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter()
    for r0 in range(0, m, chunk):
        hip.radius_knn(src, qry[r0:r0 + chunk], radius, k=k)
    tables_only_ms = (time.perf_counter() - t) * 1e3
    scale = np.abs(vals).max() * k * 2.0 ** -52
    return dict(queries=m, sources=len(src), F=F, k=k, radius=radius, empty=int((cnt == 0).sum()),
                mean_neighbours=round(float(cnt.mean()), 2), max_neighbours=int(cnt.max()),
                fused_wall_ms=_median_min(walls), fused_kernel_ms=_median_min(kern),
                table_route_wall_ms=round(table_ms, 1), table_route_tables_only_wall_ms=round(tables_only_ms, 1),
                table_bytes_per_query=k * 16, fused_bytes_per_query=24 + 8 * F,
                table_over_fused_wall=round(table_ms / float(np.median(walls)), 2),
                max_abs_difference=float(np.abs(fused - tab).max()), difference_bound=float(scale),
                sha256=hashlib.sha256(fused.tobytes() + cnt.tobytes()).hexdigest()[:24],
                note="table route: hip.radius_knn in chunks of %d queries + NumPy mean over the real entries" % chunk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, nargs="*", default=[5_000_000, 20_000_000])
    ap.add_argument("--voxels", type=float, nargs="*", default=[0.1, 0.02])
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--skip-transfer", action="store_true")
    ap.add_argument("--skip-occupancy", action="store_true")
    ap.add_argument("--cpu", action="store_true", help="the NumPy yardstick of the occupancy cases; needs no GPU")
    a = ap.parse_args()
    if not a.skip_occupancy:
        for n in a.tiles:
            tile = synth.forest(n)
            comp = np.ascontiguousarray(tile[:synth.TREE_UNIT:4])
            for size in a.voxels:
                if a.cpu:
                    print(json.dumps({"case": "occupancy_cpu_numpy", **occupancy_cpu(tile, comp, size)}), flush=True)
                else:
                    print(json.dumps({"case": "occupancy_gpu", **occupancy_gpu(tile, comp, size)}), flush=True)
    if not a.cpu and not a.skip_occupancy:
        tree = synth.forest(synth.TREE_UNIT)
        tile = in_box_tile(tree, min(a.tiles))
        for size in a.voxels:
            print(json.dumps({"case": "occupancy_gpu", **occupancy_gpu(tile, np.ascontiguousarray(tree[::4]), size,
                                                                       "in_box")}), flush=True)
    if not a.cpu and not a.skip_transfer:
        for F in a.features:
            print(json.dumps({"case": "transfer_gpu", **transfer_gpu(a.queries, F)}), flush=True)


if __name__ == "__main__":
    main()
