"""Inputs and the comparison shared by tests/test_allhits_host.py (the mirror oracle on the CPU) and
tests/test_gpu_rays_all_hits.py (the HIP all-hits path): every crossing that list_intersections
reports, and every one it does not, against the INDEPENDENT fp64 evaluation of oracle/ray_f64.c
(signed volumes, another formulation than the kernels' Moller-Trumbore) over ALL ray x triangle pairs.

What is held (the constants are those of tests/test_gpu_rays_f64.py, imported, not restated):
  structure  counts is the per-ray histogram of ray_ids and sums to the number of records; records
             strictly ascend in (ray id, triangle id), so no pair is listed twice; ids in range.
  hit/miss   a pair on which the list and fp64 (pierces and t > 0) disagree must be explained in
             double precision: the smallest barycentric weight within EDGE_TOL of 0 (the crossing
             lies on an edge or vertex up to what fp32 resolves), or |t| <= DEPTH_TOL (a crossing
             at the ray origin). Their number is bounded by MAX_DISAGREE of the fp64 hits.
  t          on agreeing pairs |t - t64| / t64 <= T_RTOL for steep hits that are not near, and the
             same bound on the error across the triangle's plane (relative to max(distance,
             NEAR * diagonal)) for every hit, grazing and near ones included.
  u, v       the point (1-u-v) v0 + u v1 + v v2 against the same point from the fp64 weights,
             <= UV_POINT_RTOL of the distance on steep hits: the bound that file holds on the hit
             point (an error du in u moves the point by du * |e1|, which fp32 Moller-Trumbore keeps
             near eps32 * |o - v0|, far inside it).
The cases are built once per process from fixed seeds, cast to float32 first, and are read-only."""
import functools

import numpy as np

import oracle
from pyqsm_amd import synth

from tests.test_gpu_rays_f64 import DEPTH_TOL, EDGE_TOL, GRAZING, NEAR, T_RTOL

UV_POINT_RTOL = 2e-5         # the bound of tests/test_gpu_rays_f64.py on the reconstructed hit point
MAX_DISAGREE = 0.002         # share of the fp64 hits that may disagree (each one explained)
N_RAYS = 2049                # one more than two chunks of the 64-bit offset scan
KEYS = ("counts", "ray_ids", "primitive_ids", "t_hit", "primitive_uvs")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def general_rays(verts, n, seed):
    """Differing origins and directions: origins around the mesh's box, aimed at points in it."""
    rng = np.random.default_rng(seed)
    lo, hi = verts.min(0), verts.max(0)
    o = rng.uniform(lo - 2, hi + 2, (n, 3))
    target = rng.uniform(lo, hi, (n, 3))
    return _f32(np.concatenate([o, target - o], axis=1))


def _sun():
    v, t = synth.canopy_mesh(600, seed=2, side=0.5)
    return v, t, synth.sun_rays(v, N_RAYS)


def _sun_low():
    v, t = synth.canopy_mesh(600, seed=2, side=0.5)
    return v, t, synth.sun_rays(v, N_RAYS, elevation_deg=12.0, azimuth_deg=200.0)


def _general():
    v, t = synth.canopy_mesh(600, seed=3, side=0.5)
    return v, t, general_rays(v, N_RAYS, seed=1)


CASES = {"sun": _sun, "sun_low": _sun_low, "general": _general}


@functools.lru_cache(maxsize=None)
def case(name):
    """(verts f32 [V,3], tris i32 [T,3], rays f32 [R,6]) — read-only, shared between tests."""
    v, t, r = CASES[name]()
    out = (_f32(v), np.ascontiguousarray(t, dtype=np.int32), _f32(r))
    for a in out:
        a.setflags(write=False)
    return out


def fp64_all_pairs(verts, tris, rays):
    """oracle.ray_tri_pairs_f64 on every (ray, triangle) pair: (pierces & t > 0 bool, t f64,
    bary f64 [.., 3]), each [R, T] (row = ray). NaN where the fp64 volumes vanish together."""
    rays = _f32(rays).reshape(-1, 6)
    R, T = len(rays), len(tris)
    if R == 0 or T == 0:
        return np.zeros((R, T), bool), np.full((R, T), np.nan), np.full((R, T, 3), np.nan)
    pierces, t, bary = oracle.ray_tri_pairs_f64(verts, tris, np.repeat(rays, T, axis=0),
                                                np.tile(np.arange(T, dtype=np.int64), R))
    t = t.reshape(R, T)
    with np.errstate(invalid="ignore"):
        hit = pierces.reshape(R, T) & (t > 0)
    return hit, t, bary.reshape(R, T, 3)


def structure_violations(result, R, T):
    """The ways in which `result` is not a well-formed list over R rays and T triangles."""
    bad = []
    counts, rid, pid = result["counts"], result["ray_ids"], result["primitive_ids"]
    n = len(rid)
    if counts.shape != (R,):
        return [f"counts has shape {counts.shape}, not ({R},)"]
    if not (len(pid) == n and result["t_hit"].shape == (n,) and result["primitive_uvs"].shape == (n, 2)):
        return ["record arrays differ in length"]
    if int(counts.astype(np.int64).sum()) != n:
        bad.append(f"counts sum to {int(counts.astype(np.int64).sum())}, {n} records")
    if n and (int(rid.max()) >= R or int(pid.max()) >= T):
        return bad + ["a ray or triangle id is out of range"]
    if not np.array_equal(np.bincount(rid.astype(np.int64), minlength=R), counts):
        bad.append("counts is not the per-ray histogram of ray_ids")
    key = rid.astype(np.int64) * max(T, 1) + pid.astype(np.int64)
    step = np.diff(key)
    if (step == 0).any():
        bad.append(f"{int((step == 0).sum())} duplicate (ray, triangle) records")
    if (step < 0).any():
        bad.append(f"records not ascending in (ray id, triangle id) at {int(np.argmax(step < 0))}")
    return bad


def compare_all_hits(result, verts, tris, rays):
    """`result` (the dict of hip.list_intersections / oracle.list_intersections) against fp64 on all
    pairs. Returns the record; :func:`check_record` asserts the bounds on it."""
    rays = _f32(rays).reshape(-1, 6)
    R, T = len(rays), len(tris)
    rec = {"rays": R, "pairs": R * T, "listed": int(len(result["ray_ids"])),
           "structure": structure_violations(result, R, T)}
    hit64, t64, b64 = fp64_all_pairs(verts, tris, rays)
    rec["fp64_hits"] = int(hit64.sum())
    rid, pid = result["ray_ids"].astype(np.int64), result["primitive_ids"].astype(np.int64)
    if len(rid) != len(pid) or (len(rid) and (rid.max() >= R or pid.max() >= T)):
        return rec                                     # reported above; nothing below can be indexed
    if not (len(result["t_hit"]) == len(result["primitive_uvs"]) == len(rid)):
        return rec
    listed = np.zeros((R, T), bool)
    listed[rid, pid] = True
    # ---- disagreements, each explained in double precision
    dis = listed != hit64
    with np.errstate(invalid="ignore"):
        on_edge = np.abs(b64.min(axis=2)) <= EDGE_TOL  # NaN (vanishing volumes) explains nothing
        at_origin = np.abs(t64) <= DEPTH_TOL
    unexplained = dis & ~(on_edge | at_origin)
    rec.update(disagreements=int(dis.sum()), unexplained=int(unexplained.sum()),
               unexplained_pairs=[tuple(map(int, p)) for p in np.argwhere(unexplained)[:8]])
    # ---- agreeing pairs: t, then u and v
    same = hit64[rid, pid]
    r_, p_ = rid[same], pid[same]
    rec["same"] = int(same.sum())
    if not len(r_):
        return rec
    t32 = result["t_hit"][same].astype(np.float64)
    uv32 = result["primitive_uvs"][same].astype(np.float64)
    tt, bb = t64[r_, p_], b64[r_, p_]
    tv = verts[tris[p_]].astype(np.float64)
    d = rays[r_, 3:].astype(np.float64)
    nrm = np.cross(tv[:, 1] - tv[:, 0], tv[:, 2] - tv[:, 0])
    cosang = np.abs((nrm * d).sum(1)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(d, axis=1))
    dist = tt * np.linalg.norm(d, axis=1)
    near_len = NEAR * float(np.linalg.norm(verts.astype(np.float64).max(0) - verts.astype(np.float64).min(0)))
    steep = (cosang >= GRAZING) & (dist >= near_len)
    rel = np.abs(t32 - tt) / tt
    across = rel * cosang * dist / np.maximum(dist, near_len)
    pt64 = (bb[:, :, None] * tv).sum(1)
    w32 = np.stack([1.0 - uv32[:, 0] - uv32[:, 1], uv32[:, 0], uv32[:, 1]], axis=1)
    dpt = np.linalg.norm((w32[:, :, None] * tv).sum(1) - pt64, axis=1) / dist
    rec.update(grazing_or_near=int((~steep).sum()),
               max_rel_t_plain=float(rel[steep].max()) if steep.any() else 0.0,
               max_rel_t_all=float(rel.max()), max_rel_t_across_plane=float(across.max()),
               max_abs_uv=float(np.abs(uv32 - bb[:, 1:]).max()),
               max_rel_uv_point=float(dpt[steep].max()) if steep.any() else 0.0)
    return rec


def check_record(rec):
    """The conditions every case must meet."""
    assert rec["structure"] == [], rec["structure"]
    assert rec["unexplained"] == 0, (rec["unexplained"], rec["unexplained_pairs"])
    assert rec["disagreements"] <= MAX_DISAGREE * rec["fp64_hits"], (rec["disagreements"], rec["fp64_hits"])
    assert rec["same"] > 0.1 * rec["rays"], rec["same"]             # the case exercises real hits
    assert rec["max_rel_t_plain"] <= T_RTOL, rec["max_rel_t_plain"]
    assert rec["max_rel_t_across_plane"] <= T_RTOL, rec["max_rel_t_across_plane"]
    assert rec["max_rel_uv_point"] <= UV_POINT_RTOL, rec["max_rel_uv_point"]


def copy_result(result):
    return {k: np.array(result[k]) for k in KEYS}


def split_by_ray(result):
    """Record indices [begin, end) of every ray, from `counts` alone."""
    end = np.cumsum(result["counts"].astype(np.int64))
    return end - result["counts"], end
