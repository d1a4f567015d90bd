"""NumPy-facing calls into libpyqsm_hip.so.

One thin function per C-ABI entry point: validates shapes/dtypes, hands plain
pointers to the library, raises :class:`pyqsm_amd._lib.PyQSMHipError` on failure.
No computation happens in Python here.
"""
from __future__ import annotations

import ctypes
import weakref
from typing import NamedTuple

import numpy as np

from . import _lib
from ._lib import check, i64, i32, dbl, vp

MISS_PRIM = np.uint32(0xFFFFFFFF)


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _points(points) -> np.ndarray:
    pts = np.ascontiguousarray(np.asarray(points), dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"expected points of shape [n,3], got {pts.shape}")
    return pts


# ---------------------------------------------------------------- device buffers

class DeviceBuffer:
    """A block of HBM owned by the caller, for the *_dev entry points."""

    def __init__(self, nbytes: int, device: int = 0):
        self.device = int(device)
        self.nbytes = int(nbytes)
        ptr = vp()
        check(_lib.load().pyqsm_dev_malloc(self.device, self.nbytes, ctypes.byref(ptr)))
        self.ptr = ptr.value

    @classmethod
    def from_array(cls, a: np.ndarray, device: int = 0) -> "DeviceBuffer":
        a = np.ascontiguousarray(a)
        buf = cls(a.nbytes, device)
        buf.upload(a)
        return buf

    def upload(self, a: np.ndarray) -> None:
        a = np.ascontiguousarray(a)
        if a.nbytes > self.nbytes:
            raise ValueError("array larger than device buffer")
        check(_lib.load().pyqsm_h2d(self.device, self.ptr, _p(a), a.nbytes))

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        if out.nbytes > self.nbytes:
            raise ValueError("requested more bytes than the device buffer holds")
        check(_lib.load().pyqsm_d2h(self.device, _p(out), self.ptr, out.nbytes))
        return out

    def free(self) -> None:
        if self.ptr:
            _lib.load().pyqsm_dev_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def sync(device: int = 0) -> None:
    check(_lib.load().pyqsm_sync(int(device)))


def prof_enable(on, device: int = 0) -> None:
    """0 / False off; 1 / True phase timers; 2 also single solver kernels and counters."""
    check(_lib.load().pyqsm_prof_enable(int(device), int(on)))


def prof_reset(device: int = 0) -> None:
    check(_lib.load().pyqsm_prof_reset(int(device)))


def prof_get(name: str, device: int = 0):
    """(total milliseconds, launches) recorded under `name` since the last reset."""
    ms, cnt = dbl(0.0), i64(0)
    check(_lib.load().pyqsm_prof_get(int(device), name.encode(), ctypes.byref(ms),
                                     ctypes.byref(cnt)))
    return ms.value, cnt.value


# ---------------------------------------------------------------- ray casting

def _mesh(verts, tris):
    v = np.ascontiguousarray(np.asarray(verts), dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(np.asarray(tris), dtype=np.int32).reshape(-1, 3)
    return v, t


def cast_rays(verts, tris, rays, device: int = 0):
    """Closest hit. Returns t_hit f32 (+inf = miss), primitive_ids u32
    (0xFFFFFFFF = miss), primitive_uvs f32 [...,2]; leading shape follows `rays`."""
    v, t = _mesh(verts, tris)
    r = np.ascontiguousarray(np.asarray(rays), dtype=np.float32)
    if r.shape[-1] != 6:
        raise ValueError(f"rays must have last dimension 6, got {r.shape}")
    lead = r.shape[:-1]
    r2 = r.reshape(-1, 6)
    R = r2.shape[0]
    t_hit = np.empty(R, dtype=np.float32)
    prim = np.empty(R, dtype=np.uint32)
    uv = np.empty((R, 2), dtype=np.float32)
    check(_lib.load().pyqsm_cast_rays(_p(v), v.shape[0], _p(t), t.shape[0], _p(r2), R,
                                      _p(t_hit), _p(prim), _p(uv), int(device)))
    return t_hit.reshape(lead), prim.reshape(lead), uv.reshape(lead + (2,))


def cast_rays_multi(verts, tris, rays, n_devices: int = 0, with_uv: bool = True):
    """The same closest-hit sweep on ``n_devices`` GPUs driven from this one process
    (``pyqsm_cast_rays_multi``: mesh replicated by RCCL broadcast, rays in contiguous shards,
    results all-gathered; 0 = every visible GPU). No torch involved. Returns what
    :func:`cast_rays` returns, bit for bit (``with_uv=False``: uv is None and half the bytes
    are gathered)."""
    v, t = _mesh(verts, tris)
    r = np.ascontiguousarray(np.asarray(rays), dtype=np.float32)
    if r.shape[-1] != 6:
        raise ValueError(f"rays must have last dimension 6, got {r.shape}")
    lead = r.shape[:-1]
    r2 = r.reshape(-1, 6)
    R = r2.shape[0]
    t_hit = np.empty(R, dtype=np.float32)
    prim = np.empty(R, dtype=np.uint32)
    uv = np.empty((R, 2), dtype=np.float32) if with_uv else None
    check(_lib.load().pyqsm_cast_rays_multi(_p(v), v.shape[0], _p(t), t.shape[0], _p(r2), R,
                                            _p(t_hit), _p(prim), _p(uv) if with_uv else None,
                                            int(n_devices)))
    return t_hit.reshape(lead), prim.reshape(lead), uv.reshape(lead + (2,)) if with_uv else None


def list_intersections(verts, tris, rays, device: int = 0):
    """Every crossing with t > 0, ordered by ray id then triangle id."""
    v, t = _mesh(verts, tris)
    r = np.ascontiguousarray(np.asarray(rays), dtype=np.float32).reshape(-1, 6)
    R = r.shape[0]
    lib = _lib.load()
    counts = np.zeros(R, dtype=np.int32)
    total = i64(0)
    check(lib.pyqsm_list_intersections(_p(v), v.shape[0], _p(t), t.shape[0], _p(r), R, _p(counts),
                                       None, None, None, None, 0, ctypes.byref(total),
                                       int(device)))
    n = int(total.value)
    ray_ids = np.empty(n, dtype=np.uint32)
    prim = np.empty(n, dtype=np.uint32)
    ts = np.empty(n, dtype=np.float32)
    uv = np.empty((n, 2), dtype=np.float32)
    if n:
        check(lib.pyqsm_list_intersections(_p(v), v.shape[0], _p(t), t.shape[0], _p(r), R,
                                           _p(counts), _p(ray_ids), _p(prim), _p(ts), _p(uv), n,
                                           ctypes.byref(total), int(device)))
    return {"ray_ids": ray_ids, "primitive_ids": prim, "t_hit": ts, "primitive_uvs": uv,
            "counts": counts}


def point_mesh_distance(verts, tris, queries, device: int = 0):
    """(dist f32 [Q], prim u32 [Q]): unsigned distance to the mesh and the closest triangle."""
    v, t = _mesh(verts, tris)
    q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 3)
    dist = np.empty(q.shape[0], dtype=np.float32)
    prim = np.empty(q.shape[0], dtype=np.uint32)
    check(_lib.load().pyqsm_point_mesh_distance(_p(v), v.shape[0], _p(t), t.shape[0], _p(q), q.shape[0],
                                                _p(dist), _p(prim), int(device)))
    return dist, prim


class DeviceMesh:
    """A mesh expanded into the sweep's 48-byte records, resident in HBM."""

    def __init__(self, verts, tris, device: int = 0):
        v, t = _mesh(verts, tris)
        self.device = int(device)
        self.n_tris = t.shape[0]
        dv = DeviceBuffer.from_array(v, device) if v.size else None
        dt = DeviceBuffer.from_array(t, device) if t.size else None
        self.records = DeviceBuffer(max(1, self.n_tris) * 48, device)
        if self.n_tris:
            check(_lib.load().pyqsm_expand_tris_dev(dv.ptr, v.shape[0], dt.ptr, self.n_tris,
                                                    self.records.ptr, self.device))
            sync(device)
        for b in (dv, dt):
            if b is not None:
                b.free()


def cast_rays_dev(mesh: DeviceMesh, rays_ptr: int, n_rays: int, t_hit_ptr: int, prim_ptr: int,
                  uv_ptr: int | None = None) -> None:
    """Asynchronous sweep over HBM-resident rays (pointers are device addresses)."""
    check(_lib.load().pyqsm_cast_rays_dev(mesh.records.ptr, mesh.n_tris, rays_ptr, int(n_rays),
                                          t_hit_ptr, prim_ptr, uv_ptr, mesh.device))


# ---------------------------------------------------------------- DBSCAN / kNN

def dbscan(points, eps: float, min_pts: int, device: int = 0, radius_inclusive: bool = True):
    """labels int64 [n] (-1 = noise), core mask bool [n]. ``radius_inclusive=False``: the strict
    neighbourhood d2 < eps^2 (``pyqsm_dbscan_ex``) instead of scikit-learn's d2 <= eps^2."""
    pts = _points(points)
    n = pts.shape[0]
    labels = np.empty(n, dtype=np.int64)
    core = np.zeros(n, dtype=np.uint8)
    check(_lib.load().pyqsm_dbscan_ex(_p(pts), n, float(eps), int(min_pts), int(bool(radius_inclusive)),
                                      _p(labels), _p(core), int(device)))
    return labels, core.astype(bool)


def dbscan_dev(xyz_ptr: int, n: int, eps: float, min_pts: int, labels_ptr: int,
               core_ptr: int | None = None, device: int = 0, want_count: bool = False,
               radius_inclusive: bool = True):
    """Asynchronous clustering of an HBM-resident cloud; returns the cluster count
    when `want_count` (that read-back synchronises)."""
    cnt = i64(0)
    check(_lib.load().pyqsm_dbscan_dev_ex(xyz_ptr, int(n), float(eps), int(min_pts),
                                          int(bool(radius_inclusive)), labels_ptr, core_ptr,
                                          ctypes.byref(cnt) if want_count else None, int(device)))
    return int(cnt.value) if want_count else None


def octant_directory(points, eps: float, device: int = 0, cap: int = 1 << 25):
    """The cell directory DBSCAN bins ``points`` with at ``eps``, read out on the device (for tests):
    ``dims`` int32 [3] (cells per axis, borders included) and ``begin`` int32 [prod(dims) + 1],
    ``begin[c]`` = points in cells with id < c. Grids of more than ``cap`` entries: PYQSM_ERANGE."""
    pts = _points(points)
    dims = np.zeros(3, dtype=np.int32)
    begin = np.empty(int(cap), dtype=np.int32)
    check(_lib.load().pyqsm_octant_directory(_p(pts), pts.shape[0], float(eps), _p(dims), _p(begin), int(cap),
                                             int(device)))
    return dims, begin[: int(np.prod(dims.astype(np.int64))) + 1].copy()


class CoreRamp(NamedTuple):
    lo: np.float32
    hi: np.float32
    K: np.float32
    A: np.float32
    B: np.float32
    usable: bool


def core_ramp_constants(eps: float, radius_inclusive: bool = True) -> CoreRamp:
    """The fp32 thresholds and ramp constants of DBSCAN's core pass at ``eps`` (for tests; no GPU)."""
    out = np.zeros(6, dtype=np.float32)
    check(_lib.load().pyqsm_core_ramp_constants(float(eps), int(bool(radius_inclusive)), _p(out)))
    return CoreRamp(out[0], out[1], out[2], out[3], out[4], bool(out[5] != 0))


def core_ramp_probe(d, eps: float, radius_inclusive: bool = True, device: int = 0):
    """(s_in, s_hi) float32 [n]: the core pass's two ramps of the squared distances ``d``, on the device."""
    d = np.ascontiguousarray(np.asarray(d), dtype=np.float32).reshape(-1)
    s_in = np.empty_like(d)
    s_hi = np.empty_like(d)
    check(_lib.load().pyqsm_core_ramp_probe(_p(d), d.shape[0], float(eps), int(bool(radius_inclusive)),
                                            _p(s_in), _p(s_hi), int(device)))
    return s_in, s_hi


def knn(points, k: int, exclude_self: bool = True, device: int = 0):
    """idx int32 [n,k], squared distances float64 [n,k], ascending by (d2, index)."""
    pts = _points(points)
    n = pts.shape[0]
    idx = np.empty((n, int(k)), dtype=np.int32)
    d2 = np.empty((n, int(k)), dtype=np.float64)
    check(_lib.load().pyqsm_knn(_p(pts), n, int(k), int(bool(exclude_self)), _p(idx), _p(d2),
                                int(device)))
    return idx, d2


def knn_dev(xyz_ptr: int, n: int, k: int, exclude_self: bool, idx_ptr: int, d2_ptr: int,
            device: int = 0) -> None:
    check(_lib.load().pyqsm_knn_dev(xyz_ptr, int(n), int(k), int(bool(exclude_self)), idx_ptr,
                                    d2_ptr, int(device)))


# ---------------------------------------------------------------- RANSAC

SHAPES = {"circle": 0, "cylinder": 1}


def ransac(points, triples, shape: str = "circle", thresh: float = 0.2, device: int = 0):
    """center[3], axis[3], radius, inliers int64 (ascending), winning row (-1: none)."""
    pts = _points(points)
    tri = np.ascontiguousarray(np.asarray(triples), dtype=np.int64).reshape(-1, 3)
    n, H = pts.shape[0], tri.shape[0]
    if H and (tri.min() < 0 or tri.max() >= n):
        raise ValueError("sample index outside the point set")
    center = np.zeros(3)
    axis = np.zeros(3)
    radius = dbl(0.0)
    inl = np.empty(max(n, 1), dtype=np.int64)
    n_in, best = i64(0), i64(-1)
    check(_lib.load().pyqsm_ransac(_p(pts), n, _p(tri), H, SHAPES[shape], float(thresh),
                                   _p(center), _p(axis), ctypes.byref(radius), _p(inl),
                                   ctypes.byref(n_in), ctypes.byref(best), int(device)))
    return center, axis, radius.value, inl[:n_in.value].copy(), int(best.value)


def ransac_batch(points, seg_start, triples, shape: str = "circle", thresh: float = 0.2, device: int = 0):
    """``pyqsm_ransac_batch``: S point sets stacked in ``points`` (``seg_start`` int64 [S+1]), H
    hypotheses each (``triples`` int64 [S,H,3], indices local to the set). Returns ``(centers [S,3],
    axes [S,3], radii [S], inliers list of S int64 arrays (ascending, local), best int64 [S])``."""
    pts = _points(points)
    ss = np.ascontiguousarray(seg_start, dtype=np.int64)
    S = len(ss) - 1
    tri = np.ascontiguousarray(np.asarray(triples), dtype=np.int64).reshape(S, -1, 3)
    H = tri.shape[1]
    sizes = np.diff(ss)
    if H and S:
        ok = (tri >= 0).all(axis=(1, 2)) | (sizes < 3)
        if not ok.all() or (tri.max(axis=(1, 2)) >= np.maximum(sizes, 1))[sizes >= 3].any():
            raise ValueError("sample index outside its point set")
    centers = np.zeros((S, 3))
    axes = np.zeros((S, 3))
    radii = np.zeros(S)
    inl = np.empty(max(pts.shape[0], 1), dtype=np.int64)
    n_in = np.zeros(S, dtype=np.int64)
    best = np.full(S, -1, dtype=np.int64)
    check(_lib.load().pyqsm_ransac_batch(_p(pts), pts.shape[0], _p(ss), S, _p(tri), H, SHAPES[shape],
                                         float(thresh), _p(centers), _p(axes), _p(radii), _p(inl), _p(n_in),
                                         _p(best), int(device)))
    ends = np.cumsum(n_in)
    inliers = [inl[e - c:e].copy() for c, e in zip(n_in, ends)]
    return centers, axes, radii, inliers, best


def ransac_models(points, triples, device: int = 0):
    """f64 [H,8] = (cx,cy,cz, ax,ay,az, r, valid)."""
    pts = _points(points)
    tri = np.ascontiguousarray(np.asarray(triples), dtype=np.int64).reshape(-1, 3)
    models = np.zeros((tri.shape[0], 8))
    check(_lib.load().pyqsm_ransac_models(_p(pts), pts.shape[0], _p(tri), tri.shape[0],
                                          _p(models), int(device)))
    return models


def ransac_count(points, models, shape: str = "circle", thresh: float = 0.2, device: int = 0):
    """Inlier count of every hypothesis, int32 [H]."""
    pts = _points(points)
    m = np.ascontiguousarray(models, dtype=np.float64).reshape(-1, 8)
    counts = np.zeros(m.shape[0], dtype=np.int32)
    check(_lib.load().pyqsm_ransac_count(_p(pts), pts.shape[0], _p(m), m.shape[0], SHAPES[shape],
                                         float(thresh), _p(counts), int(device)))
    return counts


# ---------------------------------------------------------------- plane segmentation

def _plane_samples(samples) -> np.ndarray:
    smp = np.ascontiguousarray(np.asarray(samples), dtype=np.int64)
    if smp.ndim != 2:
        raise ValueError(f"expected samples of shape [H,m], got {smp.shape}")
    return smp


def _plane_axis(axis):
    if axis is None:
        return None
    ax = np.ascontiguousarray(np.asarray(axis, dtype=np.float64).reshape(3))
    return ax


def plane_models(points, samples, axis=None, cos_limit: float = 0.0, device: int = 0):
    """``pyqsm_plane_models``: the hypothesis planes f64 [H,4] = (a, b, c, d) of ``samples`` int64
    [H,m]; invalid hypotheses are rows of zeros. ``axis`` (unit) and ``cos_limit`` > 0 restrict the
    normals to a cone."""
    pts = _points(points)
    smp = _plane_samples(samples)
    H, m = smp.shape
    ax = _plane_axis(axis)
    planes = np.zeros((H, 4))
    check(_lib.load().pyqsm_plane_models(_p(pts), pts.shape[0], _p(smp), H, m, _p(ax), float(cos_limit),
                                         _p(planes), int(device)))
    return planes


def plane_count(points, planes, thresh: float, device: int = 0):
    """``pyqsm_plane_count``: int32 [H], the points strictly within ``thresh`` of every plane."""
    pts = _points(points)
    pl = np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 4)
    counts = np.zeros(pl.shape[0], dtype=np.int32)
    check(_lib.load().pyqsm_plane_count(_p(pts), pts.shape[0], _p(pl), pl.shape[0], float(thresh), _p(counts),
                                        int(device)))
    return counts


def segment_plane(points, samples, thresh: float, probability: float = 0.99999999, axis=None,
                  cos_limit: float = 0.0, device: int = 0):
    """``pyqsm_segment_plane``: ``(plane_fit [4], plane_hyp [4], inliers int64 ascending, best, used)``."""
    pts = _points(points)
    smp = _plane_samples(samples)
    H, m = smp.shape
    ax = _plane_axis(axis)
    fit, hyp = np.zeros(4), np.zeros(4)
    inl = np.empty(max(pts.shape[0], 1), dtype=np.int64)
    n_in, best, used = i64(0), i64(-1), i64(0)
    check(_lib.load().pyqsm_segment_plane(_p(pts), pts.shape[0], _p(smp), H, m, float(thresh), float(probability),
                                          _p(ax), float(cos_limit), _p(fit), _p(hyp), _p(inl), ctypes.byref(n_in),
                                          ctypes.byref(best), ctypes.byref(used), int(device)))
    return fit, hyp, inl[:n_in.value].copy(), int(best.value), int(used.value)


class PlaneSegments:
    """What ``segment_planes`` found: ``planes`` f64 [k,4] (refitted), ``hypothesis_planes`` f64 [k,4],
    ``labels`` int32 [n] (the plane of every point, -1: none), ``counts`` / ``best`` / ``used`` int64
    [k]."""

    def __init__(self, planes, hypothesis_planes, labels, counts, best, used):
        self.planes = planes
        self.hypothesis_planes = hypothesis_planes
        self.labels = labels
        self.counts = counts
        self.best = best
        self.used = used

    def __len__(self):
        return len(self.planes)

    def indices(self, i: int) -> np.ndarray:
        """The points of plane ``i``: int64, ascending."""
        return np.flatnonzero(self.labels == int(i)).astype(np.int64)

    def rest(self) -> np.ndarray:
        """The points on no plane: int64, ascending."""
        return np.flatnonzero(self.labels < 0).astype(np.int64)

    def __repr__(self):
        return f"PlaneSegments with {len(self.planes)} planes over {len(self.labels)} points."


def segment_planes(points, draws, thresh: float, probability: float = 0.99999999, min_inliers: int = 1,
                   axis=None, cos_limit: float = 0.0, device: int = 0) -> PlaneSegments:
    """``pyqsm_segment_planes``: up to P planes peeled off the cloud on the device; ``draws`` uint64
    [P,H,m] (sample j of hypothesis h in round r is alive point ``mulhi64(draws[r,h,j], n_alive)``)."""
    pts = _points(points)
    dr = np.ascontiguousarray(np.asarray(draws), dtype=np.uint64)
    if dr.ndim != 3:
        raise ValueError(f"expected draws of shape [P,H,m], got {dr.shape}")
    P, H, m = dr.shape
    ax = _plane_axis(axis)
    n = pts.shape[0]
    labels = np.full(max(n, 1), -1, dtype=np.int32)
    fit, hyp = np.zeros((max(P, 1), 4)), np.zeros((max(P, 1), 4))
    counts = np.zeros(max(P, 1), dtype=np.int64)
    best = np.full(max(P, 1), -1, dtype=np.int64)
    used = np.zeros(max(P, 1), dtype=np.int64)
    k = i64(0)
    check(_lib.load().pyqsm_segment_planes(_p(pts), n, _p(dr), P, H, m, float(thresh), float(probability),
                                           int(min_inliers), _p(ax), float(cos_limit), _p(labels), _p(fit), _p(hyp),
                                           _p(counts), _p(best), _p(used), ctypes.byref(k), int(device)))
    k = int(k.value)
    return PlaneSegments(fit[:k].copy(), hyp[:k].copy(), labels[:n], counts[:k].copy(), best[:k].copy(),
                         used[:k].copy())


# ---------------------------------------------------------------- contraction solve

def _csr(L):
    """(indptr i32, indices i32, data f64, n) of a scipy sparse matrix or a
    (indptr, indices, data) triple."""
    if isinstance(L, tuple):
        indptr, indices, data = L
    else:
        L = L.tocsr()
        L.sort_indices()
        indptr, indices, data = L.indptr, L.indices, L.data
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.float64)
    return indptr, indices, data, indptr.shape[0] - 1


def lbc_solve(L, wl, wh, pts, rtol: float = 1e-10, max_it: int = 20000, device: int = 0):
    """Solve (W_L L' L W_L + W_H^2) x = W_H^2 p (A = [L W_L ; W_H], skeletonize.py:164) for the
    three coordinates.
    Returns (x [n,3], iterations, relative residuals [3])."""
    indptr, indices, data, n = _csr(L)
    p = _points(pts)
    if p.shape[0] != n:
        raise ValueError("L and pts disagree on n")
    wl = np.ascontiguousarray(np.broadcast_to(np.asarray(wl, dtype=np.float64), (n,)))
    wh = np.ascontiguousarray(np.broadcast_to(np.asarray(wh, dtype=np.float64), (n,)))
    out = np.empty_like(p)
    iters = i32(0)
    resid = np.zeros(3)
    rc = _lib.load().pyqsm_lbc_solve(_p(indptr), _p(indices), _p(data), n, _p(wl), _p(wh), _p(p),
                                     float(rtol), int(max_it), _p(out), ctypes.byref(iters),
                                     _p(resid), int(device))
    if rc not in (0, -6):
        check(rc)
    return out, int(iters.value), resid, rc == 0


def spmv3(L, x, device: int = 0):
    indptr, indices, data, n = _csr(L)
    x = _points(x)
    y = np.empty_like(x)
    check(_lib.load().pyqsm_spmv3(_p(indptr), _p(indices), _p(data), n, _p(x), _p(y), int(device)))
    return y


def amg_probe(L, cw, wh, rhs=None, device: int = 0) -> dict:
    """For tests (``pyqsm_amg_probe``): the multigrid hierarchy of ``B = diag(cw) L + diag(wh)`` as
    ``lbc_solve`` builds it, and one cycle of it per right-hand side ``rhs[r]`` ([m, n, 3]).

    ``n_levels``; with fewer than two levels nothing else (``levels`` is empty, no cycle is run).
    ``levels[l]``: ``n, indptr, indices, vals, diag, dinv`` and, where a coarser level follows,
    ``agg, mptr, members`` and (unless PYQSM_AMG_AP=0) ``ap_ptr, ap_idx, ap_val``; absent ones are None.
    ``coarse``: "host" / "device" (a dense inverse, ``inverse`` [nc, nc] fp64) or "sweeps".
    ``x64`` f64 / ``x32`` f32 [m, n, 3]: the fp64 interface's result and the fp32 interface's on
    ``rhs.astype(float32)``; ``dot64`` / ``dot32`` [m, 3]: the ``rhs . x`` the cycles return."""
    indptr, indices, data, n = _csr(L)
    cw = np.ascontiguousarray(np.broadcast_to(np.asarray(cw, dtype=np.float64), (n,)))
    wh = np.ascontiguousarray(np.broadcast_to(np.asarray(wh, dtype=np.float64), (n,)))
    rhs = np.zeros((0, n, 3)) if rhs is None else np.ascontiguousarray(rhs, dtype=np.float64)
    if rhs.ndim != 3 or rhs.shape[1:] != (n, 3):
        raise ValueError(f"expected right-hand sides of shape [m,{n},3], got {rhs.shape}")
    m = rhs.shape[0]
    meta = np.zeros(108, dtype=np.int64)
    x64, x32, dots = np.zeros((m, n, 3)), np.zeros((m, n, 3), dtype=np.float32), np.zeros((m, 2, 3))
    cap = [4 * (n + 1) + 3 * len(indices), 4 * n + 2 * len(indices) + 1024 * 1024, len(indices)]
    for _ in range(2):        # the second time with the sizes the first one reported
        ibuf, dbuf, fbuf = np.zeros(cap[0], dtype=np.int32), np.zeros(cap[1]), np.zeros(cap[2], dtype=np.float32)
        check(_lib.load().pyqsm_amg_probe(_p(indptr), _p(indices), _p(data), n, _p(cw), _p(wh), _p(rhs), m,
                                          _p(meta), _p(ibuf), cap[0], _p(dbuf), cap[1], _p(fbuf), cap[2],
                                          _p(x64), _p(x32), _p(dots), int(device)))
        if meta[0] < 2 or meta[7]:
            break
        cap = [int(v) for v in meta[4:7]]
    out = {"n_levels": int(meta[0]), "levels": [], "coarse": None, "inverse": None}
    if meta[0] < 2:
        return out
    cur = {"i": 0, "d": 0, "f": 0}

    def take(which, buf, count):
        a = buf[cur[which]:cur[which] + count].copy()
        cur[which] += count
        return a

    for l in range(int(meta[0])):
        ln, nnz, nagg, nap = (int(v) for v in meta[8 + 4 * l:12 + 4 * l])
        lv = dict.fromkeys(("agg", "mptr", "members", "ap_ptr", "ap_idx", "ap_val"))
        lv["n"] = ln
        lv["indptr"], lv["indices"] = take("i", ibuf, ln + 1), take("i", ibuf, nnz)
        lv["vals"], lv["diag"], lv["dinv"] = take("d", dbuf, nnz), take("d", dbuf, ln), take("d", dbuf, ln)
        if nagg >= 0:
            lv["agg"], lv["mptr"] = take("i", ibuf, ln), take("i", ibuf, nagg + 1)
            lv["members"] = take("i", ibuf, int(lv["mptr"][-1]))
        if nap >= 0:
            lv["ap_ptr"], lv["ap_idx"], lv["ap_val"] = take("i", ibuf, ln + 1), take("i", ibuf, nap), take("f", fbuf, nap)
        out["levels"].append(lv)
    out["coarse"] = ("sweeps", "host", "device")[int(meta[1])]
    if meta[1]:
        nc, ld = int(meta[2]), int(meta[3])
        inv = take("d", dbuf, ld * ld).reshape(ld, ld)
        out["inverse"] = np.ascontiguousarray(inv.T if meta[1] == 1 else inv[:nc, :nc])   # (the host's is stored transposed)
    out.update(x64=x64, x32=x32, dot64=dots[:, 0].copy(), dot32=dots[:, 1].copy())
    return out


def clamp(pts: np.ndarray, lo, hi, device: int = 0) -> np.ndarray:
    """In-place clamp of a C-contiguous float64 [n,3] array."""
    if not (isinstance(pts, np.ndarray) and pts.dtype == np.float64 and pts.flags.c_contiguous):
        raise ValueError("clamp works in place on a C-contiguous float64 array")
    lo = np.ascontiguousarray(lo, dtype=np.float64)
    hi = np.ascontiguousarray(hi, dtype=np.float64)
    check(_lib.load().pyqsm_clamp(_p(pts), pts.shape[0], _p(lo), _p(hi), int(device)))
    return pts


# ---------------------------------------------------------------- radius queries

def ball_query(points, center, radius: float, device: int = 0) -> np.ndarray:
    """Ascending int64 indices of the points with |p - center| <= radius."""
    pts = _points(points)
    ctr = np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    out = np.empty(max(pts.shape[0], 1), dtype=np.int64)
    cnt = i64(0)
    check(_lib.load().pyqsm_ball_query(_p(pts), pts.shape[0], _p(ctr), float(radius), _p(out),
                                       ctypes.byref(cnt), int(device)))
    return out[:cnt.value].copy()


def radius_mark(src, queries, radius: float, k: int = 500, device: int = 0):
    """(mask bool [n], counts int32 [m]): source points that are among the k nearest
    neighbours within `radius` (strict) of at least one query point."""
    s = _points(src)
    q = _points(queries)
    mark = np.zeros(s.shape[0], dtype=np.uint8)
    counts = np.zeros(q.shape[0], dtype=np.int32)
    check(_lib.load().pyqsm_radius_mark(_p(s), s.shape[0], _p(q), q.shape[0], float(radius),
                                        int(k), _p(mark), _p(counts), int(device)))
    return mark.astype(bool), counts


# ---------------------------------------------------------------- down-sampling

def radius_label(src, queries, query_labels, radius: float, k: int = 500, device: int = 0):
    """int32 [n]: for every source point the smallest label among the query points that
    select it (k nearest within ``radius``, strict), -1 where none does; and the per-query
    neighbour counts."""
    s = _points(src)
    q = _points(queries)
    ql = np.ascontiguousarray(query_labels, dtype=np.int32).reshape(-1)
    if ql.shape[0] != q.shape[0]:
        raise ValueError("one label per query point")
    lab = np.empty(max(s.shape[0], 1), dtype=np.int32)
    counts = np.zeros(max(q.shape[0], 1), dtype=np.int32)
    check(_lib.load().pyqsm_radius_label(_p(s), s.shape[0], _p(q), q.shape[0], _p(ql), float(radius),
                                         int(k), _p(lab), _p(counts), int(device)))
    return lab[:s.shape[0]], counts[:q.shape[0]]


def grow_clusters(src, owner, seed_points, seed_labels, n_clusters: int, radius: float, k: int = 200,
                  cycles: int = 150, min_new: int = 5, device: int = 0):
    """The region growing of ``tree_isolation.extend_seed_clusters`` in one device-resident call
    (``pyqsm_grow_clusters``). ``owner`` int32 [n]: -1 free, else a cluster index; ``seed_points``
    [m,3] with ``seed_labels`` [m]: the frontier of cycle 0. Returns ``(owner int32 [n], cycle
    int32 [n], finished int32 [n_clusters], stats int64 [4])``: the cluster of every point, the
    cycle it was acquired in (-1: never), per cluster the cycles it queried in (-1: still growing
    when ``cycles`` ran out), and (cycles run, frontier queries served, points acquired, most
    queries in one cycle)."""
    s = _points(src)
    q = _points(seed_points)
    own = np.ascontiguousarray(owner, dtype=np.int32).reshape(-1)
    ql = np.ascontiguousarray(seed_labels, dtype=np.int32).reshape(-1)
    if own.shape[0] != s.shape[0]:
        raise ValueError("one owner per source point")
    if ql.shape[0] != q.shape[0]:
        raise ValueError("one label per seed point")
    n, nc = s.shape[0], int(n_clusters)
    owner_out = np.empty(max(n, 1), dtype=np.int32)
    cycle_out = np.empty(max(n, 1), dtype=np.int32)
    finished = np.empty(max(nc, 1), dtype=np.int32)
    stats = np.zeros(4, dtype=np.int64)
    check(_lib.load().pyqsm_grow_clusters(_p(s), n, _p(own), _p(q), _p(ql), q.shape[0], nc, float(radius),
                                          int(k), int(cycles), int(min_new), _p(owner_out), _p(cycle_out),
                                          _p(finished), _p(stats), int(device)))
    return owner_out[:n], cycle_out[:n], finished[:max(nc, 0)], stats


def radius_knn(src, queries, radius: float, k: int = 500, device: int = 0):
    """(dist f64 [m,k], idx int64 [m,k]) like ``cKDTree(src).query(queries, k,
    distance_upper_bound=radius)``: ascending by (distance, index), padded with inf / n."""
    s = _points(src)
    q = _points(queries)
    m = q.shape[0]
    idx = np.empty((m, int(k)), dtype=np.int64)
    dist = np.empty((m, int(k)), dtype=np.float64)
    check(_lib.load().pyqsm_radius_knn(_p(s), s.shape[0], _p(q), m, float(radius), int(k), _p(idx),
                                       _p(dist), int(device)))
    return dist, idx


# ---------------------------------------------------------------- cluster adjacency

class ClusterAdjacency(NamedTuple):
    """Rows of the cluster-to-cluster graph, ascending by (a, b) in the caller's label values."""
    a: np.ndarray          # int64 [r] source cluster label
    b: np.ndarray          # int64 [r] target cluster label
    dist: np.ndarray       # float64 [r] minimum distance
    n_pairs: np.ndarray    # int64 [r] point pairs within the threshold
    src_idx: np.ndarray | None = None   # int64 [r] closest point pair (return_pairs=True)
    tgt_idx: np.ndarray | None = None


ADJ_SAME_CLOUD, ADJ_WITNESS, ADJ_NO_CACHE = 1, 2, 4


def _dense_labels(labels, n: int, what: str):
    """(int32 [n] dense labels with -1 for ignored points, int64 sorted label values)."""
    lab = np.asarray(labels).reshape(-1)
    if lab.shape[0] != n:
        raise ValueError(f"one label per {what} point: {lab.shape[0]} labels for {n} points")
    if lab.size and not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"{what} labels must be integers")
    lab = lab.astype(np.int64)
    keep = lab >= 0
    values, inv = np.unique(lab[keep], return_inverse=True)
    dense = np.full(n, -1, dtype=np.int32)
    dense[keep] = inv.astype(np.int32)
    return dense, values


def _adjacency_call(s, sl, S, t, tl, T, threshold, flags, stats, device):
    """One C-ABI call, repeated with a larger capacity when the first guess was too small."""
    lib = _lib.load()
    cap = int(min(S * T, max(4096, 16 * (S + T)))) if S and T else 0
    while True:
        n_out = max(cap, 1)
        a, b = np.empty(n_out, np.int32), np.empty(n_out, np.int32)
        d2, cnt = np.empty(n_out, np.float64), np.empty(n_out, np.int64)
        wit = bool(flags & ADJ_WITNESS)
        si = np.empty(n_out, np.int64) if wit else None
        ti = np.empty(n_out, np.int64) if wit else None
        st = np.zeros(2, np.int64) if stats is not None else None
        found = i64(0)
        check(lib.pyqsm_cluster_adjacency(_p(s), _p(sl), s.shape[0], int(S), _p(t), _p(tl),
                                          0 if t is None else t.shape[0], int(T), float(threshold), int(flags),
                                          cap, _p(a), _p(b), _p(d2), _p(cnt), _p(si), _p(ti), ctypes.byref(found),
                                          _p(st), int(device)))
        r = int(found.value)
        if r <= cap:
            break
        cap = r
    if stats is not None:
        stats["distance_tests"] = stats.get("distance_tests", 0) + int(st[0])
        stats["atomic_pairs"] = stats.get("atomic_pairs", 0) + int(st[1])
    return (a[:r].astype(np.int64), b[:r].astype(np.int64), d2[:r], cnt[:r],
            si[:r] if wit else None, ti[:r] if wit else None)


def cluster_adjacency(points, labels, threshold: float, targets=None, target_labels=None,
                      return_pairs: bool = False, max_table: int = 1 << 26, device: int = 0, *,
                      cache: bool = True, stats: dict | None = None) -> ClusterAdjacency:
    """The sparse cluster-to-cluster distance graph of labelled points: for every (source cluster a,
    target cluster b) with at least one point pair within ``threshold`` (inclusive, fp64), the
    minimum distance and the number of such point pairs — what pyQSM's ``determine_adjacency``
    gets from one ``sparse_distance_matrix`` per cluster pair. Labels are any integers; negative
    ones mean "ignore this point". ``targets=None``: one labelled cloud against itself, rows with
    a < b only, every unordered point pair counted once. ``return_pairs``: also the indices of the
    closest point pair (ties: smallest source index, then smallest target index). Rows ascend by
    (a, b). One call handles ``max_table`` cluster pairs (at most 2^26); beyond that the sources
    are served in label ranges. ``cache=False`` and ``stats`` (a dict that receives
    ``distance_tests`` and ``atomic_pairs``) are for measurements and change no result."""
    s = _points(points)
    sl, s_vals = _dense_labels(labels, s.shape[0], "source")
    same = targets is None
    if same:
        if target_labels is not None:
            raise ValueError("target_labels without targets")
        t, tl, t_vals = s, sl, s_vals
    else:
        t = _points(targets)
        tl, t_vals = _dense_labels(target_labels, t.shape[0], "target")
    S, T = len(s_vals), len(t_vals)
    max_table = int(min(max(int(max_table), 1), 1 << 26))
    flags = (ADJ_WITNESS if return_pairs else 0) | (0 if cache else ADJ_NO_CACHE)
    if S * T <= max_table:
        if same:
            parts = [_adjacency_call(s, sl, S, None, None, S, threshold, flags | ADJ_SAME_CLOUD, stats, device)]
        else:
            parts = [_adjacency_call(s, sl, S, t, tl, T, threshold, flags, stats, device)]
    else:
        if T > max_table:
            raise ValueError(f"{T} target clusters exceed max_table = {max_table}")
        step = max_table // T
        order = np.argsort(sl, kind="stable")            # source points by dense label
        bounds = np.searchsorted(sl[order], np.arange(0, S + step, step))
        parts = []
        for k, lo in enumerate(range(0, S, step)):
            sel = order[bounds[k]:bounds[k + 1]]
            sel.sort()                                   # ascending indices: the witness tie-break holds
            hi = min(lo + step, S)
            a, b, d2, cnt, si, ti = _adjacency_call(np.ascontiguousarray(s[sel]), sl[sel] - np.int32(lo), hi - lo,
                                                    t, tl, T, threshold, flags, stats, device)
            a = a + lo
            if si is not None:
                si = sel[si]
            if same:                                     # the tile met the whole cloud: keep a < b
                keep = a < b
                a, b, d2, cnt = a[keep], b[keep], d2[keep], cnt[keep]
                if si is not None:
                    si, ti = si[keep], ti[keep]
            parts.append((a, b, d2, cnt, si, ti))
    cat = [np.concatenate([p[k] for p in parts]) if parts[0][k] is not None else None for k in range(6)]
    return ClusterAdjacency(s_vals[cat[0]], t_vals[cat[1]], np.sqrt(cat[2]), cat[3], cat[4], cat[5])


# ---------------------------------------------------------------- radius graph: degrees and pairs

RADIUS_MAX_RADII = 8


def radius_degrees(points, radii, device: int = 0, *, stats: dict | None = None):
    """(degree int32 [R, n], n_pairs int64 [R]) of the radius graph at every radius of ``radii`` (1 to 8,
    any order, repeats allowed; row k belongs to ``radii[k]``): ``degree[k, i]`` is the number of other
    points within ``radii[k]`` of point i (d2 <= r*r in fp64, inclusive, coincident points counted), what
    ``cKDTree.query_ball_point(points, r, return_length=True) - 1`` gives; ``n_pairs`` is the length of
    ``query_pairs(r)``. One grid at the largest radius serves all of them. ``stats`` (a dict) receives
    ``distance_tests`` and ``candidates_staged``."""
    pts = _points(points)
    rr = np.ascontiguousarray(np.atleast_1d(np.asarray(radii, dtype=np.float64)))
    if rr.ndim != 1:
        raise ValueError("radii must be a scalar or one-dimensional")
    n, R = pts.shape[0], rr.shape[0]
    degree = np.zeros((R, n), dtype=np.int32)
    n_pairs = np.zeros(max(R, 1), dtype=np.int64)
    st = np.zeros(2, dtype=np.int64) if stats is not None else None
    check(_lib.load().pyqsm_radius_degrees(_p(pts), n, _p(rr), R, _p(degree), _p(n_pairs), _p(st), int(device)))
    if stats is not None:
        stats["distance_tests"] = stats.get("distance_tests", 0) + int(st[0])
        stats["candidates_staged"] = stats.get("candidates_staged", 0) + int(st[1])
    return degree, n_pairs[:R]


def radius_pairs(points, radius: float, n_pairs: int | None = None, device: int = 0) -> np.ndarray:
    """int32 [m, 2]: every pair of points within ``radius`` once, as (i, j) with i < j, ascending by
    (i, j): ``cKDTree.query_pairs(radius, output_type='ndarray')``, sorted. ``n_pairs``: the number of
    pairs when the caller has it from :func:`radius_degrees`; without it the call is repeated once with
    the room the first one asked for."""
    pts = _points(points)
    lib = _lib.load()
    cap = 0 if n_pairs is None else int(n_pairs)
    for _ in range(2):
        out = np.empty((max(cap, 1), 2), dtype=np.int32)
        found = i64(0)
        check(lib.pyqsm_radius_pairs(_p(pts), pts.shape[0], float(radius), cap, _p(out), ctypes.byref(found),
                                     int(device)))
        if int(found.value) <= cap:
            return out[: int(found.value)]
        cap = int(found.value)
    raise RuntimeError("pyqsm_radius_pairs: the pair count changed between two calls")


def radius_components(points, radii, device: int = 0, members: bool = False):
    """The connected components of the radius graph at every radius of ``radii`` (1 to 8, any order,
    repeats allowed), ranked by (size descending, smallest member ascending):
    ``sorted(connected_components(g), key=len, reverse=True)`` over ``query_pairs(r)`` with ties in the
    order of their smallest point, no pair stored. Returns ``(component int32 [R, n], sizes)``,
    ``sizes`` a list of R int32 arrays (``sizes[k][s]`` = the points of rank ``s`` at ``radii[k]``), and
    with ``members=True`` a third item, int32 [R, n]: the point indices ascending by (component, index),
    so the points of rank ``s`` are ``members[k][off[s]:off[s + 1]]`` with ``off`` the prefix sums of
    ``sizes[k]``."""
    pts = _points(points)
    rr = np.ascontiguousarray(np.atleast_1d(np.asarray(radii, dtype=np.float64)))
    if rr.ndim != 1:
        raise ValueError("radii must be a scalar or one-dimensional")
    n, R = pts.shape[0], rr.shape[0]
    component = np.zeros((R, n), dtype=np.int32)
    sizes = np.zeros((R, n), dtype=np.int32)
    mem = np.zeros((R, n), dtype=np.int32) if members else None
    count = np.zeros(max(R, 1), dtype=np.int64)
    check(_lib.load().pyqsm_radius_components(_p(pts), n, _p(rr), R, _p(component), _p(sizes), _p(mem), _p(count),
                                              int(device)))
    out = (component, [sizes[k, : int(count[k])].copy() for k in range(R)])
    return out + (mem,) if members else out


# ---------------------------------------------------------------- projected area (alpha shape)

ALPHA_BOUNDARY = 1
ALPHA_MAX_EXTENT = 1 << 20      # lattice units per axis within a segment
ALPHA_MAX_A2 = 1 << 40


class AlphaArea(NamedTuple):
    """Per-segment results of :func:`alpha_area`."""
    twice_area: np.ndarray            # int64 [n_seg] twice the area, lattice units^2
    n_live: np.ndarray                # int64 [n_seg] points after merging coincident ones
    n_boundary: np.ndarray            # int64 [n_seg] directed boundary edges
    edges: np.ndarray | None          # int64 [sum n_boundary, 2] (return_boundary=True)
    edge_start: np.ndarray | None     # int64 [n_seg + 1] rows of `edges` per segment
    stats: dict

    def boundary(self, i: int) -> np.ndarray:
        """The boundary edges of segment i: int64 [r, 2] pairs of indices into the call's points,
        kept side on the left, ascending by (a, b)."""
        if self.edges is None:
            raise ValueError("alpha_area was called without return_boundary=True")
        return self.edges[self.edge_start[i]:self.edge_start[i + 1]]


def alpha_area(ij, a2: int, seg_start=None, return_boundary: bool = False, max_tests: int | None = None,
               device: int = 0) -> AlphaArea:
    """Twice the exact alpha-shape area of integer lattice points, per segment: the total area of
    the cells of the Delaunay subdivision with circumradius^2 <= ``a2`` (inclusive), decided by
    integer predicates only. ``ij`` int32 [n, 2]; ``seg_start`` [n_seg + 1] splits it into
    independent clouds (default: one). Coincident points are merged, the lowest index takes part.
    A segment may span at most 2^20 lattice units per axis and ``a2`` at most 2^40.
    ``max_tests`` (default: about ten seconds of one MI355X) refuses a call whose estimated
    point-against-edge tests exceed it, before the edge pass runs."""
    pts = np.asarray(ij)
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"expected lattice points of shape [n,2], got {pts.shape}")
    if pts.size and not np.issubdtype(pts.dtype, np.integer):
        raise ValueError("lattice points must be integers")
    if pts.size and (pts.min() < -(1 << 31) or pts.max() >= (1 << 31)):
        raise ValueError("lattice points must fit int32")
    pts = np.ascontiguousarray(pts, dtype=np.int32)
    n = pts.shape[0]
    seg = np.array([0, n], np.int64) if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
    if seg.ndim != 1 or seg.shape[0] < 1:
        raise ValueError("seg_start must hold n_seg + 1 offsets")
    a2 = int(a2)
    if a2 < 0 or a2 >= 1 << 64:
        raise ValueError("a2 must be a non-negative 64-bit integer")
    n_seg = seg.shape[0] - 1
    twice, live, nb = (np.zeros(max(n_seg, 1), np.int64) for _ in range(3))
    st = np.zeros(5, np.int64)
    lib = _lib.load()
    out = vp()
    check(lib.pyqsm_alpha_area(_p(pts), n, _p(seg), n_seg, a2, 0 if max_tests is None else int(max_tests),
                               ALPHA_BOUNDARY if return_boundary else 0, _p(twice), _p(live), _p(nb),
                               ctypes.byref(out), _p(st), int(device)))
    twice, live, nb = twice[:n_seg], live[:n_seg], nb[:n_seg]
    edges = start = None
    if return_boundary:
        start = np.concatenate([[0], np.cumsum(nb)]).astype(np.int64)
        edges = _adopt(lib, out, i64, 2 * int(start[-1]), np.int64).reshape(-1, 2) if out.value \
            else np.zeros((0, 2), np.int64)
    stats = dict(zip(("estimated_tests", "tests", "exact_fallbacks", "edges", "merged_duplicates"),
                     (int(v) for v in st)))
    return AlphaArea(twice, live, nb, edges, start, stats)


# ---------------------------------------------------------------- convex hull, points in boxes

HULL_MAX_EXTENT = 1 << 20                 # lattice units per axis and segment
HULL_DEFAULT_MAX_TESTS = 2_000_000_000_000    # PYQSM_HULL_DEFAULT_MAX_TESTS: ten seconds at 2.0e11 tests/s
HULL_MAX_FACET_VERTS = 1024               # PYQSM_HULL_MAX_FACET_VERTS
BOXES_MAX = 256                           # PYQSM_BOXES_MAX


class ConvexHulls(NamedTuple):
    """Results of :func:`convex_hull`."""
    tris: np.ndarray      # int32 [T, 3] indices into ijk; a smallest, outward, ascending by (a, b, c) per segment
    tri_ptr: np.ndarray   # int64 [n_seg + 1]
    dim: np.ndarray       # int32 [n_seg] affine dimension of the distinct points, -1 for an empty segment
    stats: dict


def convex_hull(ijk, seg_start=None, max_tests: int | None = None, device: int = 0) -> ConvexHulls:
    """``pyqsm_convex_hull``: the exact convex hull of integer lattice points, per segment. ``ijk``
    int32 [n, 3]; ``seg_start`` [n_seg + 1] splits it into independent clouds (default: one), each
    spanning at most 2^20 units per axis. Coincident points are merged (the lowest index takes part);
    a facet with more than three points on its plane is a fan from its vertex of lowest index.
    ``max_tests`` (default: about ten seconds of one MI355X) ends the call once the running count of
    orient tests exceeds it."""
    pts = np.asarray(ijk)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"expected lattice points of shape [n,3], got {pts.shape}")
    if pts.size and not np.issubdtype(pts.dtype, np.integer):
        raise ValueError("lattice points must be integers")
    if pts.size and (pts.min() < -(1 << 31) or pts.max() >= (1 << 31)):
        raise ValueError("lattice points must fit int32")
    pts = np.ascontiguousarray(pts, dtype=np.int32)
    n = pts.shape[0]
    seg = np.array([0, n], np.int64) if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
    if seg.ndim != 1 or seg.shape[0] < 1:
        raise ValueError("seg_start must hold n_seg + 1 offsets")
    n_seg = seg.shape[0] - 1
    dim = np.full(max(n_seg, 1), -1, np.int32)
    st = np.zeros(6, np.int64)
    lib = _lib.load()
    out_t, out_p = vp(), vp()
    check(lib.pyqsm_convex_hull(_p(pts), n, _p(seg), n_seg, 0 if max_tests is None else int(max_tests),
                                ctypes.byref(out_t), ctypes.byref(out_p), _p(dim), _p(st), int(device)))
    tri_ptr = _adopt(lib, out_p, i64, n_seg + 1, np.int64)
    T = int(tri_ptr[-1])
    if out_t.value and T > 0:
        tris = _adopt(lib, out_t, i32, 3 * T, np.int32).reshape(-1, 3)
    else:
        if out_t.value:
            lib.pyqsm_free(out_t)
        tris = np.zeros((0, 3), np.int32)
    stats = dict(zip(("candidates", "rounds", "tests", "flat_facets", "merged_duplicates", "prefilter_rounds"),
                     (int(v) for v in st)))
    return ConvexHulls(tris, tri_ptr, dim[:n_seg], stats)


def _boxes15(boxes) -> np.ndarray:
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64))
    if b.ndim != 2 or b.shape[1] != 15:
        raise ValueError(f"expected boxes of shape [B,15] (centre, R row-major, half-extent), got {b.shape}")
    return b


def points_in_boxes(points, boxes, device: int = 0):
    """``pyqsm_points_in_boxes``: ``(ptr int64 [B + 1], idx int64)``, the points inside each oriented
    box, ascending inside a box. ``points`` float64 [n, 3] or a :class:`DeviceBuffer` holding them
    (then ``pyqsm_points_in_boxes_dev``: a tile uploaded once answers any number of calls);
    ``boxes`` float64 [B, 15]: centre, R row-major, half-extent. Point p is in a box iff
    ``|((d.x R[0][i] + d.y R[1][i]) + d.z R[2][i])| <= half_i`` for every axis, d = p - centre, in
    fp64 and this order. More boxes than one call takes (256, and n * B < 2^31) are chunked here."""
    b = _boxes15(boxes)
    lib = _lib.load()
    if isinstance(points, DeviceBuffer):
        n, src, fn, device = points.nbytes // 24, points.ptr, lib.pyqsm_points_in_boxes_dev, points.device
        keep = points
    else:
        keep = _points(points)
        n, src, fn = keep.shape[0], _p(keep), lib.pyqsm_points_in_boxes
    B = b.shape[0]
    step = max(1, min(BOXES_MAX, 0x7FFFFF00 // max(n, 1)))
    ptrs, idxs, base = [np.zeros(1, np.int64)], [], 0
    for k0 in range(0, B, step):
        part = np.ascontiguousarray(b[k0:k0 + step])
        ptr = np.zeros(part.shape[0] + 1, np.int64)
        out = vp()
        check(fn(src, n, _p(part), part.shape[0], _p(ptr), ctypes.byref(out), int(device)))
        if out.value:
            idxs.append(_adopt(lib, out, i64, int(ptr[-1]), np.int64))
        ptrs.append(ptr[1:] + base)
        base += int(ptr[-1])
    idx = np.concatenate(idxs) if idxs else np.zeros(0, np.int64)
    return np.concatenate(ptrs), idx


# ---------------------------------------------------------------- colours: HSV classes, lift, histogram, masks

COLOR_MAX_RULES = 16            # PYQSM_COLOR_MAX_RULES
COLOR_MAX_BINS = 4096           # PYQSM_COLOR_MAX_BINS
COLOR_NONE = 255                # PYQSM_COLOR_NONE
COLOR_MASKS = {"sum_gt": 0, "green": 1}     # PYQSM_MASK_SUM_GT, PYQSM_MASK_GREEN


def _colors(colors, what: str = "colors") -> np.ndarray:
    c = np.ascontiguousarray(np.asarray(colors), dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError(f"expected {what} of shape [n,3], got {c.shape}")
    return c


def _color_check(code: int) -> None:
    """A NaN or a value outside [0, 1] is a ValueError, as matplotlib raises one."""
    if code == -1 and b"outside [0, 1]" in (_lib.load().pyqsm_last_error() or b""):
        raise ValueError("colour values must be in the range 0 to 1")
    check(code)


def rgb_to_hsv(colors, device: int = 0) -> np.ndarray:
    """``pyqsm_rgb_to_hsv``: ``matplotlib.colors.rgb_to_hsv`` of float64 [n,3] rows, bit for bit."""
    c = _colors(colors)
    out = np.empty_like(c)
    _color_check(_lib.load().pyqsm_rgb_to_hsv(_p(c), c.shape[0], _p(out), int(device)))
    return out


def hsv_to_rgb(hsv, device: int = 0) -> np.ndarray:
    """``pyqsm_hsv_to_rgb``: ``matplotlib.colors.hsv_to_rgb`` of float64 [n,3] rows, bit for bit."""
    c = _colors(hsv, "hsv")
    out = np.empty_like(c)
    _color_check(_lib.load().pyqsm_hsv_to_rgb(_p(c), c.shape[0], _p(out), int(device)))
    return out


def _color_rules(rules, closed):
    r = np.ascontiguousarray(np.asarray(rules, dtype=np.float64).reshape(-1, 6))
    cl = np.ascontiguousarray(np.asarray(closed, dtype=np.int32).reshape(-1))
    if r.shape[0] != cl.shape[0]:
        raise ValueError(f"{r.shape[0]} rules but {cl.shape[0]} closed masks")
    if r.shape[0] > COLOR_MAX_RULES:
        raise ValueError(f"at most {COLOR_MAX_RULES} rules per call")
    return r, cl


class HsvSegment(NamedTuple):
    """Result of :func:`hsv_segment`."""
    cls: np.ndarray          # uint8 [n]: the first rule that holds, 255 for none
    counts: np.ndarray       # int64 [K + 1]: rows per class, "none" last
    members: np.ndarray      # int64 [n] the CSR by class (ascending inside a class), or None
    rgb: np.ndarray          # float64 [n,3] the corrected colours, or None
    hsv: np.ndarray          # float64 [n,3] rgb_to_hsv of the corrected colours, or None


def hsv_segment(colors, rules, closed, min_s: float = 0.2, lift_div: float = 3.0, members: bool = True,
                corrected: bool = True, hsv: bool = True, device: int = 0) -> HsvSegment:
    """``pyqsm_hsv_segment``: saturation lift (``s + (1 - s) / lift_div`` where ``s < min_s``), round trip
    through rgb and the class of every row, the first of ``rules`` float64 [K,6] = (h_lo, h_hi, s_lo, s_hi,
    v_lo, v_hi) that holds on the hsv of the corrected colour; ``closed`` int32 [K]: bit 2c / 2c + 1 make
    the lower / upper bound of channel c inclusive."""
    c = _colors(colors)
    r, cl = _color_rules(rules, closed)
    n, K = c.shape[0], r.shape[0]
    cls = np.empty(n, np.uint8)
    counts = np.zeros(K + 1, np.int64)
    mem = np.empty(n, np.int64) if members else None
    rgb = np.empty((n, 3)) if corrected else None
    hs = np.empty((n, 3)) if hsv else None
    _color_check(_lib.load().pyqsm_hsv_segment(_p(c), n, float(min_s), float(lift_div), _p(r), _p(cl), K, _p(cls),
                                               _p(counts), _p(mem), _p(rgb), _p(hs), int(device)))
    return HsvSegment(cls, counts, mem, rgb, hs)


def hsv_segment_dev(rgb_ptr: int, n: int, rules, closed, cls_ptr: int, min_s: float = 0.2, lift_div: float = 3.0,
                    members_ptr=None, rgb_out_ptr=None, hsv_out_ptr=None, device: int = 0) -> np.ndarray:
    """:func:`hsv_segment` on ``n`` device-resident rows, every output but the counts (returned) left in
    the caller's device buffers: cls uint8 [n], members int64 [n], rgb_out / hsv_out float64 [n,3]."""
    r, cl = _color_rules(rules, closed)
    counts = np.zeros(r.shape[0] + 1, np.int64)
    _color_check(_lib.load().pyqsm_hsv_segment_dev(rgb_ptr, int(n), float(min_s), float(lift_div), _p(r), _p(cl),
                                                   r.shape[0], cls_ptr, _p(counts), members_ptr, rgb_out_ptr,
                                                   hsv_out_ptr, int(device)))
    return counts


def hsv_histogram(values, bins=(20, 1, 1), is_hsv: bool = False, cls=None, which: int = -1,
                  device: int = 0) -> np.ndarray:
    """``pyqsm_hsv_histogram``: ``np.histogramdd(hsv, bins, range=[(0, 1)] * 3)[0]`` as int64 [bh, bs, bv] of
    hsv rows, or of rgb rows converted first; with ``cls`` uint8 [n] and ``which >= 0`` only the rows of
    that class."""
    c = _colors(values, "values")
    b = np.ascontiguousarray(np.asarray(bins, dtype=np.int32).reshape(-1))
    if b.shape[0] != 3:
        raise ValueError(f"expected three bin counts, got {b.shape[0]}")
    if (b < 1).any():
        raise ValueError("every bin count must be at least 1")
    k = None
    if int(which) >= 0:
        if cls is None:
            raise ValueError("which needs the class bytes")
        k = np.ascontiguousarray(np.asarray(cls, dtype=np.uint8).reshape(-1))
        if k.shape[0] != c.shape[0]:
            raise ValueError(f"{k.shape[0]} classes for {c.shape[0]} rows")
    nb = int(b[0]) * int(b[1]) * int(b[2])
    hist = np.zeros(min(nb, COLOR_MAX_BINS), np.int64)
    _color_check(_lib.load().pyqsm_hsv_histogram(_p(c), c.shape[0], int(bool(is_hsv)), _p(b), _p(k), int(which),
                                                 _p(hist), int(device)))
    return hist.reshape(tuple(int(v) for v in b))


def color_mask(colors, kind="sum_gt", param: float = 2.7, device: int = 0) -> np.ndarray:
    """``pyqsm_color_mask``: the ascending indices of the rows with ``((0.0 + r) + g) + b > param``
    (``kind='sum_gt'``) or ``g > r and g > b and 0.5 < r / b < 2`` (``kind='green'``)."""
    c = _colors(colors)
    idx = np.empty(c.shape[0], np.int64)
    count = i64(0)
    _color_check(_lib.load().pyqsm_color_mask(_p(c), c.shape[0], COLOR_MASKS[kind], float(param), _p(idx),
                                              ctypes.byref(count), int(device)))
    return idx[:count.value].copy()


# ---------------------------------------------------------------- pairwise-distance order statistics

PDIST_MAX_RANKS = 32                          # PYQSM_PDIST_MAX_RANKS
PDIST_DEFAULT_MAX_PAIRS = 1_200_000_000_000   # PYQSM_PDIST_DEFAULT_MAX_PAIRS: ten seconds at 9.3e11 evaluations/s


class PdistSelect(NamedTuple):
    """Per-segment results of :func:`pdist_select`."""
    values: np.ndarray      # float64 [n_seg, n_ranks] the distances of the given ranks (0.0 in unused slots)
    n_pairs: np.ndarray     # int64 [n_seg] M_s = n_s (n_s - 1) / 2
    max_pair: np.ndarray    # int64 [n_seg, 2] the farthest pair (i < j, local to the segment), (-1, -1) without pairs
    stats: dict


def pdist_select(points, seg_start, ranks, max_pairs: int = 0, device: int = 0) -> PdistSelect:
    """``pyqsm_pdist_select``: elements of the sorted ``scipy.spatial.distance.pdist`` of every
    segment, bit for bit, without the distances being stored. ``points`` float64 [n, 2] or [n, 3];
    ``seg_start`` [n_seg + 1] splits them into independent clouds (None: one); ``ranks`` int64
    [n_seg, n_ranks] (or [n_ranks] for one segment), 0-based, a negative rank marks an unused slot.
    At most 32 ranks per segment. ``max_pairs`` (0: about ten seconds of one MI355X) refuses a call
    with more point pairs before anything is launched."""
    pts = np.ascontiguousarray(np.asarray(points), dtype=np.float64)
    if pts.ndim != 2:
        raise ValueError(f"expected points of shape [n,dim], got {pts.shape}")
    n, dim = pts.shape
    seg = np.array([0, n], np.int64) if seg_start is None else np.ascontiguousarray(seg_start, dtype=np.int64)
    if seg.ndim != 1 or seg.shape[0] < 1:
        raise ValueError("seg_start must hold n_seg + 1 offsets")
    n_seg = seg.shape[0] - 1
    rk = np.ascontiguousarray(ranks, dtype=np.int64)
    if rk.ndim == 1 and n_seg == 1:
        rk = rk.reshape(1, -1)
    if rk.ndim != 2 or rk.shape[0] != n_seg:
        raise ValueError(f"expected ranks of shape [{n_seg}, n_ranks], got {rk.shape}")
    n_ranks = rk.shape[1]
    values = np.zeros((n_seg, n_ranks), np.float64)
    n_pairs = np.zeros(max(n_seg, 1), np.int64)
    far = np.full((max(n_seg, 1), 2), -1, np.int64)
    st = np.zeros(3, np.int64)
    check(_lib.load().pyqsm_pdist_select(_p(pts), n, dim, _p(seg), n_seg, _p(rk), n_ranks, int(max_pairs),
                                         _p(values), _p(n_pairs), _p(far), _p(st), int(device)))
    stats = dict(zip(("pairs", "pair_evaluations", "passes"), (int(v) for v in st)))
    return PdistSelect(values, n_pairs[:n_seg], far[:n_seg], stats)


# ---------------------------------------------------------------- epiphyte split: selection, labels, k-means++

KEY_NORM = -1                   # PYQSM_KEY_NORM
SELECT_MAX_RANKS = PDIST_MAX_RANKS
COMPARISONS = {"gt": 0, "ge": 1, "lt": 2, "le": 3}
KMEANSPP_MAX_K = 64             # PYQSM_KMEANSPP_MAX_K


def _rows(values):
    """float64 [n, 1] or [n, 3] rows of a [n] or [n, 3] array."""
    v = np.ascontiguousarray(np.asarray(values), dtype=np.float64)
    if v.ndim == 1:
        v = v.reshape(-1, 1)
    if v.ndim != 2 or v.shape[1] not in (1, 3):
        raise ValueError(f"expected values of shape [n] or [n,3], got {v.shape}")
    return v


def _key(key, width: int) -> int:
    if key == "norm":
        key = KEY_NORM
    key = int(key)
    if key == KEY_NORM and width == 3 or 0 <= key < width:
        return key
    raise ValueError(f"key must be a column below {width}" + (" or 'norm'" if width == 3 else "") + f", got {key!r}")


def _ranks(ranks, n: int) -> np.ndarray:
    rk = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
    if rk.shape[0] > SELECT_MAX_RANKS:
        raise ValueError(f"at most {SELECT_MAX_RANKS} ranks per call")
    if (rk >= n).any():
        raise ValueError(f"a rank beyond the {n} values")
    return rk


def _select_check(code: int) -> None:
    """A NaN among the values is a ValueError, as np.percentile's callers expect."""
    if code == -1 and b"NaN" in (_lib.load().pyqsm_last_error() or b""):
        raise ValueError("the values hold a NaN")
    check(code)


def select_values(values, ranks, key=0, device: int = 0) -> np.ndarray:
    """``pyqsm_select_values``: ``np.sort(keys)[ranks]`` bit for bit (-0.0 comes back as 0.0), the keys
    of ``values`` [n] or [n,3] being column ``key`` or, with ``key='norm'``, the row norms
    ``sqrt(((x*x) + (y*y)) + (z*z))``. At most 32 ranks; a negative rank is an unused slot (0.0)."""
    v = _rows(values)
    rk = _ranks(ranks, v.shape[0])
    out = np.zeros(rk.shape[0])
    _select_check(_lib.load().pyqsm_select_values(_p(v), v.shape[0], v.shape[1], _key(key, v.shape[1]), _p(rk),
                                                  rk.shape[0], _p(out), int(device)))
    return out


def select_values_dev(v_ptr: int, n: int, width: int, ranks, key=0, device: int = 0) -> np.ndarray:
    """:func:`select_values` on ``n`` device-resident rows of ``width`` values."""
    rk = _ranks(ranks, int(n))
    out = np.zeros(rk.shape[0])
    _select_check(_lib.load().pyqsm_select_values_dev(v_ptr, int(n), int(width), _key(key, int(width)), _p(rk),
                                                      rk.shape[0], _p(out), int(device)))
    return out


def split_above_dev(v_ptr: int, n: int, width: int, threshold: float, key=0, cmp: str = "gt", rows_ptr=None,
                    idx_ptr=None, out_rows_ptr=None, device: int = 0) -> int:
    """``pyqsm_split_above_dev``: the device rows with ``cmp(key(row), threshold)`` (``cmp`` one of gt, ge,
    lt, le), their ascending indices into ``idx_ptr`` (int64) and rows of ``rows_ptr`` [n,3] into
    ``out_rows_ptr``; returns how many."""
    cnt = i64(0)
    check(_lib.load().pyqsm_split_above_dev(v_ptr, int(n), int(width), _key(key, int(width)), COMPARISONS[cmp],
                                            float(threshold), rows_ptr, idx_ptr, out_rows_ptr, ctypes.byref(cnt),
                                            int(device)))
    return int(cnt.value)


class ShiftComponents(NamedTuple):
    """Result of :func:`shift_components`."""
    labels: np.ndarray       # uint8 [n]: 0 low shift (wood), 1 leaf, 2 epiphyte
    thresholds: np.ndarray   # float64 [2]: P(q_mag) of the norms, P(q_z) of the high rows' z (NaN without high rows)
    counts: np.ndarray       # int64 [3] rows per label


def shift_components(shift, q_mag: float = 65, q_z: float = 60, device: int = 0) -> ShiftComponents:
    """``pyqsm_shift_components``: the two percentile splits of ``identify_epiphytes`` on the first
    contraction step's shift vectors [n,3], in one call."""
    s = _points(shift)
    labels = np.zeros(s.shape[0], np.uint8)
    thr, counts = np.full(2, np.nan), np.zeros(3, np.int64)
    _select_check(_lib.load().pyqsm_shift_components(_p(s), s.shape[0], float(q_mag), float(q_z), _p(labels), _p(thr),
                                                     _p(counts), int(device)))
    return ShiftComponents(labels, thr, counts)


def shift_components_dev(shift_ptr: int, n: int, labels_ptr: int, q_mag: float = 65, q_z: float = 60,
                         device: int = 0):
    """:func:`shift_components` on device-resident shifts, labels (uint8 [n]) left on the device: returns
    ``(thresholds, counts)``."""
    thr, counts = np.full(2, np.nan), np.zeros(3, np.int64)
    _select_check(_lib.load().pyqsm_shift_components_dev(shift_ptr, int(n), float(q_mag), float(q_z), labels_ptr,
                                                         _p(thr), _p(counts), int(device)))
    return thr, counts


class KMeansPP(NamedTuple):
    """Result of :func:`kmeans_pp`."""
    labels: np.ndarray       # int32 [n]
    centres: np.ndarray      # float64 [k, d]
    inertia: float
    n_iter: int
    n_empty: int             # centres without a member
    seeds: np.ndarray        # int64 [k] the points the seeding chose


def kmeanspp_trials(k: int) -> int:
    """Candidates per seeding step: scikit-learn's ``2 + int(log(k))``."""
    return 2 + int(np.log(k))


def _kmeans_pp_args(n, d, k, first, uniforms, max_iter, tol):
    if d not in (1, 2, 3):
        raise ValueError(f"points of 1, 2 or 3 columns, got {d}")
    if not 1 <= k <= KMEANSPP_MAX_K:
        raise ValueError(f"between 1 and {KMEANSPP_MAX_K} clusters, got {k}")
    if n < k:
        raise ValueError(f"n_samples={n} should be >= n_clusters={k}.")
    u = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(-1)
    if u.shape[0] != (k - 1) * kmeanspp_trials(k):
        raise ValueError(f"{(k - 1) * kmeanspp_trials(k)} uniforms are needed, got {u.shape[0]}")
    return u, (np.empty(n, np.int32), np.empty((k, d)), dbl(0.0), i32(0), i32(0), np.empty(k, np.int64))


def _kmeans_pp_call(fn, x, n, d, k, first, u, max_iter, tol, out, device) -> KMeansPP:
    labels, centres, inertia, n_iter, n_empty, seeds = out
    check(fn(x, n, d, k, int(first), _p(u), u.shape[0], int(max_iter), float(tol), _p(labels), _p(centres),
             ctypes.byref(inertia), ctypes.byref(n_iter), ctypes.byref(n_empty), _p(seeds), int(device)))
    return KMeansPP(labels, centres, inertia.value, int(n_iter.value), int(n_empty.value), seeds)


def kmeans_pp(points, k: int, first: int, uniforms, max_iter: int = 300, tol: float = 1e-4,
              device: int = 0) -> KMeansPP:
    """``pyqsm_kmeans_pp``: k-means++ seeding and Lloyd iterations of ``points`` [n,d], d <= 3, from the
    caller's draws: ``first``, the first centre's point, and ``(k - 1) * kmeanspp_trials(k)`` uniforms in
    [0, 1) (``math_utils.clustering.kmeanspp_draws``)."""
    x = np.ascontiguousarray(np.asarray(points), dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    if x.ndim != 2:
        raise ValueError(f"expected points of shape [n,d], got {x.shape}")
    n, d = x.shape
    u, out = _kmeans_pp_args(n, d, int(k), first, uniforms, max_iter, tol)
    return _kmeans_pp_call(_lib.load().pyqsm_kmeans_pp, _p(x), n, d, int(k), first, u, max_iter, tol, out, device)


def kmeans_pp_dev(x_ptr: int, n: int, d: int, k: int, first: int, uniforms, max_iter: int = 300, tol: float = 1e-4,
                  device: int = 0) -> KMeansPP:
    """:func:`kmeans_pp` on ``n`` device-resident points of ``d`` columns."""
    u, out = _kmeans_pp_args(int(n), int(d), int(k), first, uniforms, max_iter, tol)
    return _kmeans_pp_call(_lib.load().pyqsm_kmeans_pp_dev, x_ptr, int(n), int(d), int(k), first, u, max_iter, tol,
                           out, device)


# ---------------------------------------------------------------- mesh checks

MESH_PAIRS = 1
MESH_TILE_ROWS = 256            # triangles per tile of the self-intersection sweep
MESH_MAX_EXTENT = 1 << 20       # lattice units per axis
MESH_DEFAULT_MAX_TESTS = 16_000_000_000_000   # PYQSM_MESH_DEFAULT_MAX_TESTS: ten seconds at 1.6e12 box tests/s
EDGE_BOUNDARY, EDGE_OVER_TWO, EDGE_SAME_DIRECTION = 1, 2, 4


class MeshTopology(NamedTuple):
    """Results of :func:`mesh_topology`."""
    edges: np.ndarray               # int32 [E, 2] undirected edges (a < b), ascending by (a, b)
    edge_count: np.ndarray          # int32 [E] triangles at each edge
    edge_flags: np.ndarray          # uint8 [E] EDGE_BOUNDARY | EDGE_OVER_TWO | EDGE_SAME_DIRECTION
    tri_cluster: np.ndarray         # int32 [T] cluster of each triangle, numbered by smallest member
    cluster_n: np.ndarray           # int64 [C] triangles per cluster
    cluster_area: np.ndarray | None  # float64 [C] (with vertices)
    vertex_flags: np.ndarray        # uint8 [V] 1 = non-manifold vertex
    summary: dict


class MeshIntersections(NamedTuple):
    """Results of :func:`mesh_self_intersections`."""
    n_pairs: int
    pairs: np.ndarray | None        # int32 [n_pairs, 2], i < j, ascending (return_pairs=True)
    tri_hit: np.ndarray             # uint8 [T] 1 = the triangle is in some pair
    stats: dict


def _tris_i32(tris) -> np.ndarray:
    t = np.asarray(tris)
    if t.size and not np.issubdtype(t.dtype, np.integer):
        raise ValueError("triangle indices must be integers")
    if t.size and (t.min() < -(1 << 31) or t.max() >= (1 << 31)):
        raise ValueError("triangle indices must fit int32")
    return np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)


def mesh_topology(tris, n_verts: int, verts=None, device: int = 0) -> MeshTopology:
    """The edge table, the triangle clusters (with their areas when ``verts`` f64 [V,3] is given),
    vertex manifoldness and orientability of an indexed triangle mesh, decided by vertex index
    alone (nothing is welded). Every output has a fixed order and the same bits on every run.
    An index outside ``[0, n_verts)`` or a triangle that repeats an index is refused."""
    t = _tris_i32(tris)
    nt, nv = t.shape[0], int(n_verts)
    v = None
    if verts is not None:
        v = np.ascontiguousarray(np.asarray(verts), dtype=np.float64)
        if v.shape != (nv, 3):
            raise ValueError(f"expected vertices of shape [{nv},3], got {v.shape}")
    cl = np.zeros(max(nt, 1), np.int32)
    vf = np.zeros(max(nv, 1), np.uint8)
    summ = np.zeros(8, np.int64)
    lib = _lib.load()
    e_ptr, ec_ptr, ef_ptr, cn_ptr, ca_ptr = vp(), vp(), vp(), vp(), vp()
    check(lib.pyqsm_mesh_topology(_p(t), nt, nv, _p(v), ctypes.byref(e_ptr), ctypes.byref(ec_ptr),
                                  ctypes.byref(ef_ptr), _p(cl), ctypes.byref(cn_ptr), ctypes.byref(ca_ptr),
                                  _p(vf), _p(summ), int(device)))
    ne, nc = int(summ[0]), int(summ[5])

    def take(ptr, ctype, count, dtype):
        return _adopt(lib, ptr, ctype, count, dtype) if ptr.value and count else np.zeros(0, dtype)

    edges = take(e_ptr, i32, 2 * ne, np.int32).reshape(-1, 2)
    area = None
    if v is not None:
        area = take(ca_ptr, dbl, nc, np.float64)
    summary = dict(zip(("edges", "boundary_edges", "over_two_edges", "same_direction_edges",
                        "non_manifold_vertices", "clusters", "orientable", "isolated_vertices"),
                       (int(x) for x in summ)))
    return MeshTopology(edges, take(ec_ptr, i32, ne, np.int32), take(ef_ptr, ctypes.c_uint8, ne, np.uint8),
                        cl[:nt], take(cn_ptr, i64, nc, np.int64), area, vf[:nv], summary)


def mesh_self_intersections(ijk, tris, return_pairs: bool = True, max_tests: int | None = None,
                            device: int = 0) -> MeshIntersections:
    """The pairs ``i < j`` of triangles of a lattice mesh (``ijk`` int32 [V,3], at most 2^20 units of
    extent per axis) that share no vertex index, are not degenerate and whose closed triangles have
    a common point, decided with integer predicates only: a brute-force sweep of all pairs.
    ``max_tests`` refuses a call with more than that many pairs, T (T - 1) / 2, before anything is
    launched; None: ``MESH_DEFAULT_MAX_TESTS``, ten seconds at the 1.6e12 box tests per second measured
    on one MI355X (about 5.6 M triangles)."""
    p = np.asarray(ijk)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"expected lattice vertices of shape [V,3], got {p.shape}")
    if p.size and not np.issubdtype(p.dtype, np.integer):
        raise ValueError("lattice vertices must be integers")
    if p.size and (p.min() < -(1 << 31) or p.max() >= (1 << 31)):
        raise ValueError("lattice vertices must fit int32")
    p = np.ascontiguousarray(p, dtype=np.int32)
    t = _tris_i32(tris)
    nt = t.shape[0]
    hit = np.zeros(max(nt, 1), np.uint8)
    st = np.zeros(6, np.int64)
    n_pairs = i64(0)
    out = vp()
    lib = _lib.load()
    code = lib.pyqsm_mesh_self_intersections(_p(p), p.shape[0], _p(t), nt, MESH_PAIRS if return_pairs else 0,
                                             0 if max_tests is None else int(max_tests), ctypes.byref(n_pairs),
                                             ctypes.byref(out), _p(hit), _p(st), int(device))
    stats = dict(zip(("pairs_considered", "box_survivors", "shared_index_skipped", "degenerate_triangles",
                      "exact_tests", "pairs_reported"), (int(x) for x in st)))
    if code != 0:
        try:
            check(code)
        except _lib.PyQSMHipError as err:
            err.stats = stats       # what ran before the refusal (nothing, for a refused size)
            raise
    pairs = None
    if return_pairs:
        pairs = _adopt(lib, out, i32, 2 * n_pairs.value, np.int32).reshape(-1, 2) if out.value \
            else np.zeros((0, 2), np.int32)
    return MeshIntersections(int(n_pairs.value), pairs, hit[:nt], stats)


# ---------------------------------------------------------------- mesh hole filling

FILL_MAX_LOOP = 128             # PYQSM_FILL_MAX_LOOP: the longest loop that is patched
FILL_WAVE_MAX = 32              # PYQSM_FILL_WAVE_MAX: up to here one wave patches a loop, beyond it one block
LOOP_REPEATED_VERTEX, LOOP_TOO_LONG = 1, 2
_FILL_STATS = ("boundary_half_edges", "loops", "loops_filled", "loops_repeated_vertex", "loops_too_long",
               "open_chain_half_edges", "zero_area_rows", "existing_diagonals")


class BoundaryLoops(NamedTuple):
    """Results of :func:`mesh_boundary_loops`."""
    ptr: np.ndarray                 # int32 [n_loops + 1]
    verts: np.ndarray               # int32 [ptr[-1]] the loops' vertices in the fill direction
    stats: dict

    def loop(self, i: int) -> np.ndarray:
        return self.verts[self.ptr[i]:self.ptr[i + 1]]


class HoleFill(NamedTuple):
    """Results of :func:`mesh_fill_holes`."""
    ptr: np.ndarray                 # int32 [n_loops + 1]
    verts: np.ndarray               # int32 [ptr[-1]]
    flags: np.ndarray               # uint8 [n_loops] LOOP_REPEATED_VERTEX | LOOP_TOO_LONG; 0: filled
    area: np.ndarray                # float64 [n_loops] the patch's area; 0 where not filled
    new_tris: np.ndarray            # int32 [n_new, 3]
    new_loop: np.ndarray            # int32 [n_new] the loop each new row closes
    stats: dict

    def loop(self, i: int) -> np.ndarray:
        return self.verts[self.ptr[i]:self.ptr[i + 1]]


def _fill_take(lib, ptr, ctype, count, dtype):
    return _adopt(lib, ptr, ctype, count, dtype) if ptr.value and count else np.zeros(0, dtype)


def mesh_boundary_loops(tris, n_verts: int, device: int = 0) -> BoundaryLoops:
    """The boundary loops of an indexed triangle mesh: the cycles of "next boundary
    half-edge about the head vertex", each listed from its smallest vertex in the direction a patch
    would run, the loops ascending by that vertex. Half-edges whose walk meets an edge of more than two
    triangles or a same-direction pair lie on open chains and are only counted. Decided by vertex index
    alone; the same bytes on every run."""
    t = _tris_i32(tris)
    st = np.zeros(8, np.int64)
    n_loops, p_ptr, v_ptr = i64(0), vp(), vp()
    lib = _lib.load()
    check(lib.pyqsm_mesh_boundary_loops(_p(t), t.shape[0], int(n_verts), ctypes.byref(n_loops), ctypes.byref(p_ptr),
                                        ctypes.byref(v_ptr), _p(st), int(device)))
    nl = int(n_loops.value)
    ptr = _fill_take(lib, p_ptr, i32, nl + 1, np.int32) if nl else np.zeros(1, np.int32)
    verts = _fill_take(lib, v_ptr, i32, int(ptr[-1]), np.int32)
    return BoundaryLoops(ptr, verts, dict(zip(_FILL_STATS, (int(x) for x in st))))


def mesh_fill_holes(tris, verts, max_edges: int | None = None, device: int = 0) -> HoleFill:
    """The boundary loops of :func:`mesh_boundary_loops` and, for every loop of at most ``max_edges``
    edges (None: ``FILL_MAX_LOOP``; more is refused) that repeats no vertex, its minimum-area
    triangulation in fp64: ``L - 2`` rows over the loop's own vertices, in pre-order of the split tree,
    ties to the lowest apex. The rows traverse each boundary edge against the triangle that is there;
    appended to ``tris`` they close the hole. Nothing is welded or refined, and whether a patch
    intersects the mesh is for ``mesh_self_intersections`` to say."""
    t = _tris_i32(tris)
    v = np.ascontiguousarray(np.asarray(verts), dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"expected vertices of shape [V,3], got {v.shape}")
    st = np.zeros(8, np.int64)
    n_loops, n_new = i64(0), i64(0)
    p_ptr, v_ptr, f_ptr, a_ptr, t_ptr, l_ptr = vp(), vp(), vp(), vp(), vp(), vp()
    lib = _lib.load()
    check(lib.pyqsm_mesh_fill_holes(_p(t), t.shape[0], v.shape[0], _p(v), 0 if max_edges is None else int(max_edges),
                                    ctypes.byref(n_loops), ctypes.byref(p_ptr), ctypes.byref(v_ptr),
                                    ctypes.byref(f_ptr), ctypes.byref(a_ptr), ctypes.byref(n_new),
                                    ctypes.byref(t_ptr), ctypes.byref(l_ptr), _p(st), int(device)))
    nl, nn = int(n_loops.value), int(n_new.value)
    ptr = _fill_take(lib, p_ptr, i32, nl + 1, np.int32) if nl else np.zeros(1, np.int32)
    return HoleFill(ptr, _fill_take(lib, v_ptr, i32, int(ptr[-1]), np.int32),
                    _fill_take(lib, f_ptr, ctypes.c_uint8, nl, np.uint8), _fill_take(lib, a_ptr, dbl, nl, np.float64),
                    _fill_take(lib, t_ptr, i32, 3 * nn, np.int32).reshape(-1, 3),
                    _fill_take(lib, l_ptr, i32, nn, np.int32), dict(zip(_FILL_STATS, (int(x) for x in st))))


# ---------------------------------------------------------------- surface reconstruction (ball pivoting)

RECON_MAX_RHO2 = 1 << 22        # PYQSM_RECON_MAX_RHO2: rho <= 2^11 lattice units
RECON_CHUNK = 1024              # PYQSM_RECON_CHUNK: stencil points staged in LDS at a time
RECON_SLICE = 16                # PYQSM_RECON_SLICE: points of a cell one block serves
RECON_DEFAULT_MAX_TESTS = 1_000_000_000_000   # PYQSM_RECON_DEFAULT_MAX_TESTS: ten seconds at 1.1e11 pair tests/s
RECON_NORMAL_SCALE = 1 << 14    # normals are snapped to rint(n * 2^14), int16


class BallPivotRefused(_lib.PyQSMHipError, ValueError):
    """``pyqsm_ball_pivot`` refused its input (``PYQSM_EINVAL``, ``PYQSM_ERANGE``: a radius or a cloud
    outside the bounds, an estimate above ``max_tests``, too many triangles). A ``ValueError`` like the
    refusals :func:`ball_pivot` raises before it calls the library; ``.stats`` holds the call's counters."""


class BallPivot(NamedTuple):
    """Results of :func:`ball_pivot`."""
    triangles: np.ndarray           # int32 [T, 3], smallest index first, ascending by (a, b, c)
    levels: np.ndarray              # int32 [T] index into the ascending radii
    n_unresolved_ties: int          # triangles kept although a point off their plane lies on their ball
    stats: dict


def snap_normals(normals) -> np.ndarray:
    """int16 [n,3]: ``rint(n * 2^14)`` of unit (or shorter) normals, as :func:`ball_pivot` takes them."""
    v = np.asarray(normals, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"expected normals of shape [n,3], got {v.shape}")
    if not np.isfinite(v).all():
        raise ValueError("normals must be finite")
    if v.size and np.abs(v).max() > 1.0 + 1e-9:
        raise ValueError("normals must have unit length or less")
    return np.rint(v * RECON_NORMAL_SCALE).astype(np.int16)


def ball_pivot(ijk, normals_i16, rho2_list, max_tests: int | None = None, device: int = 0) -> BallPivot:
    """The triangles of lattice points a ball of radius rho rests on from the normals' side, decided by
    integer predicates only: ``ijk`` int32 [n,3], ``normals_i16`` int16 [n,3]
    (:func:`snap_normals`), ``rho2_list`` the squared radii in lattice units^2, processed ascending,
    each at most ``RECON_MAX_RHO2``. ``max_tests`` (default ``RECON_DEFAULT_MAX_TESTS``) refuses a call in
    which the estimated pair tests of a level exceed it, before the triangle pass of any level runs
    (the binning that the estimate needs has run). Refusals are ``ValueError``s: raised here, or as
    :class:`BallPivotRefused` when the library refuses. ``stats["exact_fallbacks"]`` may differ between
    runs (it depends on the order of the points within a grid cell); nothing else does."""
    p = np.asarray(ijk)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"expected lattice points of shape [n,3], got {p.shape}")
    if p.size and not np.issubdtype(p.dtype, np.integer):
        raise ValueError("lattice points must be integers")
    if p.size and (p.min() < -(1 << 31) or p.max() >= (1 << 31)):
        raise ValueError("lattice points must fit int32")
    # per axis, as the library measures it: local coordinates are ijk - min of their own axis
    if p.size and int((p.max(axis=0).astype(np.int64) - p.min(axis=0).astype(np.int64)).max()) >= (1 << 31):
        raise ValueError("the cloud spans more than 2^31 lattice units")
    p = np.ascontiguousarray(p, dtype=np.int32)
    n = p.shape[0]
    nr = np.asarray(normals_i16)
    if nr.shape != (n, 3):
        raise ValueError(f"expected normals of shape [{n},3], got {nr.shape}")
    if nr.size and not np.issubdtype(nr.dtype, np.integer):
        raise ValueError("normals must be integers: snap_normals")
    if nr.size and (nr.min() < -(1 << 15) or nr.max() >= (1 << 15)):
        raise ValueError("normals must fit int16")
    nr = np.ascontiguousarray(nr, dtype=np.int16)
    r2 = sorted(int(r) for r in np.asarray(rho2_list).reshape(-1).tolist())
    if not r2:
        raise ValueError("at least one radius is needed")
    for r in r2:
        if r < 1:
            raise ValueError("rho^2 must be a positive integer (lattice units^2)")
        if r > RECON_MAX_RHO2:
            shift = 1
            while (r >> (2 * shift)) > RECON_MAX_RHO2:
                shift += 1
            raise ValueError(f"rho^2 = {r} exceeds 2^22 lattice units^2 (rho <= 2048): "
                             f"a quantum 2^{shift} times as large would fit")
    radii = np.asarray(r2, dtype=np.uint64)
    st = np.zeros(8, np.int64)
    n_tris = i64(0)
    out = vp()
    lib = _lib.load()
    code = lib.pyqsm_ball_pivot(_p(p), _p(nr), n, _p(radii), len(r2), 0 if max_tests is None else int(max_tests),
                                ctypes.byref(n_tris), ctypes.byref(out), _p(st), int(device))
    stats = dict(zip(("estimated_tests", "tests", "exact_fallbacks", "candidates", "unresolved_ties",
                      "max_stencil", "max_cell_points", "blocks"), (int(x) for x in st)))
    if code in (-1, -4):            # PYQSM_EINVAL, PYQSM_ERANGE: a refusal, in ValueError style
        msg = lib.pyqsm_last_error()
        err = BallPivotRefused(code, msg.decode("utf-8", "replace") if msg else "")
        err.stats = stats           # what ran before the refusal
        raise err
    check(code)
    rows = _adopt(lib, out, i32, 4 * n_tris.value, np.int32).reshape(-1, 4) if out.value \
        else np.zeros((0, 4), np.int32)
    return BallPivot(np.ascontiguousarray(rows[:, :3]), np.ascontiguousarray(rows[:, 3]),
                     stats["unresolved_ties"], stats)


# ---------------------------------------------------------------- 3-D alpha shape

ALPHA3_CHUNK = 1024             # PYQSM_ALPHA3_CHUNK: neighbours staged in LDS at a time
ALPHA3_SLICE = 16               # PYQSM_ALPHA3_SLICE: points of a cell one work item serves
ALPHA3_DEFAULT_MAX_TESTS = 4_000_000_000_000   # PYQSM_ALPHA3_DEFAULT_MAX_TESTS: ten seconds at 4.1e11 pair tests/s
ALPHA3_REGULAR, ALPHA3_SINGULAR = 1, 2         # the kinds of a row
_ALPHA3_STATS = ("estimated_tests", "tests", "exact_fallbacks", "candidates", "unresolved_ties", "max_stencil",
                 "max_cell_points", "work_items")


class AlphaShapeRefused(_lib.PyQSMHipError, ValueError):
    """``pyqsm_alpha_shape3`` refused its input (``PYQSM_EINVAL``, ``PYQSM_ERANGE``: a radius or a cloud outside
    the bounds, an estimate above ``max_tests``, too many rows). A ``ValueError`` like the refusals
    :func:`alpha_shape3` raises before it calls the library; ``.stats`` holds the call's counters."""


class AlphaShape3(NamedTuple):
    """Results of :func:`alpha_shape3`."""
    rows: np.ndarray                # int32 [R, 4]: (a, b, c, kind), a the smallest index, ascending by (a, b, c)
    vol6: list                      # per segment: six times the enclosed volume in lattice units^3, Python int
    stats: dict


def alpha_shape3(ijk, rho2: int, seg_start=None, faces: str = "regular", max_tests: int | None = None,
                 device: int = 0) -> AlphaShape3:
    """The 3-D alpha shape of lattice points at ``alpha^2 = rho2`` lattice units^2, decided by integer
    predicates only: the triples with exactly one empty ball of radius alpha through them
    (``kind`` 1, oriented out of the solid) and, with ``faces="all"``, those with two (``kind`` 2, ``b < c``).
    ``ijk`` int32 [n,3]; ``seg_start`` [n_seg + 1] splits it into independent clouds on one lattice.
    ``vol6[s]`` is the exact sum of ``det(a - o, b - o, c - o)`` over the regular rows of segment ``s``; it is
    six times a volume only when ``stats["unresolved_ties"]`` is 0. ``max_tests``: the work cap of
    :func:`ball_pivot`. Refusals are ``ValueError``s: raised here, or as :class:`AlphaShapeRefused` when the
    library refuses. ``stats["exact_fallbacks"]`` may differ between runs; nothing else does."""
    p = np.asarray(ijk)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"expected lattice points of shape [n,3], got {p.shape}")
    if p.size and not np.issubdtype(p.dtype, np.integer):
        raise ValueError("lattice points must be integers")
    if p.size and (p.min() < -(1 << 31) or p.max() >= (1 << 31)):
        raise ValueError("lattice points must fit int32")
    if p.size and int((p.max(axis=0).astype(np.int64) - p.min(axis=0).astype(np.int64)).max()) >= (1 << 31):
        raise ValueError("the cloud spans more than 2^31 lattice units")
    p = np.ascontiguousarray(p, dtype=np.int32)
    n = p.shape[0]
    if faces not in ("regular", "all"):
        raise ValueError(f"faces must be 'regular' or 'all', got {faces!r}")
    r = int(rho2)
    if r < 1:
        raise ValueError("rho^2 must be a positive integer (lattice units^2)")
    if r > RECON_MAX_RHO2:
        shift = 1
        while (r >> (2 * shift)) > RECON_MAX_RHO2:
            shift += 1
        raise ValueError(f"rho^2 = {r} exceeds 2^22 lattice units^2 (rho <= 2048): "
                         f"a quantum 2^{shift} times as large would fit")
    if seg_start is None:
        seg, n_seg = None, 1
    else:
        seg = np.ascontiguousarray(seg_start, dtype=np.int64)
        if seg.ndim != 1 or seg.shape[0] < 1 or seg[0] != 0 or seg[-1] != n or (np.diff(seg) < 0).any():
            raise ValueError("seg_start must hold n_seg + 1 ascending offsets from 0 to n")
        n_seg = seg.shape[0] - 1
    st = np.zeros(8, np.int64)
    halves = np.zeros((max(n_seg, 1), 2), np.uint64)
    n_rows = i64(0)
    out = vp()
    lib = _lib.load()
    code = lib.pyqsm_alpha_shape3(_p(p), n, None if seg is None else _p(seg), n_seg, r, int(faces == "all"),
                                  0 if max_tests is None else int(max_tests), ctypes.byref(n_rows),
                                  ctypes.byref(out), _p(halves), _p(st), int(device))
    stats = dict(zip(_ALPHA3_STATS, (int(x) for x in st)))
    if code in (-1, -4):            # PYQSM_EINVAL, PYQSM_ERANGE: a refusal, in ValueError style
        msg = lib.pyqsm_last_error()
        err = AlphaShapeRefused(code, msg.decode("utf-8", "replace") if msg else "")
        err.stats = stats           # what ran before the refusal
        raise err
    check(code)
    rows = _adopt(lib, out, i32, 4 * n_rows.value, np.int32).reshape(-1, 4) if out.value \
        else np.zeros((0, 4), np.int32)
    vol6 = []
    for lo, hi in halves[:n_seg].tolist():
        v = (int(hi) << 64) | int(lo)
        vol6.append(v - (1 << 128) if v >> 127 else v)
    return AlphaShape3(rows, vol6, stats)


def fps(points, num_samples: int, start_index: int = 0, device: int = 0) -> np.ndarray:
    """Farthest-point sampling: int32 indices in selection order."""
    pts = _points(points)
    out = np.empty(int(num_samples), dtype=np.int32)
    check(_lib.load().pyqsm_fps(_p(pts), pts.shape[0], int(num_samples), int(start_index),
                                _p(out), int(device)))
    return out


# ---------------------------------------------------------------- Laplacian

def _adopt(lib, ptr, ctype, count: int, dtype):
    """NumPy array over a buffer the library malloc'ed; the buffer is released with
    ``pyqsm_free`` once the array and every view of it are gone."""
    buf = (ctype * count).from_address(ptr.value)
    weakref.finalize(buf, lib.pyqsm_free, ctypes.c_void_p(ptr.value))
    return np.frombuffer(buf, dtype=dtype, count=count)


def host_empty(shape, dtype=np.float64) -> np.ndarray:
    """``np.empty`` in the library's pool of page-locked host buffers (``pyqsm_host_alloc``): what
    the device writes into it arrives at link speed and without blocking the calling thread. The
    buffer goes back to the pool when the array and every view of it are gone."""
    shape = tuple(int(q) for q in np.atleast_1d(shape))
    dt = np.dtype(dtype)
    count = int(np.prod(shape)) if len(shape) else 1
    lib = _lib.load()
    ptr = lib.pyqsm_host_alloc(max(count * dt.itemsize, 1))
    if not ptr:
        raise MemoryError("pyqsm_host_alloc failed")
    buf = (ctypes.c_uint8 * max(count * dt.itemsize, 1)).from_address(ptr)
    weakref.finalize(buf, lib.pyqsm_free, ctypes.c_void_p(ptr))
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


def pc_laplacian(points, k: int = 30, moll: float = 1e-5, device: int = 0, seg_start=None):
    """(indptr, indices, data) CSR triple and lumped mass [n]. ``seg_start`` (int64 [S+1], from 0
    to n): the points are S clouds stacked into one array and the mollification length is taken
    per cloud (``pyqsm_pc_laplacian_seg``)."""
    pts = _points(points)
    n = pts.shape[0]
    lib = _lib.load()
    nnz = i64(0)
    ip, ix, dv = vp(), vp(), vp()
    mass = np.empty(n, dtype=np.float64)
    if seg_start is not None and len(seg_start) > 2:
        ss = np.ascontiguousarray(seg_start, dtype=np.int64)
        check(lib.pyqsm_pc_laplacian_seg(_p(pts), n, _p(ss), len(ss) - 1, int(k), float(moll),
                                         ctypes.byref(nnz), ctypes.byref(ip), ctypes.byref(ix),
                                         ctypes.byref(dv), _p(mass), int(device)))
    else:
        check(lib.pyqsm_pc_laplacian(_p(pts), n, int(k), float(moll), ctypes.byref(nnz),
                                     ctypes.byref(ip), ctypes.byref(ix), ctypes.byref(dv), _p(mass),
                                     int(device)))
    # the library's malloc'ed outputs become the NumPy arrays themselves (91 MB per million points
    # that are not copied again); pyqsm_free runs when the last view of a buffer is gone
    indptr = _adopt(lib, ip, ctypes.c_int32, n + 1, np.int32)
    indices = _adopt(lib, ix, ctypes.c_int32, max(nnz.value, 1), np.int32)[:nnz.value]
    data = _adopt(lib, dv, ctypes.c_double, max(nnz.value, 1), np.float64)[:nnz.value]
    return (indptr, indices, data), mass


def extreme_points(points, dirs, device: int = 0) -> np.ndarray:
    """Index of the point with the largest ``x . d`` for every row ``d`` of ``dirs`` [D,3]."""
    pts = _points(points)
    d = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).reshape(-1, 3))
    idx = np.empty(len(d), dtype=np.int64)
    check(_lib.load().pyqsm_extreme_points(_p(pts), pts.shape[0], _p(d), len(d), _p(idx), int(device)))
    return idx


def outside_halfspaces(points, equations, margin: float, device: int = 0) -> np.ndarray:
    """Ascending indices of the points that are NOT strictly inside the polytope
    ``a . x + o <= 0`` (rows ``(a, o)`` of ``equations`` [F,4], F <= 256)."""
    pts = _points(points)
    eq = np.ascontiguousarray(np.asarray(equations, dtype=np.float64).reshape(-1, 4))
    idx = np.empty(pts.shape[0], dtype=np.int64)
    count = i64(0)
    check(_lib.load().pyqsm_outside_halfspaces(_p(pts), pts.shape[0], _p(eq), len(eq), float(margin),
                                               _p(idx), ctypes.byref(count), int(device)))
    return idx[:count.value].copy()


# ---------------------------------------------------------------- the whole contraction loop

def extract_skeleton(points, lo, hi, k: int, moll: float, max_iter: int, termination_ratio: float,
                     contraction_factor: float, attraction_factor: float, max_contraction: float,
                     max_attraction: float, rtol: float, solver_max_it: int, seg_start=None,
                     keep_steps: bool = True, device: int = 0):
    """``pyqsm_extract_skeleton``: the loop of skeletonize.py:240-373 device-resident, for one
    cloud or several stacked ones (``seg_start`` int64 [S+1]; ``lo`` / ``hi`` float64 [S,3]).
    Returns ``(points [n,3], total_shift [n,3], steps [T,n,3] or None, n_steps int32 [S],
    solve_log list of {"iters", "resid", "ok"})``."""
    pts = _points(points)
    n = pts.shape[0]
    ss = (np.array([0, n], dtype=np.int64) if seg_start is None
          else np.ascontiguousarray(seg_start, dtype=np.int64))
    S = len(ss) - 1
    lo = np.ascontiguousarray(np.asarray(lo, dtype=np.float64).reshape(S, 3))
    hi = np.ascontiguousarray(np.asarray(hi, dtype=np.float64).reshape(S, 3))
    T = max(int(max_iter), 1)
    # page-locked results: the per-step shifts leave the device while the next step runs
    out = host_empty(pts.shape)
    total = host_empty(pts.shape)
    steps = host_empty((T, n, 3)) if keep_steps else None   # rows < n_solves are written by the library
    n_steps = np.zeros(S, dtype=np.int32)
    iters = np.zeros(T, dtype=np.int32)
    resid = np.zeros(T)
    ok = np.zeros(T, dtype=np.uint8)
    n_solves = i32(0)
    check(_lib.load().pyqsm_extract_skeleton(
        _p(pts), n, _p(ss), S, int(k), float(moll), int(max_iter), float(termination_ratio),
        float(contraction_factor), float(attraction_factor), float(max_contraction),
        float(max_attraction), _p(lo), _p(hi), float(rtol), int(solver_max_it), _p(out), _p(total),
        _p(steps), _p(n_steps), _p(iters), _p(resid), _p(ok), ctypes.byref(n_solves), int(device)))
    log = [{"iters": int(iters[t]), "resid": [float(resid[t])] * 3, "ok": bool(ok[t])}
           for t in range(n_solves.value)]
    return out, total, steps, n_steps, log


# ---------------------------------------------------------------- cloud cleaning

def _voxel_size(voxel_size) -> float:
    v = float(voxel_size)
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size!r}")
    return v


def _stat_args(nb_neighbors, std_ratio):
    nb, r = int(nb_neighbors), float(std_ratio)
    if nb < 1:
        raise ValueError(f"nb_neighbors must be at least 1, got {nb_neighbors!r}")
    if not r > 0:
        raise ValueError(f"std_ratio must be positive, got {std_ratio!r}")
    if nb > 2**31 - 1:
        raise ValueError("nb_neighbors must fit in int32")
    return nb, r


def voxel_down_sample(points, voxel_size: float, colors=None, return_trace: bool = False,
                      device: int = 0):
    """``pyqsm_voxel_down_sample``: (means [m,3], colour means [m,3] or None) and, with
    ``return_trace``, also (inverse int64 [n], offsets int64 [m+1], members int64 [n]).
    Rows are ordered by the smallest input index of each voxel."""
    pts = _points(points)
    v = _voxel_size(voxel_size)
    n = pts.shape[0]
    col = None
    if colors is not None:
        col = np.ascontiguousarray(np.asarray(colors), dtype=np.float64)
        if col.shape != pts.shape:
            raise ValueError(f"colors must have the points' shape {pts.shape}, got {col.shape}")
    lib = _lib.load()
    m, px, pc = i64(0), vp(), vp()
    inverse = np.empty(n, dtype=np.int64) if return_trace else None
    offsets = np.empty(n + 1, dtype=np.int64) if return_trace else None
    members = np.empty(n, dtype=np.int64) if return_trace else None
    check(lib.pyqsm_voxel_down_sample(_p(pts), n, _p(col), v, ctypes.byref(m), ctypes.byref(px),
                                      ctypes.byref(pc) if col is not None else None, _p(inverse),
                                      _p(offsets), _p(members), int(device)))
    M = m.value
    xyz = _adopt(lib, px, ctypes.c_double, max(3 * M, 1), np.float64)[:3 * M].reshape(M, 3) \
        if px.value else np.zeros((0, 3))
    rgb = None
    if col is not None:
        rgb = _adopt(lib, pc, ctypes.c_double, max(3 * M, 1), np.float64)[:3 * M].reshape(M, 3) \
            if pc.value else np.zeros((0, 3))
    if return_trace:
        return xyz, rgb, (inverse, offsets[:M + 1].copy(), members)
    return xyz, rgb


def stat_outlier(points, nb_neighbors: int, std_ratio: float, return_stats: bool = False,
                 device: int = 0):
    """``pyqsm_stat_outlier``: kept indices int64 (ascending); with ``return_stats`` also
    ``avg`` float64 [n] and ``(mean, std, thr)``."""
    pts = _points(points)
    nb, r = _stat_args(nb_neighbors, std_ratio)
    n = pts.shape[0]
    keep = np.empty(n, dtype=np.int64)
    cnt = i64(0)
    avg = np.empty(n, dtype=np.float64) if return_stats else None
    stats = np.full(3, np.nan) if return_stats else None
    check(_lib.load().pyqsm_stat_outlier(_p(pts), n, nb, r, _p(keep), ctypes.byref(cnt), _p(avg),
                                         _p(stats), int(device)))
    keep = keep[:cnt.value].copy()
    if return_stats:
        return keep, avg, tuple(float(s) for s in stats)
    return keep


def clean_cloud(points, voxel_size: float, neighbors, ratio: float, iters: int, device: int = 0):
    """``pyqsm_clean_cloud``: the voxel step (``voxel_size`` 0: off), then ``iters`` rounds of
    statistical outlier removal, all in HBM. Returns the points left, float64 [m,3]."""
    pts = _points(points)
    v = 0.0 if not voxel_size else _voxel_size(voxel_size)
    it = int(iters)
    if it < 0:
        raise ValueError(f"iters must be >= 0, got {iters!r}")
    nb, r = float(neighbors), float(ratio)
    if it:
        _stat_args(int(nb), r)
        if int(nb) * 2 ** (it - 1) > 2**31 - 1:
            raise ValueError("neighbors doubled iters - 1 times must fit in int32")
    lib = _lib.load()
    m, px = i64(0), vp()
    check(lib.pyqsm_clean_cloud(_p(pts), pts.shape[0], v, nb, r, it, ctypes.byref(m),
                                ctypes.byref(px), int(device)))
    M = m.value
    return _adopt(lib, px, ctypes.c_double, max(3 * M, 1), np.float64)[:3 * M].reshape(M, 3)


# ---- normals --------------------------------------------------------------------------------
def _search_args(radius, max_nn):
    """(radius, max_nn) of a normal search; radius <= 0, inf or None: KNN search."""
    r = 0.0 if radius is None else float(radius)
    if np.isnan(r):
        raise ValueError("radius must not be NaN")
    hybrid = r > 0 and np.isfinite(r)
    nn = int(max_nn)
    top = 256 if hybrid else 192
    if not 1 <= nn <= top:
        raise ValueError(f"max_nn must be in [1, {top}] for a {'hybrid' if hybrid else 'KNN'} search, got {max_nn!r}")
    return (r if hybrid else 0.0), nn


def _normals_like(normals, n):
    if normals is None:
        return None
    nrm = np.ascontiguousarray(np.asarray(normals), dtype=np.float64)
    if nrm.shape != (n, 3):
        raise ValueError(f"normals must have shape {(n, 3)}, got {nrm.shape}")
    return nrm


def _orient_k(k):
    kk = int(k)
    if not 1 <= kk <= 192:
        raise ValueError(f"k must be in [1, 192], got {k!r}")
    return kk


def estimate_normals(points, radius, max_nn: int, normals=None, device: int = 0):
    """``pyqsm_estimate_normals``: float64 [n,3] unit normals. ``radius`` > 0 and finite: hybrid
    search (up to ``max_nn`` nearest with d2 < radius^2); otherwise the ``max_nn`` nearest.
    ``normals`` (the cloud's previous normals) set the sign and are kept where a neighbourhood
    is degenerate; without them the sign makes n_z >= 0 and the fallback is (0, 0, 1)."""
    pts = _points(points)
    r, nn = _search_args(radius, max_nn)
    n = pts.shape[0]
    prev = _normals_like(normals, n)
    out = np.empty((n, 3), dtype=np.float64)
    check(_lib.load().pyqsm_estimate_normals(_p(pts), n, r, nn, _p(prev), _p(out), int(device)))
    return out


def orient_normals_tangent_plane(points, normals, k: int, return_rounds: bool = False, device: int = 0):
    """``pyqsm_orient_normals_tangent_plane``: the normals with their signs made consistent along
    the minimum spanning forest of the kNN graph (weights 1 - |dot|), each component rooted at
    its highest point with n_z >= 0 there. With ``return_rounds`` also the Boruvka round count."""
    pts = _points(points)
    n = pts.shape[0]
    nrm = _normals_like(normals, n)
    kk = _orient_k(k)
    out = np.empty((n, 3), dtype=np.float64)
    rounds = i32(0)
    check(_lib.load().pyqsm_orient_normals_tangent_plane(_p(pts), n, _p(nrm), kk, _p(out),
                                                         ctypes.byref(rounds), int(device)))
    return (out, rounds.value) if return_rounds else out


def stem_cloud(points, radius, max_nn: int, orient_k: int, angle_cutoff: float, crop_offset: float = 0.5,
               normals=None, device: int = 0):
    """``pyqsm_stem_cloud``: crop, normals, orientation and the angle filter in HBM. Returns
    (kept input indices int64 ascending, their oriented normals float64 [m,3])."""
    pts = _points(points)
    r, nn = _search_args(radius, max_nn)
    n = pts.shape[0]
    prev = _normals_like(normals, n)
    kk = _orient_k(orient_k)
    t = float(angle_cutoff)
    if np.isnan(t):
        raise ValueError("angle_cutoff must not be NaN")
    keep = np.empty(n, dtype=np.int64)
    nrm = np.empty((n, 3), dtype=np.float64)
    m = i64(0)
    check(_lib.load().pyqsm_stem_cloud(_p(pts), n, _p(prev), float(crop_offset), r, nn, kk, t, _p(keep),
                                       _p(nrm), ctypes.byref(m), int(device)))
    return keep[:m.value].copy(), nrm[:m.value].copy()


# ---------------------------------------------------------------- k-means, silhouette, ball step

KMEANS_MAX_K = 8        # PYQSM_KMEANS_MAX_K
KMEANS_MAX_Q = 4        # PYQSM_KMEANS_MAX_Q
SILHOUETTE_MAX_K = 65536


def _xyz_for_xy(data) -> np.ndarray:
    """[m,2] (or [m,3]) as the [m,3] rows the k-means kernels read (z unused)."""
    d = np.asarray(data, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] not in (2, 3):
        raise ValueError(f"expected points of shape [m,2] or [m,3], got {d.shape}")
    if d.shape[1] == 3:
        return np.ascontiguousarray(d)
    out = np.zeros((d.shape[0], 3))
    out[:, :2] = d
    return out


def kmeans(data, init, iters: int = 10, device: int = 0):
    """``pyqsm_kmeans``: Lloyd on the x, y of ``data`` ([m,2] or [m,3]) from the centroids ``init``
    [k,2]. Returns ``(centroids f64 [k,2], labels int32 [m])`` as kmeans2(minit='matrix')."""
    xyz = _xyz_for_xy(data)
    c0 = np.ascontiguousarray(init, dtype=np.float64).reshape(-1, 2)
    k = c0.shape[0]
    cent = np.empty((k, 2))
    labels = np.empty(xyz.shape[0], dtype=np.int32)
    check(_lib.load().pyqsm_kmeans(_p(xyz), xyz.shape[0], k, int(iters), _p(c0), _p(cent), _p(labels),
                                   int(device)))
    return cent, labels


def silhouette(points, labels, k: int | None = None, return_samples: bool = False, device: int = 0):
    """``pyqsm_silhouette``: ``(score, labels present)`` (and the per-point values when
    ``return_samples``) of ``points`` [m,3] under ``labels`` in [0, k)."""
    pts = _points(points)
    lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
    if lab.shape[0] != pts.shape[0]:
        raise ValueError("one label per point")
    k = int(lab.max()) + 1 if k is None and len(lab) else int(k or 1)
    score, present = dbl(0.0), i32(0)
    samples = np.empty(pts.shape[0]) if return_samples else None
    check(_lib.load().pyqsm_silhouette(_p(pts), pts.shape[0], _p(lab), k, ctypes.byref(score),
                                       ctypes.byref(present), _p(samples), int(device)))
    if return_samples:
        return score.value, int(present.value), samples
    return score.value, int(present.value)


def _select_args(m, k0, inits):
    nk = len(inits)
    init = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1, 2)
                                                for c in inits]))
    if init.shape[0] != sum(k0 + q for q in range(nk)):
        raise ValueError("inits[q] must hold k0 + q centroids")
    return nk, init, np.empty((nk, m), dtype=np.int32), np.empty(nk), np.empty(nk, dtype=np.int32)


def kmeans_select(points, k0: int, inits, iters: int = 10, device: int = 0):
    """``pyqsm_kmeans_select``: for q < len(inits), k = k0 + q, Lloyd on the xy of ``points`` [m,3]
    from ``inits[q]`` [k,2], then the silhouette of the 3-D points under those labels. Returns
    ``(labels int32 [nk,m], scores f64 [nk], present int32 [nk])``."""
    pts = _points(points)
    nk, init, labels, scores, present = _select_args(pts.shape[0], k0, inits)
    check(_lib.load().pyqsm_kmeans_select(_p(pts), pts.shape[0], int(k0), nk, int(iters), _p(init),
                                          _p(labels), _p(scores), _p(present), int(device)))
    return labels, scores, present


def kmeans_select_dev(xyz_ptr: int, m: int, k0: int, inits, iters: int = 10, device: int = 0):
    """:func:`kmeans_select` on ``m`` device-resident points (a ball step's gathered buffer)."""
    nk, init, labels, scores, present = _select_args(int(m), k0, inits)
    check(_lib.load().pyqsm_kmeans_select_dev(xyz_ptr, int(m), int(k0), nk, int(iters), _p(init),
                                              _p(labels), _p(scores), _p(present), int(device)))
    return labels, scores, present


def ball_excl_dev(xyz_ptr: int, n: int, found_ptr: int, center, radius: float, idx_ptr: int,
                  out_xyz_ptr: int, device: int = 0) -> int:
    """``pyqsm_ball_excl_dev``: the unfound points within ``radius`` of ``center`` compacted into
    ``idx_ptr`` (int64, ascending) and ``out_xyz_ptr`` (f64 [.,3]); returns how many."""
    c = np.ascontiguousarray(center, dtype=np.float64).reshape(3)
    cnt = i64(0)
    check(_lib.load().pyqsm_ball_excl_dev(xyz_ptr, int(n), found_ptr, _p(c), float(radius), idx_ptr,
                                          out_xyz_ptr, ctypes.byref(cnt), int(device)))
    return int(cnt.value)


def mark_found_dev(found_ptr: int, n: int, idx, device: int = 0) -> None:
    """``pyqsm_mark_found_dev``: set the device mask at the host indices ``idx``."""
    ix = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
    check(_lib.load().pyqsm_mark_found_dev(found_ptr, int(n), _p(ix), ix.shape[0], int(device)))


# ---------------------------------------------------------------- geometric features, smoothing

# jakteristics' FEATURE_NAMES, in its order (the ids pyqsm_geometric_features takes)
FEATURE_NAMES = ("eigenvalue_sum", "omnivariance", "eigenentropy", "anisotropy", "planarity", "linearity",
                 "PCA1", "PCA2", "surface_variation", "sphericity", "verticality", "nx", "ny", "nz")
SMOOTH_MAX_K = 192
SMOOTH_REDUCERS = {"mean": 0, "median": 1, "min": 2, "amin": 2, "max": 3, "amax": 3}


def feature_ids(feature_names) -> np.ndarray:
    """The FEATURE_NAMES ids of ``feature_names`` (a name or a sequence of names), in that order;
    ValueError naming the valid ones for anything else."""
    names = [feature_names] if isinstance(feature_names, str) else list(feature_names)
    if not 1 <= len(names) <= 32:
        raise ValueError(f"between 1 and 32 feature names are needed, got {len(names)}")
    bad = [f for f in names if f not in FEATURE_NAMES]
    if bad:
        raise ValueError(f"unknown feature name(s) {bad}; valid names: {', '.join(FEATURE_NAMES)}")
    return np.array([FEATURE_NAMES.index(f) for f in names], dtype=np.int32)


def _feature_args(radius, max_k, metric):
    r = float(radius)
    if not (r > 0 and np.isfinite(r)):
        raise ValueError(f"radius must be positive and finite, got {radius!r}")
    mk = int(max_k)
    if not 1 <= mk <= 0x7FFFFFFF:
        raise ValueError(f"max_k must be in [1, 2^31 - 1], got {max_k!r}")
    codes = {"euclidean": 2, "l2": 2, "manhattan": 1, "l1": 1, "cityblock": 1}
    if metric not in codes:
        raise ValueError(f"metric must be one of {sorted(codes)}, got {metric!r}")
    return r, mk, codes[metric]


def geometric_features(points, radius, feature_names=None, max_k: int = 50000, metric: str = "euclidean",
                       return_counts: bool = False, device: int = 0):
    """``pyqsm_geometric_features``: float64 [n, F] eigenvalue features of every point's ball
    (jakteristics' formulas, columns in the order of ``feature_names``, all 14 when None); NaN
    where fewer than 3 points were kept or lambda1 == 0. ``metric`` "euclidean" or "manhattan".
    With ``return_counts`` also the int32 [n] ball counts before the ``max_k`` cap."""
    ids = feature_ids(FEATURE_NAMES if feature_names is None else feature_names)
    r, mk, code = _feature_args(radius, max_k, metric)
    pts = _points(points)
    n = pts.shape[0]
    out = np.empty((n, len(ids)), dtype=np.float64)
    cnt = np.empty(n, dtype=np.int32)
    check(_lib.load().pyqsm_geometric_features(_p(pts), n, r, mk, code, _p(ids), len(ids), _p(out), _p(cnt),
                                               int(device)))
    return (out, cnt) if return_counts else out


def smooth_reducer(reducer):
    """The device code of a reducer (np.mean, np.median, np.min / np.amin, np.max / np.amax or
    those names), or None for any other callable (reduced on the host)."""
    if isinstance(reducer, str):
        if reducer not in SMOOTH_REDUCERS:
            raise ValueError(f"reducer must be one of {sorted(SMOOTH_REDUCERS)} or a callable, got {reducer!r}")
        return SMOOTH_REDUCERS[reducer]
    for name, code in SMOOTH_REDUCERS.items():
        if reducer is getattr(np, name, None):
            return code
    if not callable(reducer):
        raise ValueError(f"reducer must be a name or a callable, got {reducer!r}")
    return None


def _smooth_k(k, n):
    kk = int(k)
    if not 1 <= kk <= SMOOTH_MAX_K:
        raise ValueError(f"k must be in [1, {SMOOTH_MAX_K}], got {k!r}")
    if kk > n:
        raise ValueError(f"Expected n_neighbors <= n_samples, but n_samples = {n}, n_neighbors = {kk}")
    return kk


def smooth_values(points, values, k: int, reducer="mean", queries=None, return_indices: bool = False,
                  device: int = 0):
    """``pyqsm_smooth_values``: ``reducer`` over the values of each query's ``k`` nearest points
    (ascending by (d2, index); the queries are the points themselves when ``queries`` is None).
    ``values`` [n] or [n, F] gives [m] or [m, F]. np.mean / np.median / np.min / np.max (or their
    names) reduce on the device; any other callable gets ``values[idx]`` ([m, k, ...]) with
    ``axis=1`` on the host. The result has the dtype NumPy's reducer would give. With
    ``return_indices`` also the int64 [m, k] neighbour table."""
    pts = _points(points)
    n = pts.shape[0]
    vals = np.asarray(values)
    if vals.ndim not in (1, 2) or vals.shape[0] != n:
        raise ValueError(f"values must have shape [{n}] or [{n}, F], got {vals.shape}")
    kk = _smooth_k(k, n)
    code = smooth_reducer(reducer)
    qry = None if queries is None else _points(queries)
    if qry is not None and not np.isfinite(qry).all():
        raise ValueError("query coordinates must be finite")
    m = n if qry is None else qry.shape[0]
    is_int = vals.dtype.kind in "iub"
    big_int = is_int and vals.size and np.abs(vals.astype(np.float64)).max() >= 2.0 ** 53
    if vals.dtype.kind not in "iubf" or (big_int and code in (2, 3)):
        code = None                                # exact on the host, from the GPU's table
    host = code is None
    want_idx = host or return_indices
    idx = np.empty((m, kk), dtype=np.int32) if want_idx else None
    F = 1 if vals.ndim == 1 else vals.shape[1]
    if host:
        check(_lib.load().pyqsm_smooth_values(_p(pts), n, _p(qry), m, None, F, kk, -1, None, _p(idx), int(device)))
        red = getattr(np, reducer) if isinstance(reducer, str) else reducer
        res = red(vals[idx], axis=1)
    else:
        v64 = np.ascontiguousarray(vals.reshape(n, F), dtype=np.float64)
        out = np.empty((m, F), dtype=np.float64)
        check(_lib.load().pyqsm_smooth_values(_p(pts), n, _p(qry), m, _p(v64), F, kk, code, _p(out), _p(idx),
                                              int(device)))
        res = out if vals.ndim == 2 else out[:, 0]
        if vals.dtype.kind == "f" or code in (2, 3):   # integers: float64 for mean and median
            res = res.astype(vals.dtype)
    if return_indices:
        return res, idx.astype(np.int64)
    return res


# ---------------------------------------------------------------- tree-ensemble inference

FOREST_MAX_FEATURES = 64
FOREST_MAX_CLASSES = 32
FOREST_MAX_TREE_NODES = 1 << 22
FOREST_STAGED = (0, 512, 1024, 2048)


def forest_rows(X, n_features: int) -> np.ndarray:
    """``X`` as C-contiguous float32 [n, n_features], checked as scikit-learn checks it for a tree:
    NaN passes, ±inf or a finite value beyond float32's range raises ValueError."""
    a = np.asarray(X)
    if a.dtype.kind not in "iubf":
        raise ValueError(f"X must be numeric, got dtype {a.dtype}")
    if a.ndim != 2:
        raise ValueError(f"Expected 2D array, got {a.ndim}D array instead")
    if a.shape[1] != n_features:
        raise ValueError(f"X has {a.shape[1]} features, but the forest is expecting {n_features} features as input.")
    with np.errstate(over="ignore"):
        x = np.ascontiguousarray(a, dtype=np.float32)
    if np.isinf(x).any():
        raise ValueError("Input X contains infinity or a value too large for dtype('float32').")
    return x


class DeviceForest:
    """A fitted tree ensemble resident in HBM (``pyqsm_forest_create``): the trees' nodes
    concatenated, tree k in ``tree_offsets[k]:tree_offsets[k+1]``, children as node numbers within
    their tree (-1: leaf), ``value`` [nodes, C]. Context manager like :class:`DeviceMesh`."""

    def __init__(self, tree_offsets, left, right, feature, threshold, missing_left, value, n_features: int,
                 device: int = 0):
        off = np.ascontiguousarray(tree_offsets, dtype=np.int64)
        if off.ndim != 1 or off.size < 2 or off[0] != 0 or (np.diff(off) < 1).any():
            raise ValueError("tree_offsets must be [T+1], start at 0 and ascend by at least one node per tree")
        nodes = int(off[-1])
        lt = np.ascontiguousarray(left, dtype=np.int32)
        rt = np.ascontiguousarray(right, dtype=np.int32)
        ft = np.ascontiguousarray(feature, dtype=np.int32)
        th = np.ascontiguousarray(threshold, dtype=np.float64)
        ml = np.ascontiguousarray(missing_left, dtype=np.uint8)
        val = np.ascontiguousarray(value, dtype=np.float64)
        for name, a in (("left", lt), ("right", rt), ("feature", ft), ("threshold", th), ("missing_left", ml)):
            if a.shape != (nodes,):
                raise ValueError(f"{name} must have shape [{nodes}], got {a.shape}")
        if val.ndim != 2 or val.shape[0] != nodes or val.shape[1] < 1:
            raise ValueError(f"value must have shape [{nodes}, C], got {val.shape}")
        self.n_trees, self.n_classes, self.n_features = off.size - 1, int(val.shape[1]), int(n_features)
        if not 1 <= self.n_features <= FOREST_MAX_FEATURES:
            raise ValueError(f"n_features must be in [1, {FOREST_MAX_FEATURES}], got {n_features!r}")
        if self.n_classes > FOREST_MAX_CLASSES:
            raise ValueError(f"at most {FOREST_MAX_CLASSES} classes, got {self.n_classes}")
        if int(np.diff(off).max()) > FOREST_MAX_TREE_NODES:
            raise ValueError(f"at most {FOREST_MAX_TREE_NODES} nodes per tree, got {int(np.diff(off).max())}")
        self.device = int(device)
        self._h = None
        h = vp()
        check(_lib.load().pyqsm_forest_create(_p(off), _p(lt), _p(rt), _p(ft), _p(th), _p(ml), _p(val),
                                              self.n_trees, self.n_classes, self.n_features, self.device,
                                              ctypes.byref(h)))
        self._h = h.value

    def _handle(self):
        if not self._h:
            raise ValueError("the forest has been freed")
        return self._h

    def info(self) -> dict:
        """T, C, F, the node records and leaves on the device, the deepest leaf, device bytes and
        the nodes of each tree the kernel reads from LDS (``pyqsm_forest_info``)."""
        out = np.zeros(8, dtype=np.int64)
        check(_lib.load().pyqsm_forest_info(self._handle(), _p(out)))
        keys = ("n_trees", "n_classes", "n_features", "nodes", "leaves", "max_depth", "device_bytes", "staged_nodes")
        return dict(zip(keys, (int(v) for v in out)))

    def stage(self, staged_nodes: int) -> None:
        """How many of each tree's first nodes are read from LDS (speed only; 0, 512, 1024, 2048)."""
        if staged_nodes not in FOREST_STAGED:
            raise ValueError(f"staged_nodes must be one of {FOREST_STAGED}, got {staged_nodes!r}")
        check(_lib.load().pyqsm_forest_stage(self._handle(), int(staged_nodes)))

    def predict(self, X, proba: bool = True, label: bool = True, leaves: bool = False):
        """One pass over the rows (``pyqsm_forest_predict``): (proba f64 [n, C], label i32 [n] class
        index, leaves i32 [n, T]), None for what was not asked for."""
        h = self._handle()
        x = forest_rows(X, self.n_features)
        n = x.shape[0]
        p = np.empty((n, self.n_classes), dtype=np.float64) if proba else None
        lab = np.empty(n, dtype=np.int32) if label else None
        lv = np.empty((n, self.n_trees), dtype=np.int32) if leaves else None
        check(_lib.load().pyqsm_forest_predict(h, _p(x), n, _p(p), _p(lab), _p(lv)))
        return p, lab, lv

    def predict_proba(self, X) -> np.ndarray:
        return self.predict(X, True, False, False)[0]

    def predict_index(self, X) -> np.ndarray:
        return self.predict(X, False, True, False)[1]

    def apply(self, X) -> np.ndarray:
        return self.predict(X, False, False, True)[2]

    def free(self) -> None:
        if self._h:
            _lib.load().pyqsm_forest_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---------------------------------------------------------------- detail recovery

VOX_INVERT = 1
RADIUS_REDUCERS = {"mean": 0, "min": 2, "amin": 2, "max": 3, "amax": 3, "first": 4}
RADIUS_REDUCE_MAX_K = 2048
RADIUS_REDUCE_MAX_F = 64


class VoxelGrid:
    """The occupied voxels of a cloud resident in HBM (``pyqsm_voxel_grid_create``): created once,
    queried by any number of tiles. ``origin`` = min bound - voxel_size / 2, ``dims`` = largest voxel
    index + 1 per axis, rows ordered by the smallest input index each voxel holds. Context manager
    like :class:`DeviceForest`."""

    def __init__(self, points, voxel_size: float, colors=None, device: int = 0):
        pts = _points(points)
        v = _voxel_size(voxel_size)
        col = None
        if colors is not None:
            col = np.ascontiguousarray(np.asarray(colors), dtype=np.float64)
            if col.shape != pts.shape:
                raise ValueError(f"colors must have the points' shape {pts.shape}, got {col.shape}")
        self.device = int(device)
        self.has_colors = col is not None
        self._h = None
        h = vp()
        lib = _lib.load()
        check(lib.pyqsm_voxel_grid_create(_p(pts), pts.shape[0], _p(col), v, self.device, ctypes.byref(h)))
        self._h = h.value
        origin, dims = np.zeros(3), np.zeros(3, dtype=np.int64)
        size, m, nbytes = dbl(0), i64(0), i64(0)
        check(lib.pyqsm_voxel_grid_info(self._h, _p(origin), ctypes.byref(size), _p(dims), ctypes.byref(m),
                                        ctypes.byref(nbytes)))
        self.origin, self.dims, self.voxel_size = origin, dims, float(size.value)
        self.n_voxels, self.device_bytes = int(m.value), int(nbytes.value)

    def _handle(self):
        if not self._h:
            raise ValueError("the voxel grid has been freed")
        return self._h

    def query(self, points, rows: bool = False, indices: bool = False, invert: bool = False):
        """``pyqsm_voxel_grid_query``: ``included`` bool [m]; with ``rows`` also the voxel row of every
        point (int32, -1: none); with ``indices`` also the ascending int64 indices of the included
        points (``invert``: of those that are not). One value, or a tuple in that order."""
        h = self._handle()
        q = _points(points)
        m = q.shape[0]
        inc = np.zeros(m, dtype=np.uint8)
        row = np.empty(m, dtype=np.int32) if rows else None
        idx = np.empty(max(m, 1), dtype=np.int64) if indices else None
        cnt = i64(0)
        check(_lib.load().pyqsm_voxel_grid_query(h, _p(q), m, VOX_INVERT if invert else 0, _p(inc), _p(row), _p(idx),
                                                 ctypes.byref(cnt)))
        out = [inc.astype(bool)]
        if rows:
            out.append(row)
        if indices:
            out.append(idx[:cnt.value].copy())
        return out[0] if len(out) == 1 else tuple(out)

    def query_dev(self, qry_ptr: int, m: int, included_ptr=None, row_ptr=None, idx_ptr=None,
                  invert: bool = False) -> int:
        """``pyqsm_voxel_grid_query_dev`` on device arrays (qry f64 [m,3]; included u8 [m], row i32
        [m], idx i64 [capacity m], each may be None). Returns the number of listed queries."""
        cnt = i64(0)
        check(_lib.load().pyqsm_voxel_grid_query_dev(self._handle(), vp(qry_ptr), int(m), VOX_INVERT if invert else 0,
                                                     vp(included_ptr), vp(row_ptr), vp(idx_ptr), ctypes.byref(cnt)))
        return int(cnt.value)

    def voxels(self):
        """(grid_index int32 [M,3], colour means f64 [M,3] or None) in row order."""
        h = self._handle()
        gi = np.zeros((self.n_voxels, 3), dtype=np.int32)
        col = np.zeros((self.n_voxels, 3), dtype=np.float64) if self.has_colors else None
        check(_lib.load().pyqsm_voxel_grid_voxels(h, _p(gi), _p(col)))
        return gi, col

    def close(self) -> None:
        if self._h:
            _lib.load().pyqsm_voxel_grid_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def radius_reducer(reducer) -> int:
    """The device code of a reducer name (``mean``, ``min``, ``max``, ``first``) or of np.mean /
    np.min / np.max."""
    if isinstance(reducer, str):
        if reducer not in RADIUS_REDUCERS:
            raise ValueError(f"reducer must be one of {sorted(RADIUS_REDUCERS)}, got {reducer!r}")
        return RADIUS_REDUCERS[reducer]
    for name in ("mean", "min", "amin", "max", "amax"):
        if reducer is getattr(np, name, None):
            return RADIUS_REDUCERS[name]
    raise ValueError(f"reducer must be one of {sorted(RADIUS_REDUCERS)}, got {reducer!r}")


def radius_reduce(src, queries, values, radius: float, k: int = 500, reducer="mean", empty_row: int = 0,
                  return_counts: bool = False, device: int = 0):
    """``pyqsm_radius_reduce``: ``reducer`` over ``values`` ([n] or [n, F], as float64) of every query's
    neighbours — the entries ``radius_knn(src, queries, radius, k)`` returns for it — as float64 [m]
    or [m, F]. A query without neighbours gets ``values[empty_row]``, NaN for ``empty_row=-1``. With
    ``return_counts`` also the int32 [m] neighbour counts."""
    s = _points(src)
    q = _points(queries)
    n, m = s.shape[0], q.shape[0]
    vals = np.asarray(values)
    if vals.ndim not in (1, 2) or vals.shape[0] != n:
        raise ValueError(f"values must have shape [{n}] or [{n}, F], got {vals.shape}")
    F = 1 if vals.ndim == 1 else vals.shape[1]
    v64 = np.ascontiguousarray(vals.reshape(n, F), dtype=np.float64)
    out = np.empty((m, F), dtype=np.float64)
    cnt = np.zeros(m, dtype=np.int32) if return_counts else None
    check(_lib.load().pyqsm_radius_reduce(_p(s), n, _p(q), m, float(radius), int(k), _p(v64), int(F),
                                          radius_reducer(reducer), int(empty_row), _p(out), _p(cnt), int(device)))
    res = out if vals.ndim == 2 else out[:, 0]
    return (res, cnt) if return_counts else res


# ---------------------------------------------------------------- skeleton graph and cylinder table

def _edge_list(edges) -> np.ndarray:
    e = np.ascontiguousarray(np.asarray(edges), dtype=np.int32)
    if e.size == 0:
        return e.reshape(0, 2)
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError(f"expected edges of shape [e,2], got {e.shape}")
    return e


def skeletal_forest(points, k: int, return_rounds: bool = False, device: int = 0):
    """``pyqsm_skeletal_forest``: the minimum spanning forest of the undirected kNN graph. Returns
    (edges int32 [e,2] with a < b, rows ascending; d2 float64 [e], the kNN's own squared distances);
    with ``return_rounds`` also the Boruvka round count. ``len(points) - e`` components."""
    pts = _points(points)
    m = pts.shape[0]
    edges = np.empty((max(m - 1, 0), 2), dtype=np.int32)
    d2 = np.empty(max(m - 1, 0), dtype=np.float64)
    ne, rounds = i64(0), i32(0)
    check(_lib.load().pyqsm_skeletal_forest(_p(pts), m, int(k), _p(edges), _p(d2), ctypes.byref(ne),
                                            ctypes.byref(rounds), int(device)))
    edges, d2 = edges[:ne.value].copy(), d2[:ne.value].copy()
    return (edges, d2, rounds.value) if return_rounds else (edges, d2)


def skeletal_forest_dev(xyz_ptr: int, m: int, k: int, edges_ptr: int, d2_ptr: int, device: int = 0):
    """The same on device arrays (edges int32 [m - 1, 2], d2 float64 [m - 1]): (edge count, rounds)."""
    ne, rounds = i64(0), i32(0)
    check(_lib.load().pyqsm_skeletal_forest_dev(xyz_ptr, int(m), int(k), edges_ptr, d2_ptr, ctypes.byref(ne),
                                                ctypes.byref(rounds), int(device)))
    return int(ne.value), int(rounds.value)


def collapse_chains(edges, n_nodes: int, device: int = 0):
    """``pyqsm_collapse_chains`` on a forest: (kept int32 ascending, chain_ends int32 [c,2],
    chain_ptr int64 [c+1], members int32)."""
    e = _edge_list(edges)
    m, ne = int(n_nodes), e.shape[0]
    if m < 0:
        raise ValueError("n_nodes must not be negative")
    kept = np.empty(m, dtype=np.int32)
    ends = np.empty((ne, 2), dtype=np.int32)
    ptr = np.zeros(ne + 1, dtype=np.int64)
    members = np.empty(m, dtype=np.int32)
    counts = np.zeros(3, dtype=np.int64)
    check(_lib.load().pyqsm_collapse_chains(_p(e), ne, m, _p(kept), _p(ends), _p(ptr), _p(members), _p(counts),
                                            int(device)))
    nk, nc, nm = (int(v) for v in counts)
    return kept[:nk].copy(), ends[:nc].copy(), ptr[:nc + 1].copy(), members[:nm].copy()


def collapse_chains_dev(edges_ptr: int, e: int, m: int, kept_ptr: int, ends_ptr: int, ptr_ptr: int,
                        members_ptr: int, device: int = 0):
    """The same on device arrays of the worst-case sizes m, e, e + 1, m: (kept, chains, members) counts."""
    counts = np.zeros(3, dtype=np.int64)
    check(_lib.load().pyqsm_collapse_chains_dev(edges_ptr, int(e), int(m), kept_ptr, ends_ptr, ptr_ptr,
                                                members_ptr, _p(counts), int(device)))
    return tuple(int(v) for v in counts)


def chain_radii(shift, chain_ptr, members, index_map=None, device: int = 0) -> np.ndarray:
    """``pyqsm_chain_radii``: float64 [c], the mean |shift| over every chain's members (through
    ``index_map`` when given); 0 for a chain without members."""
    sh = _points(shift)
    ptr = np.ascontiguousarray(chain_ptr, dtype=np.int64)
    mem = np.ascontiguousarray(members, dtype=np.int32)
    if ptr.ndim != 1 or len(ptr) < 1 or mem.ndim != 1 or int(ptr[-1]) != len(mem):
        raise ValueError("chain_ptr must be [c+1] and end at len(members)")
    imap = None if index_map is None else np.ascontiguousarray(index_map, dtype=np.int32)
    nc = len(ptr) - 1
    out = np.empty(nc, dtype=np.float64)
    check(_lib.load().pyqsm_chain_radii(_p(sh), sh.shape[0], _p(ptr), nc, _p(mem), _p(imap),
                                        0 if imap is None else len(imap), _p(out), int(device)))
    return out


def cylinder_surfaces(params, cos_sin, device: int = 0):
    """``pyqsm_cylinder_surfaces``: params float64 [q,14] (centre, unit axis, u, v, radius, height),
    cos_sin float64 [40]. Returns (points float64 [t,3], surface_ptr int64 [q+1])."""
    par = np.ascontiguousarray(params, dtype=np.float64)
    if par.size == 0:
        par = par.reshape(0, 14)
    if par.ndim != 2 or par.shape[1] != 14:
        raise ValueError(f"expected params of shape [q,14], got {par.shape}")
    cs = np.ascontiguousarray(cos_sin, dtype=np.float64).ravel()
    if cs.shape[0] != 40:
        raise ValueError("cos_sin must hold 20 cosines and 20 sines")
    q = par.shape[0]
    lib = _lib.load()
    ptr = np.zeros(q + 1, dtype=np.int64)
    out, total = vp(), i64(0)
    check(lib.pyqsm_cylinder_surfaces(_p(par), q, _p(cs), _p(ptr), ctypes.byref(out), ctypes.byref(total),
                                      int(device)))
    if total.value == 0 or not out.value:
        return np.zeros((0, 3), dtype=np.float64), ptr
    pts = _adopt(lib, out, ctypes.c_double, total.value * 3, np.float64).reshape(-1, 3)
    return pts, ptr
