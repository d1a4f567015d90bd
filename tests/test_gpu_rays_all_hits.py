"""The all-hits path of raycast.hip (k_all_hits<0>, k_all_hits<1>, k_scan_counts_serial behind
pyqsm_list_intersections; it carries RaycastingScene.list_intersections, count_intersections,
compute_occupancy and the sign of compute_signed_distance):

  * against the INDEPENDENT fp64 evaluation of oracle/ray_f64.c over all ray x triangle pairs
    (tests/allhits_cases.py; a mirror shares any error of formulation), and bit for bit against the
    mirror oracle.list_intersections;
  * at the ray counts where the launch and the one-block 64-bit offset scan change shape (the
    256-ray block, the 1024-ray scan chunk and its carry), at T in {0, 1, 2, 3}, with no hit at
    all (the second launch is skipped) and with no ray;
  * on a stack of 300 sheets in shuffled order: counts beyond 8 bits, records in triangle-id
    order although depth order differs, exact t, only the sheets in front of the origin;
  * through the C-ABI with hits_cap below, at and above the total: a prefix, nothing written
    beyond it;
  * against the closest hit of all three closest-hit kernel families, every ray, bit for bit;
  * with zero-direction and non-finite rays mixed in, and through the wrappers built on it.

Every case is brute force over at most 3073 rays x 3000 triangles per call."""
import ctypes

import numpy as np
import pytest

import oracle
from pyqsm_amd import _lib, hip, synth
from pyqsm_amd.viz import ray_casting as rc

from tests import allhits_cases as ac
from tests import meshdist_cases as mc

pytestmark = pytest.mark.gpu

MAX_RAYS = 3073


def _same(got, ref, what=""):
    for k in ac.KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        # bit for bit: t and uv compared as the integers they are stored as (-0.0 != 0.0, NaN == NaN)
        assert np.array_equal(got[k].view(np.uint32) if got[k].dtype == np.float32 else got[k],
                              ref[k].view(np.uint32) if ref[k].dtype == np.float32 else ref[k]), (what, k)


def _empty(result, R):
    assert result["counts"].dtype == np.int32 and result["counts"].shape == (R,)
    assert not result["counts"].any()
    for k, dt, shape in (("ray_ids", np.uint32, (0,)), ("primitive_ids", np.uint32, (0,)),
                         ("t_hit", np.float32, (0,)), ("primitive_uvs", np.float32, (0, 2))):
        assert result[k].dtype == dt and result[k].shape == shape, k


# ------------------------------------------------------------------ independent reference

@pytest.mark.parametrize("name", list(ac.CASES))
def test_all_hits_against_independent_fp64(gpu, name):
    v, t, rays = ac.case(name)
    got = hip.list_intersections(v, t, rays, device=gpu)
    rec = ac.compare_all_hits(got, v, t, rays)
    print(f"{name} vs fp64:", rec)
    ac.check_record(rec)
    _same(got, oracle.list_intersections(v, t, rays), name)


# ------------------------------------------------------------------ shape edges

EDGE_R = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
CHUNK_EDGES = (1023, 1024, 2047, 2048)


@pytest.fixture(scope="module")
def edge_batches():
    """(verts, tris, {name: rays [3073, 6]}, {name: mirror result}). "carry": the same rays with
    four that cross at least two leaves moved to the indices on either side of each edge of the
    scan's 1024-ray chunks, so that the offset carried across an edge is followed by records."""
    v, t = synth.canopy_mesh(300, seed=5, side=0.6)
    plain = synth.sun_rays(v, MAX_RAYS)
    counts = oracle.list_intersections(v, t, plain)["counts"]
    donors = [int(i) for i in np.flatnonzero(counts >= 2) if int(i) not in CHUNK_EDGES][:len(CHUNK_EDGES)]
    assert len(donors) == len(CHUNK_EDGES)
    order = np.arange(MAX_RAYS)
    for at, frm in zip(CHUNK_EDGES, donors):
        order[[at, frm]] = order[[frm, at]]
    rays = {"plain": plain, "carry": np.ascontiguousarray(plain[order])}
    ref = {k: oracle.list_intersections(v, t, r) for k, r in rays.items()}
    assert (ref["carry"]["counts"][list(CHUNK_EDGES)] >= 2).all()
    assert ref["plain"]["counts"][:1023].sum() > 0                   # a non-zero carry at the first edge
    for a in (v, t, *rays.values(), *(x for r in ref.values() for x in r.values())):
        a.setflags(write=False)
    return v, t, rays, ref


@pytest.mark.parametrize("batch", ["plain", "carry"])
@pytest.mark.parametrize("R", EDGE_R)
def test_ray_count_edges(gpu, edge_batches, batch, R):
    v, t, rays, ref = edge_batches
    full = ref[batch]
    got = hip.list_intersections(v, t, rays[batch][:R], device=gpu)
    _same(got, oracle.list_intersections(v, t, rays[batch][:R]), (batch, R))
    # ... and the first R rays of the whole batch, ray by ray through counts and offsets
    assert np.array_equal(got["counts"], full["counts"][:R])
    begin, end = ac.split_by_ray(full)
    gb, ge = ac.split_by_ray(got)
    assert np.array_equal(gb, begin[:R]) and np.array_equal(ge, end[:R])
    n = int(end[R - 1])
    assert len(got["ray_ids"]) == n
    assert np.array_equal(got["ray_ids"], np.repeat(np.arange(R, dtype=np.uint32), got["counts"]))
    for k in ac.KEYS[1:]:
        assert np.array_equal(got[k], full[k][:n]), (batch, R, k)
    if R == MAX_RAYS:
        assert got["counts"].max() >= 2 and n > 1000


# ------------------------------------------------------------------ triangle-count edges

TRI_V = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [1, 0, 0]], np.float32)
TRI_T = np.array([[0, 1, 2], [0, 1, 2], [0, 3, 1]], np.int32)        # one, its duplicate, a zero-area one


def _rays_over_triangle(n=300, seed=3):
    """vertical rays over [-0.5, 2.5]^2 from both sides, a third of them through the triangle,
    some along its degenerate companion's line y = 0"""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, 6), np.float32)
    r[:, :2] = rng.uniform(-0.5, 2.5, (n, 2))
    r[::7, 1] = 0.0
    r[:, 2] = np.where(np.arange(n) % 2, 3.0, -3.0)
    r[:, 5] = -r[:, 2] / 3
    return r


@pytest.mark.parametrize("T", [1, 2, 3])
def test_one_two_three_triangles(gpu, T):
    rays = _rays_over_triangle()
    got = hip.list_intersections(TRI_V, TRI_T[:T], rays, device=gpu)
    _same(got, oracle.list_intersections(TRI_V, TRI_T[:T], rays), T)
    x, y = rays[:, 0].astype(np.float64), rays[:, 1].astype(np.float64)
    inside = (x >= 0) & (y >= 0) & (x + y <= 2)                       # edges inclusive; exact in fp32 here
    assert 50 < inside.sum() < 250
    assert np.array_equal(got["counts"], np.where(inside, min(T, 2), 0))
    assert not (got["primitive_ids"] == 2).any()                      # the zero-area triangle is never listed
    assert (got["t_hit"] == 3.0).all()
    rec = ac.compare_all_hits(got, TRI_V, TRI_T[:T], rays)
    assert rec["structure"] == [] and rec["unexplained"] == 0, rec


def test_no_triangles_no_hits_no_rays(gpu):
    v, t = synth.canopy_mesh(300, seed=5, side=0.6)
    rays = synth.sun_rays(v, 1500)
    # T = 0
    _empty(hip.list_intersections(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), rays, device=gpu), 1500)
    _empty(hip.list_intersections(v, np.zeros((0, 3), np.int32), rays, device=gpu), 1500)
    # every ray misses: total == 0, the record launch is skipped
    away = rays.copy()
    away[:, 0] += 100.0
    got = hip.list_intersections(v, t, away, device=gpu)
    _empty(got, 1500)
    _same(got, oracle.list_intersections(v, t, away), "all miss")
    behind = rays.copy()
    behind[:, 3:] *= -1                                               # the canopy lies at t < 0
    _empty(hip.list_intersections(v, t, behind, device=gpu), 1500)
    # R = 0
    _empty(hip.list_intersections(v, t, np.zeros((0, 6), np.float32), device=gpu), 0)
    # ... and the call after them is unaffected
    _same(hip.list_intersections(v, t, rays, device=gpu), oracle.list_intersections(v, t, rays), "after")


# ------------------------------------------------------------------ deep stack and order

N_SHEETS = 300


def _sheets():
    """300 unit squares (triangles 2k: y <= x, 2k + 1: y >= x) at the integer heights 1..300,
    shuffled: triangle-id order is not depth order."""
    h = np.random.default_rng(12).permutation(N_SHEETS) + 1
    sq = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    v = np.concatenate([np.c_[sq, np.full(4, z, np.float32)] for z in h])
    t = np.concatenate([np.array([[0, 1, 2], [0, 2, 3]]) + 4 * k for k in range(N_SHEETS)]).astype(np.int32)
    return v, t, h


def _xy(n, seed):
    """generic interior points, clear of the squares' edges and of the diagonal y = x"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.05, 0.95, (4 * n, 2)).astype(np.float32)
    return xy[np.abs(xy[:, 0] - xy[:, 1]) > 0.02][:n]


def _expected_stack(rays, h):
    """The exact list for vertical rays (d = (0, 0, +-1)) over the sheets: every product is exact."""
    out = {k: [] for k in ac.KEYS}
    for r, (x, y, z, _, _, dz) in enumerate(rays):
        inside = 0 < x < 1 and 0 < y < 1
        front = np.flatnonzero((h - z) * dz > 0) if inside else np.zeros(0, np.int64)   # ascending sheet id
        lower = y < x
        out["counts"].append(len(front))
        out["ray_ids"].append(np.full(len(front), r))
        out["primitive_ids"].append(2 * front + (0 if lower else 1))
        out["t_hit"].append((h[front] - z) * dz)
        u, w = (np.float32(x) - np.float32(y), y) if lower else (x, np.float32(y) - np.float32(x))
        out["primitive_uvs"].append(np.tile(np.float32([u, w]), (len(front), 1)))
    return {"counts": np.array(out["counts"], np.int32),
            "ray_ids": np.concatenate(out["ray_ids"]).astype(np.uint32),
            "primitive_ids": np.concatenate(out["primitive_ids"]).astype(np.uint32),
            "t_hit": np.concatenate(out["t_hit"]).astype(np.float32),
            "primitive_uvs": np.concatenate(out["primitive_uvs"]).astype(np.float32).reshape(-1, 2)}


def test_deep_stack_lists_in_triangle_order(gpu):
    v, t, h = _sheets()
    xy = _xy(70, seed=13)
    rays = np.zeros((80, 6), np.float32)
    rays[:70, :2] = xy
    rays[:70, 2] = np.where(np.arange(70) % 2, 400.0, -7.0)           # from above and from below
    rays[70:, :2] = np.float32([[1.5, 0.5], [-0.25, 0.5], [0.5, 1.25], [0.5, -3], [7, 7]] * 2)
    rays[70:, 2] = np.where(np.arange(10) % 2, 400.0, -7.0)
    rays[:, 5] = np.where(rays[:, 2] > 0, -1.0, 1.0)
    rays = rays[np.random.default_rng(14).permutation(80)]            # the misses among the hits
    got = hip.list_intersections(v, t, rays, device=gpu)
    want = _expected_stack(rays, h)
    _same(got, want, "stack")
    _same(got, oracle.list_intersections(v, t, rays), "stack, mirror")
    assert sorted(set(got["counts"].tolist())) == [0, N_SHEETS] and (got["counts"] == N_SHEETS).sum() == 70
    begin, end = ac.split_by_ray(got)
    for b, e in zip(begin[got["counts"] > 0], end[got["counts"] > 0]):
        assert (np.diff(got["primitive_ids"][b:e].astype(np.int64)) > 0).all()
        assert (np.diff(got["t_hit"][b:e]) < 0).any() and (np.diff(got["t_hit"][b:e]) > 0).any()
        assert np.array_equal(np.sort(got["t_hit"][b:e]), np.arange(N_SHEETS) + got["t_hit"][b:e].min())


def test_deep_stack_lists_only_what_lies_ahead(gpu):
    v, t, h = _sheets()
    xy = _xy(12, seed=15)
    rays = np.zeros((12, 6), np.float32)
    rays[:, :2] = xy
    #            between two sheets      exactly on a sheet      on the outermost sheets
    rays[:, 2] = [150.5, 150.5, 0.5, 299.5, 150, 150, 1, 1, 300, 300, 37, 262]
    rays[:, 5] = [-1, 1, -1, 1, -1, 1, 1, -1, 1, -1, 2, -0.5]
    got = hip.list_intersections(v, t, rays, device=gpu)
    assert got["counts"].tolist() == [150, 150, 0, 1, 149, 150, 299, 0, 0, 299, 263, 261]
    want = _expected_stack(rays, h)
    want["t_hit"] = (want["t_hit"] / np.repeat(np.abs(rays[:, 5]), want["counts"]) ** 2).astype(np.float32)
    _same(got, want, "ahead")                                         # t in units of |d|: exact halves and doubles
    _same(got, oracle.list_intersections(v, t, rays), "ahead, mirror")
    assert (got["t_hit"] > 0).all()


# ------------------------------------------------------------------ C-ABI hits_cap

SENTINEL_U32 = np.uint32(0xDEADBEEF)
SENTINEL_F32 = np.float32(-12345.0)


def _call(gpu, v, t, rays, cap, pad=16, null_records=False):
    n = max(cap, 0) + pad
    counts = np.full(len(rays), -99, np.int32)
    rid, pid = np.full(n, SENTINEL_U32), np.full(n, SENTINEL_U32)
    ts, uv = np.full(n, SENTINEL_F32), np.full((n, 2), SENTINEL_F32)
    total = ctypes.c_int64(-5)
    ptr = (lambda a: None) if null_records else hip._p
    code = _lib.load().pyqsm_list_intersections(hip._p(v), len(v), hip._p(t), len(t), hip._p(rays), len(rays),
                                                hip._p(counts), ptr(rid), ptr(pid), ptr(ts), ptr(uv), cap,
                                                ctypes.byref(total), gpu)
    return code, int(total.value), {"counts": counts, "ray_ids": rid, "primitive_ids": pid, "t_hit": ts,
                                    "primitive_uvs": uv}


def test_hits_cap_gives_a_prefix_and_writes_nothing_beyond(gpu):
    v, t, rays = ac.case("sun")
    full = oracle.list_intersections(v, t, rays)
    total = len(full["ray_ids"])
    assert 900 < total < 1100
    for cap in (0, 1, total - 1, total, total + 7):
        code, n_hits, out = _call(gpu, v, t, rays, cap)
        assert code == 0 and n_hits == total, cap
        assert np.array_equal(out["counts"], full["counts"]), cap
        n = min(cap, total)
        for k in ac.KEYS[1:]:
            assert np.array_equal(out[k][:n], full[k][:n]), (cap, k)
            sentinel = SENTINEL_F32 if out[k].dtype == np.float32 else SENTINEL_U32
            assert len(out[k]) == cap + 16 and (out[k][n:] == sentinel).all(), (cap, k)


def test_cabi_argument_errors(gpu):
    v, t, rays = ac.case("sun")
    code, _, _ = _call(gpu, v, t, rays, 8, null_records=True)
    assert code == -1                                                 # PYQSM_EINVAL
    assert b"hits_cap" in _lib.load().pyqsm_last_error()
    # T = 0 through the C-ABI: complete (zero) counts, n_hits 0, no record touched
    code, n_hits, out = _call(gpu, v, t[:0], rays, 8)
    assert code == 0 and n_hits == 0 and not out["counts"].any()
    assert (out["ray_ids"] == SENTINEL_U32).all() and (out["t_hit"] == SENTINEL_F32).all()
    with pytest.raises(_lib.PyQSMHipError):
        hip.list_intersections(np.zeros((3, 3), np.float32), np.array([[0, 1, 7]], np.int32),
                               np.zeros((4, 6), np.float32), device=gpu)
    with pytest.raises(_lib.PyQSMHipError):
        hip.list_intersections(np.zeros((3, 3), np.float32), np.array([[0, -1, 2]], np.int32),
                               np.zeros((4, 6), np.float32), device=gpu)
    # the library is usable after the refusals
    _same(hip.list_intersections(v, t, rays[:100], device=gpu), oracle.list_intersections(v, t, rays[:100]), "after")


# ------------------------------------------------------------------ list against closest hit

def _list_in_slices(v, t, rays, gpu):
    """list_intersections over slices of at most MAX_RAYS rays, joined (ray ids shifted back)."""
    parts = []
    for b in range(0, len(rays), MAX_RAYS):
        p = hip.list_intersections(v, t, rays[b:b + MAX_RAYS], device=gpu)
        p["ray_ids"] = p["ray_ids"] + np.uint32(b)
        parts.append(p)
    return {k: np.concatenate([p[k] for p in parts]) for k in ac.KEYS}


def _closest_from_list(lst, R):
    """(t, prim, uv) of the closest record per ray: smallest t, then smallest triangle id."""
    t = np.full(R, np.inf, np.float32)
    prim = np.full(R, 0xFFFFFFFF, np.uint32)
    uv = np.zeros((R, 2), np.float32)
    begin, _ = ac.split_by_ray(lst)
    some = np.flatnonzero(lst["counts"])
    tmin = np.minimum.reduceat(lst["t_hit"], begin[some])
    at_min = lst["t_hit"] == np.repeat(tmin, lst["counts"][some])
    idx = np.where(at_min, np.arange(len(at_min)), len(at_min))
    first = np.minimum.reduceat(idx, begin[some])                     # records ascend in triangle id
    t[some], prim[some], uv[some] = tmin, lst["primitive_ids"][first], lst["primitive_uvs"][first]
    return t, prim, uv


@pytest.fixture(scope="module")
def big_canopy():
    v, t = synth.canopy_mesh(3000, seed=9, side=0.6)
    for a in (v, t):
        a.setflags(write=False)
    return v, t


@pytest.mark.parametrize("family", ["sun", "pinhole", "general"])
def test_list_agrees_with_closest_hit_on_every_ray(gpu, big_canopy, family):
    """hip.cast_rays takes the parallel culled sweep (sun), the image-space culled sweep (pinhole)
    and k_cast_rays (general); the list is the same brute-force kernel for all three."""
    v, t = big_canopy
    if family == "sun":
        rays = synth.sun_rays(v, 4000)
    elif family == "pinhole":
        c = v.mean(0)
        rays = rc.create_rays_pinhole(90.0, c, (c[0], c[1], c[2] + 10), (0, 1, -1), 96, 64).reshape(-1, 6)
    else:
        rays = ac.general_rays(v, 4000, seed=21)
    lst = _list_in_slices(v, t, rays, gpu)
    assert ac.structure_violations(lst, len(rays), len(t)) == []
    th, prim, uv = hip.cast_rays(v, t, rays, device=gpu)
    want_t, want_prim, want_uv = _closest_from_list(lst, len(rays))
    assert np.array_equal(np.isinf(th), lst["counts"] == 0)
    assert np.array_equal(th, want_t) and np.array_equal(prim, want_prim)
    assert np.array_equal(uv.view(np.uint32), want_uv.view(np.uint32))
    assert 0.2 * len(rays) < (lst["counts"] > 0).sum() and (lst["counts"] >= 2).sum() > 100


# ------------------------------------------------------------------ non-finite and zero rays

def test_zero_and_non_finite_rays_count_nothing_and_disturb_nothing(gpu):
    v, t, rays = ac.case("sun")
    ref = oracle.list_intersections(v, t, rays)
    begin, end = ac.split_by_ray(ref)
    hitting = np.flatnonzero(ref["counts"])
    bad_at = np.concatenate([hitting[[0, 1, 2, 3]], hitting[[-1, -2]], [0, 255, 256, 1023, 1024, 2048]])
    bad_at = np.unique(bad_at)
    kinds = [lambda r: r[3:].__setitem__(slice(None), 0.0),           # zero direction
             lambda r: r.__setitem__(4, np.nan), lambda r: r.__setitem__(0, np.nan),
             lambda r: r.__setitem__(1, np.inf), lambda r: r.__setitem__(2, -np.inf),
             lambda r: r[:3].__setitem__(slice(None), np.inf)]
    mixed = rays.copy()
    for k, i in enumerate(bad_at):
        kinds[k % len(kinds)](mixed[i])
    got = hip.list_intersections(v, t, mixed, device=gpu)
    assert not got["counts"][bad_at].any()
    keep = np.ones(len(rays), bool)
    keep[bad_at] = False
    assert np.array_equal(got["counts"][keep], ref["counts"][keep])
    assert ac.structure_violations(got, len(rays), len(t)) == []
    sel = np.concatenate([np.arange(b, e) for b, e in zip(begin[keep], end[keep])])
    assert len(sel) == len(got["ray_ids"])
    for k in ac.KEYS[1:]:
        assert np.array_equal(got[k], ref[k][sel]), k
    _same(got, oracle.list_intersections(v, t, mixed), "mixed, mirror")


# ------------------------------------------------------------------ wrappers

def test_count_intersections_keeps_the_image_shape(gpu):
    v, t = synth.canopy_mesh(300, seed=5, side=0.6)
    rays = synth.sun_rays(v, 33 * 47).reshape(33, 47, 6)
    scene = rc.RaycastingScene(gpu)
    scene.add_triangles((v, t))
    counts = scene.count_intersections(rays)
    flat = scene.count_intersections(rays.reshape(-1, 6))
    assert counts.shape == (33, 47) and flat.shape == (33 * 47,) and counts.dtype == np.int32
    assert np.array_equal(counts.reshape(-1), flat) and flat.max() >= 2
    assert np.array_equal(flat, oracle.list_intersections(v, t, rays)["counts"])
    assert np.array_equal(flat, scene.list_intersections(rays.reshape(-1, 6))["counts"])


@pytest.mark.parametrize("which", ["box", "canopy"])
def test_sparse_cast_points_lie_on_their_rays(gpu, which):
    """sparse_cast_w_intersections locates every crossing from its barycentric weights; the same
    crossing located along the ray (origin + t * direction) must coincide."""
    v, t = (mc.CUBE_V, mc.CUBE_T) if which == "box" else synth.canopy_mesh(400, seed=6, side=0.8)
    num = 10 if which == "box" else 40
    seg, pcd = rc.sparse_cast_w_intersections((v, t), num=num, device=gpu)
    assert seg.shape == (num * num, 2, 3)
    rays = np.concatenate([seg[:, 0], seg[:, 1] - seg[:, 0]], axis=-1).astype(np.float32)
    lst = hip.list_intersections(v, t, rays, device=gpu)
    _same(lst, oracle.list_intersections(v, t, rays), which)
    assert len(pcd.points) == lst["counts"].sum() == len(lst["ray_ids"]) > 50
    r = rays[lst["ray_ids"].astype(np.int64)].astype(np.float64)
    along = r[:, :3] + lst["t_hit"].astype(np.float64)[:, None] * r[:, 3:]
    dist = lst["t_hit"].astype(np.float64) * np.linalg.norm(r[:, 3:], axis=1)
    err = np.linalg.norm(pcd.points - along, axis=1) / dist
    print(f"{which}: {len(err)} crossings, max |point - (o + t d)| / distance = {err.max():.3g}")
    assert err.max() <= ac.UV_POINT_RTOL
    if which == "box":
        x, y = rays[:, 0], rays[:, 1]
        clear = (x > 0) & (x < 1) & (y > 0) & (y < 1) & (x != y)       # off the edges and the face diagonal
        assert clear.sum() == 56 and (lst["counts"][clear] == 2).all()
