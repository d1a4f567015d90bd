"""pyqsm_alpha_area on the GPU against the CPU statement of its contract (tests/alpha_restatement.py,
itself pinned to scipy's Delaunay triangulation by tests/test_alpha_host.py): twice the area, the
live-point count and the boundary edge list are compared as integers, never within a tolerance."""
import numpy as np
import pytest

from pyqsm_amd import _lib, hip
from pyqsm_amd.geometry.cloud import PointCloud
from pyqsm_amd.viz import projection as pj
from tests import alpha_restatement as R

pytestmark = pytest.mark.gpu


def assert_same(res, s, ref, P, offset=0):
    """Segment s of a hip.AlphaArea against a restatement's (twice_area, boundary) for the points P."""
    assert int(res.twice_area[s]) == ref[0]
    live = len(R.live_points(P))
    assert int(res.n_live[s]) == live
    assert int(res.n_boundary[s]) == len(ref[1])
    assert [(a - offset, b - offset) for a, b in res.boundary(s).tolist()] == ref[1]


def run(P, A2, **kw):
    return hip.alpha_area(P, A2, return_boundary=True, **kw)


@pytest.mark.parametrize("name,k", [(name, k) for name in R.SMALL_GROUPS for k in range(3)])
def test_small_groups(gpu, name, k):
    make, a2s = R.SMALL_GROUPS[name]
    P, A2 = make(), a2s[k]
    res = run(P, A2)
    assert_same(res, 0, R.brute(P, A2), P)
    if name == "cocircular" and k > 0:
        assert res.stats["exact_fallbacks"] > 0      # the ties of the twelve-gon are settled in 128 bits


@pytest.mark.parametrize("move", [(0, 1, 0), (0, -1, 0), (3, 0, 1), (3, 0, -1), (7, -1, 0), (10, 0, 1)])
def test_near_ties_fall_back(gpu, move):
    P = R.cocircular(move)
    for A2 in (65000 ** 2 - 1, 65000 ** 2, 65000 ** 2 + 70000):
        res = run(P, A2)
        assert_same(res, 0, R.brute(P, A2), P)
        assert res.stats["exact_fallbacks"] > 0      # 1 part in 10^5 off a tie: inside the filter's bound


def test_coordinates_at_the_limit(gpu):
    P = R.corners()
    assert P.max() - P.min() > (1 << 20) - 2000
    A2 = 400 ** 2                                    # reaches within a corner only
    ref = R.brute(P, A2)
    assert ref[0] > 0
    assert_same(run(P, A2), 0, ref, P)


def test_inclusive_bound(gpu):
    m, s = 6, 4
    P = R.square_lattice(m, s)
    res = run(P, s * s // 2)
    assert int(res.twice_area[0]) == 2 * ((m - 1) * s) ** 2
    assert_same(res, 0, R.brute(P, s * s // 2), P)
    res = run(P, s * s // 2 - 1)
    assert int(res.twice_area[0]) == 0 and int(res.n_boundary[0]) == 0 and len(res.boundary(0)) == 0


def test_collinear_and_tiny(gpu):
    line = np.stack([np.arange(50) * 3, np.arange(50) * 7], axis=1).astype(np.int32)
    res = run(line, 10 ** 6)
    assert (int(res.twice_area[0]), int(res.n_live[0]), int(res.n_boundary[0])) == (0, 50, 0)
    assert res.stats["tests"] == 0                   # settled on the host
    for n in (0, 1, 2):
        res = run(np.zeros((n, 2), np.int32) + np.arange(n)[:, None].astype(np.int32), 100)
        assert (int(res.twice_area[0]), int(res.n_live[0]), len(res.boundary(0))) == (0, n, 0)
    res = run(np.array([[5, 5], [5, 5]], np.int32), 100)
    assert int(res.n_live[0]) == 1


def test_point_inside_a_hull_edge(gpu):
    """(0,0)-(40,0) carries (10,0) strictly inside: the long edge is killed, the two halves are edges."""
    P = np.array([[0, 0], [40, 0], [10, 0], [20, 30], [18, 11]], np.int32)
    for A2 in (300, 500, 10 ** 4):
        ref = R.brute(P, A2)
        assert_same(run(P, A2), 0, ref, P)
    assert (0, 1) not in R.brute(P, 10 ** 4)[1] and (0, 2) in R.brute(P, 10 ** 4)[1]


def test_tripled_points(gpu):
    P = R.holey_lattice()
    A2 = 50
    rng = np.random.default_rng(4)
    idx = rng.permutation(np.repeat(np.arange(len(P)), 3))
    T = P[idx]
    res, single = run(T, A2), run(P, A2)
    assert int(res.twice_area[0]) == int(single.twice_area[0]) == R.brute(P, A2)[0]
    assert int(res.n_live[0]) == int(single.n_live[0])
    assert res.stats["merged_duplicates"] == 2 * len(R.live_points(P)) + (len(P) - len(R.live_points(P))) * 3
    assert_same(res, 0, R.brute(T, A2), T)           # boundary indices name the lowest copy
    lowest = {}
    for i, (x, y) in enumerate(T.tolist()):
        lowest.setdefault((x, y), i)
    assert all(lowest[tuple(T[v])] == v for v in res.boundary(0).ravel().tolist())


def test_big_cloud(gpu):
    P, A2 = R.big_cloud(), R.big_cloud_a2()
    res = run(P, A2)
    assert_same(res, 0, R.local(P, A2), P)
    assert res.stats["tests"] <= res.stats["estimated_tests"]


def test_dense_cell_chunks_and_slices(gpu):
    """One cell of 2300 points: its stencil is staged in two chunks and served by 72 blocks."""
    P, A2 = R.dense_cloud(), 150 ** 2
    res = run(P, A2)
    assert res.stats["estimated_tests"] == len(P) ** 3          # one cell holds everything
    assert_same(res, 0, R.delaunay_filtered(P, A2), P)
    two = run(np.concatenate([P, P + 7]), A2, seg_start=[0, len(P), 2 * len(P)])
    assert int(two.twice_area[0]) == int(two.twice_area[1]) == int(res.twice_area[0])


def test_boundary_of_2049_edges(gpu):
    """683 small triangles far apart, points shuffled: 2049 boundary edges, one radix tile of 2048 and one
    row, in the two sort passes by (a, b) over ids of two 8-bit digits. Ids of one digit with many edges
    are test_small_groups, far larger lists test_big_cloud; a boundary has at least three edges, so the
    one-row list does not exist here."""
    rng = np.random.default_rng(12)
    k = np.arange(683)
    at = np.stack([k % 27, k // 27], axis=1) * 1000 + rng.integers(0, 200, (683, 2))
    legs = rng.integers(20, 31, (683, 2))                        # right triangles: R^2 <= (30^2 + 30^2) / 4 = 450
    zero = np.zeros(683, np.int64)
    tri = at[:, None, :] + np.stack([np.stack([zero, zero], 1), np.stack([legs[:, 0], zero], 1),
                                     np.stack([zero, legs[:, 1]], 1)], axis=1)
    P = tri.reshape(-1, 2)[rng.permutation(3 * 683)].astype(np.int32)
    A2 = 500
    ref = R.delaunay_filtered(P, A2)
    assert len(ref[1]) == 2049 and ref[0] == int((legs[:, 0] * legs[:, 1]).sum())
    assert_same(run(P, A2), 0, ref, P)


@pytest.fixture(scope="module")
def batch():
    rnd, lat = R.random_points(), R.holey_lattice()
    line = np.stack([np.arange(30) * 5, np.arange(30) * 2 + 7], axis=1).astype(np.int32)
    parts = [rnd, lat, rnd.copy(), np.zeros((0, 2), np.int32), line, R.square_lattice(5, 6) + 100, R.annulus()]
    return parts, 100


def test_batch_of_seven(gpu, batch):
    parts, A2 = batch
    seg = np.concatenate([[0], np.cumsum([len(p) for p in parts])])
    res = run(np.concatenate(parts), A2, seg_start=seg)
    for s, P in enumerate(parts):
        one = run(P, A2)
        assert int(res.twice_area[s]) == int(one.twice_area[0])
        assert int(res.n_live[s]) == int(one.n_live[0]) and int(res.n_boundary[s]) == int(one.n_boundary[0])
        assert np.array_equal(res.boundary(s) - seg[s], one.boundary(0))
        assert_same(res, s, R.brute(P, A2) if len(P) < 200 else R.local(P, A2), P, offset=int(seg[s]))
    assert int(res.twice_area[0]) == int(res.twice_area[2]) > 0          # the same cloud twice
    assert int(res.twice_area[3]) == 0 and int(res.twice_area[4]) == 0


def test_reproducible_and_permutation_invariant(gpu):
    P, A2 = R.random_points(n=600, size=300, seed=9), 150
    a, b = run(P, A2), run(P, A2)
    assert np.array_equal(a.twice_area, b.twice_area) and np.array_equal(a.edges, b.edges)
    assert np.array_equal(a.n_live, b.n_live) and np.array_equal(a.n_boundary, b.n_boundary)
    keep = R.live_points(P)                         # without duplicates the index map is one to one
    Q = P[keep]
    perm = np.random.default_rng(1).permutation(len(Q))
    base, shuffled = run(Q, A2), run(Q[perm], A2)
    assert int(base.twice_area[0]) == int(shuffled.twice_area[0]) == R.local(Q, A2)[0]
    back = sorted(map(tuple, perm[shuffled.boundary(0)].tolist()))
    assert back == list(map(tuple, base.boundary(0).tolist()))


def test_annulus_has_two_loops(gpu):
    P, A2 = R.annulus(), 18
    res = run(P, A2)
    ref = R.local(P, A2)
    assert_same(res, 0, ref, P)
    lp = R.loops(list(map(tuple, res.boundary(0).tolist())))
    assert len(lp) == 2
    signed = []
    for loop in lp:
        xy = P[loop].astype(np.int64)
        nx = np.roll(xy, -1, axis=0)
        signed.append(int((xy[:, 0] * nx[:, 1] - xy[:, 1] * nx[:, 0]).sum()))
    assert min(signed) < 0 < max(signed)             # the outer loop counter-clockwise, the hole clockwise
    assert sum(signed) == ref[0]


def test_work_cap(gpu):
    P, A2 = R.big_cloud(), R.big_cloud_a2()
    est = run(P, A2).stats["estimated_tests"]
    with pytest.raises(_lib.PyQSMHipError) as e:
        run(P, A2, max_tests=est - 1)
    assert str(est) in str(e.value) and str(est - 1) in str(e.value)
    small = R.random_points()
    assert_same(run(small, 900, max_tests=est - 1), 0, R.brute(small, 900), small)   # the context is fine
    assert int(run(P, A2, max_tests=est).twice_area[0]) == R.local(P, A2)[0]          # the cap is inclusive


def test_bounds_are_refused(gpu):
    P = R.random_points()
    with pytest.raises(_lib.PyQSMHipError) as e:
        run(P, (1 << 40) + 1)
    assert e.value.code == -1
    wide = np.array([[0, 0], [(1 << 20) + 1, 5], [7, 9]], np.int32)
    with pytest.raises(_lib.PyQSMHipError) as e:
        run(wide, 100)
    assert e.value.code == -1
    ok = np.array([[0, 0], [1 << 20, 5], [7, 1 << 20]], np.int32) - (1 << 19)
    assert int(run(ok, 1 << 40).twice_area[0]) == R.brute(ok, 1 << 40)[0]


# ---------------------------------------------------------------- wrappers

def test_projected_area_is_the_kernel_scaled(gpu):
    rng = np.random.default_rng(6)
    pts = rng.random((500, 3)) * [4.0, 3.0, 9.0] + [10.0, -20.0, 0.0]
    alpha = 0.4
    ij, q = pj.quantize_plane(pts)
    A2 = pj.lattice_a2(alpha, q)
    shape = pj.projected_area(pts, alpha, return_boundary=True)
    raw = hip.alpha_area(ij, A2, return_boundary=True)
    assert shape.quantum == q and shape.twice_area_q == int(raw.twice_area[0]) > 0
    assert shape.area == shape.twice_area_q * q * q / 2 and shape.n_points == int(raw.n_live[0])
    assert np.array_equal(shape.boundary, raw.boundary(0))
    d = (ij[shape.boundary[:, 1]] - ij[shape.boundary[:, 0]]).astype(np.float64)
    assert shape.perimeter == pytest.approx(np.hypot(d[:, 0], d[:, 1]).sum() * q, rel=1e-12)
    assert shape.twice_area_q == R.local(ij, A2)[0]


def test_grid_area_is_exact(gpu):
    m, h = 9, 0.25
    g = np.arange(m) * h
    pts = np.stack([*np.meshgrid(g, g, indexing="ij"), np.zeros((m, m))], axis=-1).reshape(-1, 3)
    r = h / np.sqrt(2.0)
    assert pj.projected_area(pts, r * (1 + 1e-6)).area == ((m - 1) * h) ** 2
    assert pj.projected_area(pts, r * (1 - 1e-6)).area == 0.0


def test_tilted_plane(gpu):
    rng = np.random.default_rng(8)
    pts = rng.random((300, 3)) * 5
    normal, alpha = (1.0, -2.0, 3.0), 0.6
    ij, q = pj.quantize_plane(pts, normal=normal)
    shape = pj.projected_area(pts, alpha, normal=normal)
    assert shape.quantum == q
    assert shape.twice_area_q == R.local(ij, pj.lattice_a2(alpha, q))[0] > 0


def test_project_pcd_signature(gpu):
    pts = np.random.default_rng(10).random((400, 3)) * 2
    a = pj.project_pcd(pts=pts, alpha=.2, plot=False, name="x", seed=3, off_screen=True)
    b = pj.project_pcd(point_cloud=PointCloud(pts), alpha=.2)
    assert a.area == b.area > 0 and a.twice_area_q == b.twice_area_q


def test_project_in_slices(gpu):
    rng = np.random.default_rng(12)
    pts = rng.random((6000, 3)) * [3.0, 3.0, 10.0]
    alpha = 0.5
    m = pj.project_in_slices(PointCloud(pts), seed=0, alpha=alpha)
    names = ["slice_0_20", "slice_20_40", "slice_40_60", "slice_60_80", "slice_80_100"]
    assert list(m) == names + ["total_area"]
    sub = pts[::5]
    z = sub[:, 2]
    edges = np.percentile(z, [0, 20, 40, 60, 80, 100])
    q = m[names[0]]["mesh"].quantum
    total, count = 0.0, 0
    for i, nm in enumerate(names):
        sel = (z >= edges[i]) & ((z < edges[i + 1]) if i < 4 else (z <= edges[i + 1]))
        one = pj.projected_area(sub[sel], alpha, quantum=q)
        assert m[nm]["mesh_area"] == m[nm]["mesh"].area == one.area > 0
        assert m[nm]["mesh"].twice_area_q == one.twice_area_q
        total += one.area
        count += int(sel.sum())
    assert count == len(sub) and m["total_area"] == total


def test_project_by_label(gpu):
    rng = np.random.default_rng(14)
    pts = rng.random((4000, 3)) * 4
    labels = rng.integers(-1, 3, size=4000)
    alpha = 0.5
    out = pj.project_by_label(pts, labels, alpha, every=4)
    assert sorted(out["areas"]) == [0, 1, 2]
    q = out["meshes"][0].quantum
    total = 0.0
    for lab in (0, 1, 2):
        one = pj.projected_area(pts[labels == lab][::4], alpha, quantum=q)
        assert out["areas"][lab] == one.area > 0
        total += one.area
    assert out["total_area"] == total
    shapes = pj.projected_area_batch(pts, labels=labels, alpha=alpha, return_boundary=True)
    assert [s.label for s in shapes] == [0, 1, 2]
    for s in shapes:
        assert (labels[s.boundary.ravel()] == s.label).all()      # indices refer to the points handed in
