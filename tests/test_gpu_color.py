"""The colour path on the GPU (csrc/color.hip, viz/color.py): every output is array_equal to the
NumPy restatement (tests/color_restatement.py, pinned to matplotlib's bits by tests/test_color_host.py) and
to the golden file. No tolerance anywhere."""
import functools
import os

import numpy as np
import pytest

from pyqsm_amd import _lib, hip, synth
from pyqsm_amd.geometry.cloud import PointCloud
from pyqsm_amd.viz import color as vc
from tests import color_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "color_hsv.npz"))
ALL_HUES = list(R.COLOR_CONDS)
SHAPES = [(20, 1, 1), (16, 8, 8), (12, 5, 7), (16, 16, 16)]
EDGE_SIZES = [0, 1, 63, 64, 65, 511, 512, 513]            # wave and tile edges of the ballot scan


@functools.lru_cache(maxsize=None)
def base():
    rgb = np.concatenate([R.base_set(), R.EXTREME_ROWS])
    rgb.setflags(write=False)
    return rgb


@functools.lru_cache(maxsize=None)
def expected(hues=R.DEFAULT_HUES, min_s=.2, lift_div=3.0):
    rules, closed = R.rules_of(hues)
    return R.segment(base(), rules, closed, min_s, lift_div)


def sixteen_rules():
    """K = 16: the seven of the table, then nine bands with every closed pattern on h, s and v."""
    rules, closed = R.rules_of(ALL_HUES)
    extra = np.array([(k / 9, (k + 1) / 9, .1 * (k % 3), 1.0, .05 * k, 1.0) for k in range(9)])
    return np.concatenate([rules, extra]), np.concatenate([closed, np.arange(9, dtype=np.int32) * 7 % 64])


def same(got, want):
    """cls, counts, members, corrected rgb, hsv2: all five, bit for bit."""
    cls, counts, members, rgb, hsv = want
    return (got.cls.dtype == np.uint8 and np.array_equal(got.cls, cls) and np.array_equal(got.counts, counts)
            and np.array_equal(got.members, members) and np.array_equal(got.rgb, rgb) and np.array_equal(got.hsv, hsv))


def test_restatement_counts_of_the_base_set():
    """Before anything else: no class is silently empty, and the empty-class path is exercised."""
    six = R.segment(R.base_set(), *R.rules_of(R.DEFAULT_HUES))[1]
    assert six[[5, 0, 1, 2, 3, 4]].tolist() == [202, 1655, 660, 1022, 1367, 1094]   # none white blues pink r_y greens
    seven = R.segment(R.base_set(), *R.rules_of(ALL_HUES))[1]
    assert seven[ALL_HUES.index("subblue")] == 0 and seven[ALL_HUES.index("light_greens")] == 0
    assert (np.delete(seven, [3, 5]) > 0).all()


def test_conversions_equal_restatement_and_golden(gpu):
    rgb = base()
    hsv = hip.rgb_to_hsv(rgb)
    assert np.array_equal(hsv, R.rgb_to_hsv(rgb)) and (hsv[6000:6003, 0] == 1.0).all()
    assert np.array_equal(hip.hsv_to_rgb(hsv), R.hsv_to_rgb(hsv))
    assert np.array_equal(hip.rgb_to_hsv(GOLDEN["rgb"]), GOLDEN["hsv"])
    assert np.array_equal(hip.hsv_to_rgb(GOLDEN["hsv"]), GOLDEN["rgb_back"])
    assert np.array_equal(vc.rgb_to_hsv(rgb), hsv) and np.array_equal(vc.hsv_to_rgb(hsv), R.hsv_to_rgb(hsv))


@pytest.mark.parametrize("hues", [R.DEFAULT_HUES, tuple(ALL_HUES)], ids=["five", "seven"])
def test_segment_equals_restatement(gpu, hues):
    rules, closed = R.rules_of(hues)
    got = hip.hsv_segment(base(), rules, closed)
    assert same(got, expected(hues))
    assert got.counts.sum() == len(base())
    if len(hues) == 7:
        assert got.counts[3] == 0 and got.counts[5] == 0
    bare = hip.hsv_segment(base(), rules, closed, members=False, corrected=False, hsv=False)
    assert bare.members is None and bare.rgb is None and np.array_equal(bare.cls, got.cls)
    assert np.array_equal(bare.counts, got.counts)


def test_segment_equals_golden(gpu):
    """The corrected colours without a lift are matplotlib's own round trip of the golden colours."""
    rules, closed = R.rules_of(R.DEFAULT_HUES)
    got = hip.hsv_segment(GOLDEN["rgb"], rules, closed, min_s=0.0)
    assert np.array_equal(got.rgb, GOLDEN["rgb_back"])
    assert same(got, R.segment(GOLDEN["rgb"], rules, closed, min_s=0.0))


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_wave_and_tile_edges(gpu, n):
    rgb = base()[5990 - n:5990]
    for rules, closed in (R.rules_of(R.DEFAULT_HUES), R.rules_of(()), sixteen_rules()):
        assert len(rules) in (5, 0, 16)
        got = hip.hsv_segment(rgb, rules, closed)
        assert same(got, R.segment(rgb, rules, closed)), len(rules)
        if len(rules) == 0:
            assert got.counts.tolist() == [n] and (got.cls == 255).all()
            assert np.array_equal(got.members, np.arange(n))


def test_sixteen_rules_on_the_base_set(gpu):
    rules, closed = sixteen_rules()
    want = R.segment(base(), rules, closed)
    assert (want[1][7:16] > 0).sum() >= 5                   # the bands behind the table still catch rows
    assert same(hip.hsv_segment(base(), rules, closed), want)


def test_lift_divisors(gpu):
    rgb = base()
    rules, closed = R.rules_of(R.DEFAULT_HUES)
    ident = hip.hsv_segment(rgb, rules, closed, lift_div=np.inf)
    assert np.array_equal(ident.rgb, rgb)                   # bitwise unchanged: no lift, no round trip
    assert np.array_equal(ident.hsv, R.rgb_to_hsv(rgb)) and same(ident, R.segment(rgb, rules, closed, lift_div=np.inf))
    one = hip.hsv_segment(rgb, rules, closed, lift_div=1.0)
    assert same(one, R.segment(rgb, rules, closed, lift_div=1.0))
    assert not np.array_equal(one.rgb, expected()[3])
    other = hip.hsv_segment(rgb, rules, closed, min_s=.5, lift_div=2.0)
    assert same(other, R.segment(rgb, rules, closed, .5, 2.0))


def test_refusals(gpu):
    rgb = np.array(base()[:100])
    rules, closed = R.rules_of(R.DEFAULT_HUES)
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.hsv_segment(rgb, rules, closed, lift_div=0.5)
    assert e.value.code == -1
    bad_rule = rules.copy()
    bad_rule[1, 0] = np.nan
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.hsv_segment(rgb, bad_rule, closed)
    assert e.value.code == -1
    for value in (1.0000001, np.nan):
        bad = rgb.copy()
        bad[77, 2] = value
        hip.prof_enable(True)
        hip.prof_reset()
        try:
            for call in (lambda c: hip.hsv_segment(c, rules, closed), hip.rgb_to_hsv, hip.hsv_histogram,
                         hip.color_mask):
                with pytest.raises(ValueError):
                    call(bad)
            launched = [hip.prof_get(k)[1] for k in ("hsv_segment", "pyqsm_rgb_to_hsv", "hsv_hist", "color_flags")]
        finally:
            hip.prof_enable(False)
        assert launched == [0, 0, 0, 0]                     # refused before any launch
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.hsv_histogram(rgb, (4097, 1, 1))
    assert e.value.code == -4


@pytest.mark.parametrize("bins", SHAPES)
def test_histograms(gpu, bins):
    rgb = base()
    hsv = R.rgb_to_hsv(rgb)
    want = R.histogram(hsv, bins)
    got = hip.hsv_histogram(rgb, bins)
    assert got.dtype == np.int64 and got.shape == bins and np.array_equal(got, want) and got.sum() == len(rgb)
    assert np.array_equal(got, np.histogramdd(hsv, bins, range=[(0, 1)] * 3)[0])
    assert np.array_equal(hip.hsv_histogram(hsv, bins, is_hsv=True), want)
    # values on every edge and one ulp to either side
    rng = np.random.default_rng(3)
    edges = R.edge_values(bins)
    on_edges = np.concatenate([rng.choice(edges, (4000, 3)), np.stack([edges] * 3, axis=1)])
    assert np.array_equal(hip.hsv_histogram(on_edges, bins, is_hsv=True),
                          np.histogramdd(on_edges, bins, range=[(0, 1)] * 3)[0])
    # per class
    cls = expected()[0]
    seg = vc.hue_segments(rgb)
    for which in (0, 3, 255):
        assert np.array_equal(hip.hsv_histogram(rgb, bins, cls=cls, which=which), R.histogram(hsv, bins, cls, which))
    assert np.array_equal(vc.hsv_histogram(rgb, bins, labels=seg.labels, which=3), R.histogram(hsv, bins, cls, 3))
    assert np.array_equal(vc.hsv_histogram(rgb, bins, labels=seg.labels, which=-1), R.histogram(hsv, bins, cls, 255))
    assert np.array_equal(vc.hsv_histogram(rgb, bins), want)


def test_masks(gpu):
    rgb = np.array(base())
    rgb[400:440, 2] = 0.0                                   # b == 0: r / b is inf or NaN, the row is false
    rgb[440:450] = [0.0, 0.5, 0.0]                          # 0 / 0
    rgb[450:460] = [0.3, 0.5, 0.0]
    assert len(R.mask_green(rgb)) > 100 and len(R.mask_sum_gt(rgb)) > 100
    assert np.array_equal(hip.color_mask(rgb, "green"), R.mask_green(rgb))
    assert not np.intersect1d(hip.color_mask(rgb, "green"), np.arange(400, 460)).size
    assert np.array_equal(hip.color_mask(rgb, "sum_gt", 2.7), R.mask_sum_gt(rgb, 2.7))
    assert np.array_equal(hip.color_mask(rgb, "sum_gt", 1.5), R.mask_sum_gt(rgb, 1.5))
    assert hip.color_mask(rgb, "sum_gt", 3.0).shape == (0,)
    for n in (1, 255, 256, 257):
        assert np.array_equal(hip.color_mask(rgb[:n], "sum_gt", 2.7), R.mask_sum_gt(rgb[:n], 2.7))


def test_dev_form_equals_host_form(gpu):
    rgb = base()
    n = len(rgb)
    rules, closed = R.rules_of(R.DEFAULT_HUES)
    d_rgb = hip.DeviceBuffer.from_array(rgb)
    d_cls, d_mem = hip.DeviceBuffer(n), hip.DeviceBuffer(8 * n)
    d_out, d_hsv = hip.DeviceBuffer(24 * n), hip.DeviceBuffer(24 * n)
    try:
        counts = hip.hsv_segment_dev(d_rgb.ptr, n, rules, closed, d_cls.ptr, members_ptr=d_mem.ptr,
                                     rgb_out_ptr=d_out.ptr, hsv_out_ptr=d_hsv.ptr)
        got = hip.HsvSegment(d_cls.download((n,), np.uint8), counts, d_mem.download((n,), np.int64),
                             d_out.download((n, 3), np.float64), d_hsv.download((n, 3), np.float64))
        assert same(got, expected())
        counts_only = hip.hsv_segment_dev(d_rgb.ptr, n, rules, closed, d_cls.ptr)
        assert np.array_equal(counts_only, counts)
        bad = np.array(rgb)
        bad[4321, 0] = np.nan
        d_rgb.upload(bad)
        with pytest.raises(ValueError):                     # the kernel's error word
            hip.hsv_segment_dev(d_rgb.ptr, n, rules, closed, d_cls.ptr)
    finally:
        for b in (d_rgb, d_cls, d_mem, d_out, d_hsv):
            b.free()


def test_two_runs_give_the_same_bytes(gpu):
    rules, closed = R.rules_of(ALL_HUES)
    a, b = (hip.hsv_segment(base(), rules, closed) for _ in range(2))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    h = [hip.hsv_histogram(base(), (16, 16, 16)).tobytes() for _ in range(2)]
    assert h[0] == h[1]


# ---- viz.color on a PointCloud

def cloud():
    n = len(base())
    pts = np.random.default_rng(5).random((n, 3)) * 10.0
    return PointCloud(pts, colors=np.array(base()), normals=np.roll(pts, 1, axis=1))


def same_cloud(pcd, pts, colors):
    return np.array_equal(pcd.points, pts) and np.array_equal(np.asarray(pcd.colors).reshape(-1, 3), colors)


def test_hue_segments(gpu):
    cls, counts, members, corrected, hsv2 = expected()
    seg = vc.hue_segments(base())
    assert seg.labels.dtype == np.int32 and np.array_equal(seg.labels, np.where(cls == 255, -1, cls.astype(np.int32)))
    assert np.array_equal(seg.counts, counts) and np.array_equal(seg.corrected, corrected)
    assert np.array_equal(seg.hsv, hsv2) and len(seg) == 5
    for k in range(5):
        assert np.array_equal(seg.indices(k), np.nonzero(cls == k)[0])
    assert np.array_equal(seg.rest(), np.nonzero(cls == 255)[0])
    lazy = vc.hue_segments(base(), members=False)
    assert np.array_equal(lazy.indices(2), seg.indices(2)) and np.array_equal(lazy.rest(), seg.rest())
    custom = vc.hue_segments(base(), ["pink", ((.1, .3, .2, 1.0, 0, 1.0), 0b001010)])
    rules = np.array([R.COLOR_CONDS["pink"][0], (.1, .3, .2, 1.0, 0, 1.0)])
    assert np.array_equal(custom.counts, R.segment(base(), rules, np.array([1, 0b001010], np.int32))[1])


def test_segment_hues_on_a_cloud(gpu):
    pcd = cloud()
    pts, normals = pcd.points.copy(), pcd.normals.copy()
    for hues in (R.DEFAULT_HUES, ("white", "subblue", "greens", "light_greens", "pink")):
        pcd.colors = np.array(base())
        cls, counts, _, corrected, _ = expected(tuple(hues))
        labels = np.where(cls == 255, -1, cls.astype(np.int32))
        want_hue, want_rest = R.segment_hues_layout(pts, labels, corrected, len(hues))
        hue_pcds, no_hue_pcds = vc.segment_hues(pcd, seed="t", hues=list(hues), draw_gif=False)
        assert len(hue_pcds) == len(no_hue_pcds) == len(want_hue) == 1 + int((counts[:-1] > 0).sum())
        assert hue_pcds[0] is pcd and same_cloud(pcd, pts, corrected)
        for got, (p, c) in zip(hue_pcds + no_hue_pcds, want_hue + want_rest):
            assert same_cloud(got, p, c)
        assert np.array_equal(hue_pcds[1].normals, normals[labels == 0])
    assert len(hue_pcds) == 4                               # subblue and light_greens left no entry


def test_get_color_by_hue_saturate_and_green(gpu):
    pcd = cloud()
    rgb = base()
    hsv = R.rgb_to_hsv(rgb)
    for cond, (bounds, closed) in (("pink", R.COLOR_CONDS["pink"]), ((0, .5, .5, 1, .2, 1), ((0, .5, .5, 1, .2, 1), 0))):
        idx = np.nonzero(R.holds(hsv, bounds, closed))[0]
        hue, no_hue, got = vc.get_color_by_hue(pcd, cond)
        assert np.array_equal(got, idx) and same_cloud(hue, pcd.points[idx], rgb[idx])
        assert same_cloud(no_hue, np.delete(pcd.points, idx, 0), np.delete(rgb, idx, 0))
    idx = np.nonzero(R.holds(hsv, *R.COLOR_CONDS["greens"]))[0]
    assert np.array_equal(vc.get_color_by_hue(pcd, lambda t: t[0] <= .5 and t[0] > 2 / 9 and t[2] > .2)[2], idx)
    hue, no_hue, got = vc.get_color_by_hue(pcd, "subblue")
    assert len(hue) == 0 and len(got) == 0 and len(no_hue) == len(rgb)
    green = R.mask_green(rgb)
    assert same_cloud(vc.get_green_surfaces(pcd), pcd.points[green], rgb[green])
    assert same_cloud(vc.get_green_surfaces(pcd, invert=True), np.delete(pcd.points, green, 0), np.delete(rgb, green, 0))
    white = R.mask_sum_gt(rgb)
    assert same_cloud(vc.remove_color_pts(pcd, invert=True), np.delete(pcd.points, white, 0), np.delete(rgb, white, 0))
    assert same_cloud(vc.remove_color_pts(pcd, lambda c: sum(c) > 2.7), pcd.points[white], rgb[white])
    corrected, hsv_fulls = vc.color_distribution(rgb, rgb[:100], cutoff=.01)
    assert np.array_equal(corrected, expected()[3][:100]) and len(hsv_fulls) == 2
    assert np.array_equal(hsv_fulls[0], hsv) and np.array_equal(hsv_fulls[1], hsv[:100])
    by_func, _ = vc.color_distribution(rgb, sc_func=lambda sc: sc + (1 - sc) / 3)
    assert np.array_equal(by_func, expected()[3])
    out, orig = vc.saturate_colors(pcd)
    assert out is pcd and np.array_equal(orig, rgb) and np.array_equal(pcd.colors, expected()[3])


@functools.lru_cache(maxsize=None)
def bloom_cloud():
    rng = np.random.default_rng(9)
    pts = synth.forest(2000) + rng.random((2000, 3)) * 1e-3       # random coordinates: no distance ties
    col = rng.random((2000, 3)) * .8
    col[rng.choice(2000, 150, replace=False)] = .92 + .08 * rng.random((150, 3))
    return pts[:2000], col


def test_homog_colors(gpu):
    pts, col = bloom_cloud()
    assert len(R.mask_sum_gt(col)) == 150
    pcd = PointCloud(pts.copy(), colors=col.copy())
    assert vc.homog_colors(pcd) is pcd
    want = R.homog_colors(pts, col)
    assert np.array_equal(pcd.colors, want) and len(R.mask_sum_gt(want)) == 0
    assert np.array_equal(np.delete(pcd.colors, R.mask_sum_gt(col), 0), np.delete(col, R.mask_sum_gt(col), 0))
    # fewer than 30 non-white points: k = their count
    few = np.concatenate([np.nonzero(col.sum(axis=1) <= 2.7)[0][:12], R.mask_sum_gt(col)[:40]])
    pcd = PointCloud(pts[few], colors=col[few])
    vc.homog_colors(pcd)
    assert np.array_equal(pcd.colors, R.homog_colors(pts[few], col[few]))
    assert np.abs(pcd.colors[12:] - col[few][:12].mean(axis=0)).max() < 1e-12    # every one the mean of all twelve
    # none: unchanged
    white = R.mask_sum_gt(col)
    pcd = PointCloud(pts[white], colors=col[white].copy())
    vc.homog_colors(pcd)
    assert np.array_equal(pcd.colors, col[white])
    plain = PointCloud(pts[:50], colors=col[:50] * .5)
    vc.homog_colors(plain)
    assert np.array_equal(plain.colors, col[:50] * .5)
