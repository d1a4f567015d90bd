"""The colour contract on the CPU (tests/color_restatement.py): the restatement is matplotlib's
bits (the golden file, and matplotlib itself where it imports), the hue wraps to exactly 1.0 and comes
back through case 0, the histogram is np.histogramdd on every edge, segment_hues' lists follow from
labels, the device header gives the restatement's bytes as a host program under the sanitizers, and the
host side of the wrappers (tables, PointCloud colours, drop-in registration) holds without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from pyqsm_amd import _lib, _shadow, hip
from pyqsm_amd.geometry.cloud import PointCloud
from pyqsm_amd.viz import color as vc
from tests import color_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "color_hsv.npz"))
SHAPES = [(20, 1, 1), (16, 8, 8), (12, 5, 7)]


def test_restatement_equals_the_golden_file():
    rgb, hsv, back = GOLDEN["rgb"], GOLDEN["hsv"], GOLDEN["rgb_back"]
    assert 2900 < len(rgb) < 3100 and np.array_equal(rgb[-len(R.EXTREME_ROWS):], R.EXTREME_ROWS)
    assert np.array_equal(R.rgb_to_hsv(rgb), hsv)
    assert np.array_equal(R.hsv_to_rgb(hsv), back)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "color_hsv.npz")) < 300_000


def test_restatement_equals_matplotlib():
    colors = pytest.importorskip("matplotlib.colors")
    rng = np.random.default_rng(11)
    levels = np.arange(4) / 3.0
    grid = np.stack(np.meshgrid(levels, levels, levels, indexing="ij"), axis=-1).reshape(-1, 3)
    grey = np.clip(rng.random((20000, 1)) + 1e-9 * rng.standard_normal((20000, 3)), 0, 1)
    rgb = np.concatenate([rng.random((200000, 3)), rng.integers(0, 256, (200000, 3)) / 255.0, grid, grey,
                          R.EXTREME_ROWS, R.base_set()])
    hsv = colors.rgb_to_hsv(rgb)
    assert np.array_equal(R.rgb_to_hsv(rgb), hsv)
    assert np.array_equal(R.hsv_to_rgb(hsv), colors.hsv_to_rgb(hsv))
    lifted = np.stack([hsv[:, 0], R.lift(hsv[:, 1]), hsv[:, 2]], axis=1)
    assert np.array_equal(R.hsv_to_rgb(lifted), colors.hsv_to_rgb(lifted))


def test_hue_wraps_to_one_and_comes_back_through_case_zero():
    hsv = R.rgb_to_hsv(R.EXTREME_ROWS)
    assert (hsv[:3, 0] == 1.0).all()                      # a tiny negative y: y + 1.0 rounds to 1.0
    assert 0.0 < hsv[5, 0] < 1e-15                        # the mirrored row stays at the bottom
    assert np.array_equal(hsv[3], [0, 0, 0]) and np.array_equal(hsv[4], [0, 0, 1])
    assert np.array_equal(hsv[6], [0, 1, 2.0 ** -1074])
    one = np.array([[1.0, 0.5, 0.8]])                     # i = 6, 6 % 6 == 0: (v, t, p) with f == 0
    assert np.array_equal(R.hsv_to_rgb(one), R.hsv_to_rgb(np.array([[0.0, 0.5, 0.8]])))
    assert np.array_equal(R.hsv_to_rgb(one), [[0.8, 0.8 * (1.0 - (0.5 * 1.0)), 0.8 * 0.5]])


@pytest.mark.parametrize("bins", SHAPES)
def test_histogram_equals_histogramdd_on_every_edge(bins):
    rng = np.random.default_rng(sum(bins))
    edges = R.edge_values(bins)                           # every edge and one ulp to either side
    hsv = np.concatenate([rng.random((3000, 3)), rng.choice(edges, (6000, 3)),
                          np.stack([edges, edges, edges], axis=1)])
    want = np.histogramdd(hsv, bins, range=[(0, 1)] * 3)[0]
    got = R.histogram(hsv, bins)
    assert got.dtype == np.int64 and got.shape == bins and np.array_equal(got, want) and got.sum() == len(hsv)
    cls = rng.integers(0, 3, len(hsv)).astype(np.uint8)
    assert np.array_equal(R.histogram(hsv, bins, cls, 1), np.histogramdd(hsv[cls == 1], bins, range=[(0, 1)] * 3)[0])


def test_first_match_equals_the_cascade_and_the_counts_of_the_base_set():
    rgb = R.base_set()
    rules, closed = R.rules_of(R.DEFAULT_HUES)
    cls, counts, members, corrected, hsv2 = R.segment(rgb, rules, closed)
    assert np.array_equal(cls, R.cascade(hsv2, rules, closed))
    assert counts.tolist() == [1655, 660, 1022, 1367, 1094, 202]         # white blues pink red_yellow greens none
    assert np.array_equal(np.sort(members), np.arange(len(rgb)))
    all_rules, all_closed = R.rules_of(list(R.COLOR_CONDS))
    c7 = R.segment(rgb, all_rules, all_closed)[1]
    assert c7[3] == 0 and c7[5] == 0 and c7.sum() == len(rgb)            # subblue, light_greens


def test_segment_hues_layout_from_hand_made_labels():
    pts = np.arange(24, dtype=np.float64).reshape(8, 3)
    col = np.linspace(0, 1, 24).reshape(8, 3)
    labels = np.array([2, -1, 0, 2, 4, 0, -1, 2])                        # hues 1 and 3 are empty
    hue, rest = R.segment_hues_layout(pts, labels, col, 5)
    assert len(hue) == len(rest) == 4                                    # the corrected cloud + hues 0, 2, 4
    assert np.array_equal(hue[1][0], pts[[2, 5]]) and np.array_equal(rest[1][0], pts[[0, 1, 3, 4, 6, 7]])
    assert np.array_equal(hue[2][0], pts[[0, 3, 7]]) and np.array_equal(rest[2][0], pts[[1, 4, 6]])
    assert np.array_equal(hue[3][1], col[[4]]) and np.array_equal(rest[3][1], col[[1, 6]])


def test_color_check_hashes_equal_the_restatement():
    """color_exact.hpp as a stand-alone host program under ASan and UBSan (csrc/Makefile: color_check): host
    code only, built and run on the CPU. Its hashes are the restatement's over the same generated rows."""
    if _lib.device_count() > 0:
        pytest.skip("sanitizer runs belong on machines without a GPU")
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "pyqsm_amd", "csrc"), "color_check"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "color_check: ok" in out.stdout
    got = dict(re.findall(r"^(hsv|corrected|class|hist) ([0-9a-f]{16})$", out.stdout, flags=re.M))
    rgb = R.check_inputs()
    assert f"rows {len(rgb)} wraps 3" in out.stdout and len(rgb) == 17 ** 3 + 32768 + 7
    rules, closed = R.rules_of(list(R.COLOR_CONDS))
    cls, _, _, corrected, _ = R.segment(rgb, rules, closed)
    hsv = R.rgb_to_hsv(rgb)
    want = {"hsv": hsv, "corrected": corrected, "class": cls, "hist": R.histogram(hsv, (16, 8, 8))}
    assert got == {k: "%016x" % R.fnv1a(np.ascontiguousarray(v).tobytes()) for k, v in want.items()}


def test_tables_and_constants_agree():
    assert list(vc.COLOR_CONDS) == list(R.COLOR_CONDS) and vc.DEFAULT_HUES == R.DEFAULT_HUES
    for name, (bounds, closed) in R.COLOR_CONDS.items():
        assert vc.COLOR_CONDS[name] == (bounds, closed)
    text = open(os.path.join(ROOT, "include", "pyqsm_hip.h")).read()
    for macro, value in (("PYQSM_COLOR_MAX_RULES", hip.COLOR_MAX_RULES), ("PYQSM_COLOR_MAX_BINS", hip.COLOR_MAX_BINS),
                         ("PYQSM_COLOR_NONE", hip.COLOR_NONE), ("PYQSM_MASK_SUM_GT", hip.COLOR_MASKS["sum_gt"]),
                         ("PYQSM_MASK_GREEN", hip.COLOR_MASKS["green"])):
        assert re.search(rf"#define {macro} {value}\b", text), macro
    rules, closed = vc._rules(["white", (.1, .2, .3, .4, .5, .6), ((0, 1, 0, 1, 0, 1), 63)])
    assert rules.shape == (3, 6) and closed.tolist() == [0, 0, 63] and rules[1].tolist() == [.1, .2, .3, .4, .5, .6]
    with pytest.raises(ValueError):
        vc._rules(["mauve"])
    with pytest.raises(ValueError):
        hip.hsv_segment(np.zeros((4, 3)), np.zeros((17, 6)), np.zeros(17, np.int32))
    with pytest.raises(NotImplementedError):
        vc.color_distribution(np.zeros((4, 3)), space="hsv")


def test_point_cloud_carries_colours():
    pts = np.arange(18, dtype=np.float64).reshape(6, 3)
    col = np.linspace(0, 1, 18).reshape(6, 3)
    pcd = PointCloud(pts, colors=col, normals=pts + 1)
    assert pcd.has_colors() and pcd.has_normals()
    a, b = pcd.select_by_index([4, 1]), pcd.select_by_index([4, 1], invert=True)
    assert np.array_equal(a.points, pts[[4, 1]]) and np.array_equal(a.colors, col[[4, 1]])
    assert np.array_equal(a.normals, pts[[4, 1]] + 1)
    assert np.array_equal(b.points, pts[[0, 2, 3, 5]]) and np.array_equal(b.colors, col[[0, 2, 3, 5]])
    bare = PointCloud(pts)
    assert not bare.has_colors() and bare.select_by_index([0]).colors is None
    short = PointCloud(pts, colors=col[:3])                               # not the cloud's length: not carried
    assert not short.has_colors() and short.select_by_index([0, 1]).colors is None
    assert not PointCloud().has_colors()


def test_viz_color_is_registered_and_falls_through():
    assert "segment_hues" in _shadow.HOT_FUNCTIONS["viz.color"]
    assert "rgb_to_hsv" not in _shadow.HOT_FUNCTIONS["viz.color"]          # matplotlib's own under that name
    for name in _shadow.HOT_FUNCTIONS["viz.color"]:
        assert callable(getattr(vc, name)), name
    from pyqsm_amd.geometry import epiphytes
    assert vc.split_on_percentile is epiphytes.split_on_percentile
    with pytest.raises(AttributeError):
        vc.color_compare                                                   # pyQSM's, when pyQSM is on the path
    src = open(os.path.join(ROOT, "pyqsm_amd", "viz", "color.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(matplotlib|open3d|cv2)\b", src, flags=re.M)


def test_no_rows_touch_no_device():
    """n == 0 is answered on the host: zero counts, empty arrays, also without a GPU."""
    rules, closed = R.rules_of(R.DEFAULT_HUES)
    r = hip.hsv_segment(np.zeros((0, 3)), rules, closed)
    assert r.counts.tolist() == [0] * 6 and r.cls.shape == (0,) and r.members.shape == (0,)
    assert hip.rgb_to_hsv(np.zeros((0, 3))).shape == (0, 3) and hip.hsv_to_rgb(np.zeros((0, 3))).shape == (0, 3)
    assert hip.hsv_histogram(np.zeros((0, 3)), (4, 2, 1)).tolist() == np.zeros((4, 2, 1), int).tolist()
    assert hip.color_mask(np.zeros((0, 3))).shape == (0,)


def test_refusals_come_before_any_device():
    """Bad values and bad arguments are PYQSM_EINVAL / PYQSM_ERANGE from the host checks (no GPU needed)."""
    rules, closed = R.rules_of(R.DEFAULT_HUES)
    good = np.full((5, 3), .5)
    for bad_value in (1.0000001, -1e-9, np.nan):
        bad = good.copy()
        bad[3, 1] = bad_value
        for call in (lambda c: hip.hsv_segment(c, rules, closed), hip.rgb_to_hsv, hip.hsv_to_rgb,
                     hip.hsv_histogram, hip.color_mask):
            with pytest.raises(ValueError):
                call(bad)
    for lift_div in (0.5, np.nan, -np.inf):
        with pytest.raises(_lib.PyQSMHipError) as e:
            hip.hsv_segment(good, rules, closed, lift_div=lift_div)
        assert e.value.code == -1
    nan_rule = rules.copy()
    nan_rule[2, 4] = np.nan
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.hsv_segment(good, nan_rule, closed)
    assert e.value.code == -1
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.hsv_histogram(good, (4097, 1, 1))
    assert e.value.code == -4
    with pytest.raises(_lib.PyQSMHipError) as e:
        hip.hsv_histogram(good, (17, 16, 16))
    assert e.value.code == -4
