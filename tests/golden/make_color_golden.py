"""Writes tests/golden/color_hsv.npz: about 3 000 colours and matplotlib's own rgb_to_hsv / hsv_to_rgb
outputs for them (matplotlib 3.10.8 when this was run), the bits the colour contract is pinned to.

    rgb       uniform colours, 8-bit colours, the 4-level grid (every tie between channels), near-grey
              colours at 1e-9 spread, and the hue-wrap and extreme rows of tests/color_restatement.py
    hsv       matplotlib.colors.rgb_to_hsv(rgb)
    rgb_back  matplotlib.colors.hsv_to_rgb(hsv)

    python tests/golden/make_color_golden.py
"""
import os
import sys

import numpy as np
from matplotlib.colors import hsv_to_rgb, rgb_to_hsv

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.color_restatement import EXTREME_ROWS  # noqa: E402


def colours():
    rng = np.random.default_rng(2025)
    levels = np.arange(4) / 3.0
    grid = np.stack(np.meshgrid(levels, levels, levels, indexing="ij"), axis=-1).reshape(-1, 3)
    grey = np.clip(rng.random((500, 1)) + 1e-9 * rng.standard_normal((500, 3)), 0, 1)
    return np.concatenate([rng.random((1200, 3)), rng.integers(0, 256, (1200, 3)) / 255.0, grid, grey, EXTREME_ROWS])


if __name__ == "__main__":
    rgb = colours()
    hsv = rgb_to_hsv(rgb)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "color_hsv.npz")
    np.savez_compressed(out, rgb=rgb, hsv=hsv, rgb_back=hsv_to_rgb(hsv))
    print(out, len(rgb), "colours,", os.path.getsize(out), "bytes")
