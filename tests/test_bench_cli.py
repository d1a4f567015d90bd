"""bench.py: a plain run measures the headline alone; every secondary section waits for --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = {"roofline", "binning", "knn", "ray_sweep", "skeleton", "ransac", "fps", "config5", "cpu_baseline"}
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    args = bench.parse()
    assert not args.full and args.steps == 4 and args.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-config5"])
    args = bench.parse()
    assert args.full and args.no_config5


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_the_last_step(gpu, tmp_path):
    from pyqsm_amd import hip, synth
    n = 50_000
    out = run_bench("--steps", "2", "--warmup", "1", "--points", str(n), "--dump-outputs", str(tmp_path))
    assert HEADLINE <= set(out) and not SECONDARY & set(out)
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["kernels"]["dbscan_total"]["launches"] == 2
    lab, core = hip.dbscan(synth.forest(n, seed=0), 0.1, 10, device=gpu)
    assert np.array_equal(np.load(tmp_path / "dbscan_labels.npy"), lab.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "dbscan_core.npy"), core.astype(np.float32))


@pytest.mark.gpu
def test_full_run_adds_every_secondary_section(gpu):
    out = run_bench("--full", "--steps", "2", "--warmup", "1", "--points", "200000", "--tris", "20000",
                    "--rays", "200000", "--ray-steps", "1", "--skel-iters", "2", "--no-config5")
    assert HEADLINE <= set(out) and SECONDARY - {"config5"} <= set(out)
    assert out["ray_sweep"]["culled"]["identical_to_brute_force"]
    assert out["fps"]["same_indices"]
    assert out["ransac"]["slices_of_a_tree"]["same_inliers_and_winner"]
