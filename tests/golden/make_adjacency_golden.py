"""Generates tests/golden/adjacency_blocks.npz: the labelled clouds of the cluster adjacency tests
and what SciPy's cKDTree.sparse_distance_matrix computes for them, cluster pair by cluster pair —
the loop of pyQSM/cluster_joining.py:139-155 — so the contract (tests/adjacency_restatement.py,
DESIGN.md §13) stays pinned if a later SciPy changes.

Run in the build container (SciPy 1.15.3, NumPy 2.2.6):
    python tests/golden/make_adjacency_golden.py

Block cloud: every fifth point of synth.forest(100 000, seed=3), labelled by its block of edge 0.8
(284 clusters); labels divisible by 3 are the sources. Recorded at thresholds 0.35, 0.2 and 0.01.
Lattice: arange(6)^3 * 0.25 in four label quadrants plus a copied source point, at threshold 0.25
(ties on the inclusive bound, a zero distance). Stored per case: rows (a, b), dist, n_pairs,
ascending by (a, b). The block points are stored as float32: every coordinate of the synthetic
forest is float32-representable, which the generator checks.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import adjacency_restatement as R  # noqa: E402

BLOCK_THRESHOLDS = (0.35, 0.2, 0.01)


def rows(d):
    keys = sorted(d)
    return (np.array(keys, dtype=np.int64).reshape(-1, 2), np.array([d[k][0] for k in keys], dtype=np.float64),
            np.array([d[k][1] for k in keys], dtype=np.int64))


def main():
    P, lab = R.block_cloud()
    assert np.array_equal(P.astype(np.float32).astype(np.float64), P)
    out = dict(block_points=P.astype(np.float32), block_labels=lab.astype(np.int32),
               block_thresholds=np.array(BLOCK_THRESHOLDS))
    s, sl, t, tl = R.split_blocks(P, lab)
    for k, thr in enumerate(BLOCK_THRESHOLDS):
        out[f"block{k}_ab"], out[f"block{k}_dist"], out[f"block{k}_pairs"] = rows(R.scipy_loop(s, sl, t, tl, thr))
    ls, lsl, lt, ltl = R.lattice()
    out.update(lattice_src=ls, lattice_src_labels=lsl, lattice_tgt=lt, lattice_tgt_labels=ltl,
               lattice_threshold=np.float64(0.25))
    out["lattice_ab"], out["lattice_dist"], out["lattice_pairs"] = rows(R.scipy_loop(ls, lsl, lt, ltl, 0.25))
    path = os.path.join(HERE, "adjacency_blocks.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; cluster pairs "
          + ", ".join(str(len(out[f'block{k}_ab'])) for k in range(len(BLOCK_THRESHOLDS)))
          + f" and {len(out['lattice_ab'])}")


if __name__ == "__main__":
    main()
