"""CPU model of the DBSCAN union phase's hook pass (dbscan.hip: k_hook_sub, the summary words, the seam
test of k_union_sub): how many trees and seam sub-cells are left when every sub-cell is united with its
first K connected neighbours among the 13 near negative offsets.

    python tools/hook_model.py [n] [--eps 0.1] [--min-pts 10] [--links 3] [--seed 0] [--cloud forest|uniform]
    python tools/hook_model.py --npy cloud.npy --eps 0.05 --min-pts 5

NumPy / SciPy only, no GPU. The grid is the device's: cells of edge eps (1 + 2^-20) from the bounding
box's minimum, sub-cells of half a cell. K = 1 is the hook pass alone; K = 2 adds the second link that
k_flatten_reps unites across. A million points take a few minutes and a few GB (all pairs within eps)."""
import argparse
import os
import sys

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

# the 13 lexicographically positive (dz, dy, dx) offsets of max-norm 1 as (dx, dy, dz), in the order
# k_hook_sub's lanes take them (the first 13 of kSubOffsets): the neighbour sits at MINUS the offset
NEAR = np.array([(1, 0, 0), (-1, 1, 0), (0, 1, 0), (1, 1, 0), (-1, -1, 1), (0, -1, 1), (1, -1, 1), (-1, 0, 1),
                 (0, 0, 1), (1, 0, 1), (-1, 1, 1), (0, 1, 1), (1, 1, 1)], dtype=np.int64)


def _key(h):
    """One int64 per row of non-negative integer triples (at most 2^20 per axis)."""
    return (h[:, 2] << 42) | (h[:, 1] << 21) | h[:, 0]


def sub_cell_links(P, eps, min_pts, radius_inclusive=True):
    """The core flags, the half-cell coordinates of the listed sub-cells (those with a core point), and for
    every sub-cell the sub-cells at its near negative offsets that it shares a core-core pair within eps
    with: arrays (s, t, nb) sorted by (s, t), t the offset's place in NEAR. Also the number of clusters."""
    P = np.ascontiguousarray(P, dtype=np.float64)
    r = eps if radius_inclusive else np.nextafter(eps, 0.0)
    tree = cKDTree(P)
    core = tree.query_ball_point(P, r, return_length=True) >= min_pts
    C = P[core]
    cell = eps * (1.0 + 1.0 / 1048576.0)
    h = np.floor((C - P.min(axis=0)) * (2.0 / cell)).astype(np.int64) + 2   # (+ 2: room for the offsets)
    keys, sub_of = np.unique(_key(h), return_inverse=True)
    m = keys.size
    hs = np.zeros((m, 3), dtype=np.int64)
    hs[sub_of] = h
    pairs = cKDTree(C).query_pairs(r, output_type="ndarray")
    a, b = sub_of[pairs[:, 0]], sub_of[pairs[:, 1]]
    clusters = connected_components(coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(m, m)), directed=False)[0]
    # sub-cell edges, each from the lexicographically larger (z, y, x) end: its neighbour is at a negative offset
    e = np.unique(np.stack([np.maximum(keys[a], keys[b]), np.minimum(keys[a], keys[b])], -1), axis=0)
    s, nb = np.searchsorted(keys, e[:, 0]), np.searchsorted(keys, e[:, 1])
    d = hs[s] - hs[nb]
    near = (np.abs(d).max(axis=1) == 1)
    s, nb, d = s[near], nb[near], d[near]
    t = np.argmax((d[:, None, :] == NEAR[None, :, :]).all(axis=2), axis=1)
    o = np.lexsort((t, s))
    return core, hs, s[o], t[o], nb[o], clusters


def trees_and_seams(hs, s, nb):
    """Trees of the sub-cell graph with the edges (s, nb), and the sub-cells k_union_sub would give the full
    treatment: those with a cell among the 18 of their own z-layer and the one below whose word is mixed or
    names another tree."""
    m = hs.shape[0]
    trees, root = connected_components(coo_matrix((np.ones(s.size, np.int8), (s, nb)), shape=(m, m)), directed=False)
    c = hs >> 1
    ckeys, cell_of = np.unique(_key(c), return_inverse=True)
    lo = np.full(ckeys.size, m, dtype=np.int64)
    hi = np.full(ckeys.size, -1, dtype=np.int64)
    np.minimum.at(lo, cell_of, root)
    np.maximum.at(hi, cell_of, root)
    word = np.where(lo == hi, lo, -1)                      # the cell's tree, or mixed
    seam = np.zeros(m, dtype=bool)
    mixed_touch = np.zeros(m, dtype=bool)
    for dz in (0, -1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k2 = _key(c + np.array([dx, dy, dz]))
                i = np.minimum(np.searchsorted(ckeys, k2), ckeys.size - 1)
                there = ckeys[i] == k2
                seam |= there & (word[i] != root)
                mixed_touch |= there & (word[i] == -1)
    return trees, root, seam, int((word == -1).sum()), mixed_touch


def table(P, eps, min_pts, max_links=3, radius_inclusive=True, out=sys.stdout):
    core, hs, s, t, nb, clusters = sub_cell_links(P, eps, min_pts, radius_inclusive)
    m = hs.shape[0]
    # place of every edge among its sub-cell's connected near neighbours, nearest first
    first = np.r_[True, s[1:] != s[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(s.size), 0))
    place = np.arange(s.size) - start
    per_sub = np.bincount(s, minlength=m)
    print(f"points {P.shape[0]}, non-core {int((~core).sum())}, listed sub-cells {m}, clusters {clusters}", file=out)
    print(f"sub-cells with >= 2 connected near-negative neighbours {int((per_sub >= 2).sum())}, "
          f"with one {int((per_sub == 1).sum())}, with none {int((per_sub == 0).sum())}", file=out)
    print("| near links per sub-cell | links | trees after | seam sub-cells | mixed cells | seams touching one |", file=out)
    print("|---|---|---|---|---|---|", file=out)
    rows = {}
    for K in list(range(1, max_links + 1)) + [13]:
        use = place < K
        trees, root, seam, mixed, touch = trees_and_seams(hs, s[use], nb[use])
        rows[K] = (int(use.sum()), trees, int(seam.sum()))
        name = "all 13" if K == 13 else str(K) + (" (the hook pass alone)" if K == 1 else "")
        print(f"| {name} | {int(use.sum())} | {trees} | {int(seam.sum())} | {mixed} | {int((seam & touch).sum())} |",
              file=out)
        if K == 1:
            root1 = root
    if max_links >= 2:
        second = place == 1
        crossing = int((root1[s[second]] != root1[nb[second]]).sum())
        print(f"second links that join two different first-link trees {crossing}, "
              f"unions that succeed {rows[1][1] - rows[2][1]}", file=out)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--min-pts", type=int, default=10)
    ap.add_argument("--links", type=int, default=3, help="largest K of the table")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cloud", choices=["forest", "uniform"], default="forest")
    ap.add_argument("--npy", help="an (n, 3) array instead of a synthetic cloud")
    a = ap.parse_args()
    if a.npy:
        P = np.load(a.npy)
    elif a.cloud == "forest":
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from pyqsm_amd import synth
        P = synth.forest(a.n, seed=a.seed)
    else:
        P = np.random.default_rng(a.seed).uniform(0, 1, (a.n, 3))
    table(P, a.eps, a.min_pts, a.links)


if __name__ == "__main__":
    main()
