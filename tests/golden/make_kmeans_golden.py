"""Writes tests/golden/kmeans_sklearn.npz: small general-position clouds with what scikit-learn's
KMeans(n_clusters=k, random_state=seed, n_init="auto") makes of them, and the points its k-means++
seeding chose (sklearn.cluster.kmeans_plusplus on the centred cloud, the same draws).

    python tests/golden/make_kmeans_golden.py

Needs scikit-learn (the goldens were written with 1.7.2); the tests only read the file. The clouds are
stored as float32, which they are exactly. Also prints how far the NumPy restatement
(tests/epiphyte_restatement.py) is from scikit-learn's centres and inertia: the figure DESIGN.md §22
records and tests/test_epiphyte_host.py bounds at 100 times."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import epiphyte_restatement as R  # noqa: E402

CASES = [  # name, kind, n, d, k, seed
    ("tree", "tree", 3000, 3, 20, 0),
    ("box", "box", 2000, 3, 20, 0),
    ("blobs", "blobs", 1500, 3, 8, 1),
    ("plane", "tree", 1500, 2, 5, 2),
    ("feature", "feature", 2000, 1, 2, 0),
]


def make_cloud(kind, n, d, seed):
    if kind == "feature":   # a smoothed feature column: two overlapping modes
        rng = np.random.default_rng(100 + seed)
        x = np.where(rng.random(n) < 0.4, rng.normal(0.2, 0.08, n), rng.normal(0.7, 0.12, n))[:, None]
    else:
        x = R.cloud(kind, n, d, seed=100 + seed)
    return np.ascontiguousarray(x.astype(np.float32))


def main():
    from sklearn.cluster import KMeans, kmeans_plusplus
    from pyqsm_amd.math_utils.clustering import kmeanspp_draws
    out = {"names": np.array([c[0] for c in CASES])}
    worst_centre = worst_inertia = 0.0
    for name, kind, n, d, k, seed in CASES:
        x32 = make_cloud(kind, n, d, seed)
        x = x32.astype(np.float64)
        km = KMeans(n_clusters=k, random_state=seed, n_init="auto").fit(x)
        _, idx = kmeans_plusplus(x - x.mean(axis=0), k, random_state=seed)
        out[f"{name}_x"] = x32
        out[f"{name}_k_seed"] = np.array([k, seed], np.int64)
        out[f"{name}_labels"] = km.labels_.astype(np.int32)
        out[f"{name}_centres"] = km.cluster_centers_.astype(np.float64)
        out[f"{name}_n_iter"] = np.int64(km.n_iter_)
        out[f"{name}_inertia"] = np.float64(km.inertia_)
        out[f"{name}_seeds"] = idx.astype(np.int64)
        first, u = kmeanspp_draws(n, k, seed)
        for tag, fn in (("chunk", R.kmeans_pp), ("plain", R.kmeans_pp_plain)):
            r = fn(x, k, first, u)
            same = np.array_equal(r.labels, km.labels_) and np.array_equal(r.seeds, idx) and r.n_iter == km.n_iter_
            dc = float(np.abs(r.centres - km.cluster_centers_).max())
            di = abs(r.inertia - km.inertia_) / km.inertia_
            print(f"{name:8s} {tag:5s} labels/seeds/n_iter equal: {same}  centres {dc:.3e}  inertia (rel) {di:.3e}")
            if tag == "chunk":
                worst_centre, worst_inertia = max(worst_centre, dc), max(worst_inertia, di)
    print(f"restatement against scikit-learn: centres {worst_centre:.3e}, inertia (relative) {worst_inertia:.3e}")
    path = os.path.join(HERE, "kmeans_sklearn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
