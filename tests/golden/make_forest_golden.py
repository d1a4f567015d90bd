"""Generates tests/golden/forest_small.npz: a fitted scikit-learn random forest as plain arrays
and what scikit-learn computes with it, so the inference contract (tests/forest_restatement.py,
DESIGN.md §12) stays pinned if a later scikit-learn changes.

Run in the build container (scikit-learn 1.7.2, NumPy 2.2.6):
    python tests/golden/make_forest_golden.py

15 unrestricted trees fitted on 3 000 rows of 7 features in 3 heavily overlapping Gaussian classes
(centres 0.35 standard deviations apart per axis: 19 583 nodes, 85 of the queries tie between two
classes); 2 000 queries, every 11th with NaN in one feature. Stored: the concatenated tree arrays
(tree_offsets, left, right, feature, threshold, missing_left, value, classes), X (float32),
and RandomForestClassifier's apply, predict_proba (n_jobs=1) and predict.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import forest_restatement as R  # noqa: E402


def main():
    from sklearn.ensemble import RandomForestClassifier
    Xall, yall = R.gaussian_classes(5000, 7, 3, seed=21, spread=0.35)
    Xtr, ytr, Xq = Xall[:3000], yall[:3000], Xall[3000:].copy()
    Xq[::11, 3] = np.nan
    rf = RandomForestClassifier(n_estimators=15, random_state=42, n_jobs=1).fit(Xtr, ytr)
    trees = R.trees_of(rf)
    sizes = [len(t[0]) for t in trees]
    proba = rf.predict_proba(Xq)
    srt = np.sort(proba, axis=1)
    out = dict(
        tree_offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
        left=np.concatenate([t[0] for t in trees]).astype(np.int32),
        right=np.concatenate([t[1] for t in trees]).astype(np.int32),
        feature=np.concatenate([t[2] for t in trees]).astype(np.int32),
        threshold=np.concatenate([t[3] for t in trees]).astype(np.float64),
        missing_left=np.concatenate([t[4] for t in trees]).astype(np.uint8),
        value=np.concatenate([t[5] for t in trees]).astype(np.float64),
        classes=rf.classes_.astype(np.int64), X=Xq,
        apply=rf.apply(Xq).astype(np.int32), predict_proba=proba, predict=rf.predict(Xq).astype(np.int64))
    path = os.path.join(HERE, "forest_small.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {sum(sizes)} nodes, "
          f"{int((srt[:, -1] == srt[:, -2]).sum())} tied rows of {len(Xq)}")


if __name__ == "__main__":
    main()
