"""Writes tests/golden/dialect_*.npz: float32 Gaussian embeddings pushed through sklearn's
MinMaxScaler(feature_range=(0, 1)) and normalize(norm='l1') in float64, and the full-length
NearestNeighbors(algorithm='brute').kneighbors of a few rows of the scaled matrix. Recorded
inputs and results only. Needs scikit-learn; the tests only read the files.

A case is written only if
  - the restatement (tests/dialect_reference.py) and sklearn agree on every index of every
    query's ordering,
  - neighbouring distances of every ordering differ by at least 1e-6 relative, so that
    sklearn's float64 expansion form and the difference form cannot disagree,
  - the restatement's scaling is within 1e-15 of sklearn's.

    python tests/golden/make_dialect_golden.py
"""
import os
import sys

import numpy as np
from sklearn.neighbors import NearestNeighbors
from sklearn.preprocessing import MinMaxScaler, normalize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dialect_reference as ref  # noqa: E402

# name -> (words, dimensions, queries, data seed)
CASES = {"small": (120, 5, 4, 21), "medium": (300, 48, 4, 22), "wide": (150, 300, 3, 22)}
MIN_GAP = 1e-6


def make(name, v, d, nq, seed):
    x32 = ref.gaussian_embeddings(v, d, seed)
    if name == "small":
        x32[:, 2] = 1.5       # a constant column: scale 1, every scaled value 0
    rows = np.random.default_rng(seed + 100).choice(v, size=nq, replace=False).astype(np.int32)
    scaled = MinMaxScaler(feature_range=(0, 1)).fit_transform(x32.astype(np.float64))
    scaled = normalize(scaled, norm="l1", axis=1)
    mine = ref.scale(x32)
    dist, idx = NearestNeighbors(n_neighbors=v, algorithm="brute").fit(scaled).kneighbors(scaled[rows])
    my_dist, my_idx = ref.kneighbors(scaled, rows, v)
    gap = ref.min_relative_gap(scaled, rows)
    problems = []
    if not np.array_equal(idx, my_idx):
        problems.append(f"{int(np.sum(idx != my_idx))} indices differ from sklearn's")
    if not gap >= MIN_GAP:
        problems.append(f"distance gap {gap:.3g} < {MIN_GAP}")
    if not np.abs(mine - scaled).max() <= 1e-15:
        problems.append(f"scaling differs from sklearn's by {np.abs(mine - scaled).max():.3g}")
    if problems:
        raise SystemExit(f"{name}: not written: " + "; ".join(problems))
    path = os.path.join(HERE, f"dialect_{name}.npz")
    np.savez_compressed(path, embs=x32, seed=seed, rows=rows, scaled=scaled,
                        indices=idx.astype(np.int32), distances=dist, gap=gap)
    print(f"{name}: {v} x {d}, {nq} queries, gap {gap:.3g}, scaling within "
          f"{np.abs(mine - scaled).max():.3g}, distances within "
          f"{np.abs(my_dist - dist).max():.3g}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for name, args in CASES.items():
        make(name, *args)
