"""Writes tests/golden/kmeans_*.npz: Gaussian-blob problems rounded through float32, seeded by
the restatement's k-means++ (tests/kmeans_reference.py) and solved by
sklearn.cluster.KMeans(init=<array>, n_init=1, tol=0, algorithm="lloyd"). Needs scikit-learn;
the tests only read the files.

A case is written only if a different but legitimate summation order cannot change a label or
a pick:
  - the restatement and sklearn agree label for label (and on n_iter_, with no empty cluster),
  - the smallest relative gap between a point's best and second-best squared distance, over
    all iterations, is >= 1e-7,
  - the smallest distance of a k-means++ target from a prefix-sum boundary is >= 1e-9 of the
    total.

    python tests/golden/make_kmeans_golden.py
"""
import os
import sys

import numpy as np
from sklearn.cluster import KMeans

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import kmeans_reference as ref  # noqa: E402

# name -> (points, clusters, data seed, draw seed)
CASES = {"small": (3000, 16, 11, 1), "medium": (5000, 64, 12, 2), "large": (20000, 128, 13, 3)}
MIN_GAP = 1e-7
MIN_MARGIN = 1e-9


def make(name, n, c, data_seed, u_seed):
    x32 = ref.blobs(n, c, data_seed)
    x = x32.astype(np.float64)
    u = np.random.default_rng(u_seed).random(c)
    seeds, margin = ref.plusplus(x, c, u, return_margin=True)
    mine = ref.lloyd(x, x[seeds], return_gap=True)
    sk = KMeans(n_clusters=c, init=x[seeds], n_init=1, tol=0, algorithm="lloyd", max_iter=300).fit(x)
    problems = []
    if not np.array_equal(sk.labels_, mine["labels"]):
        problems.append(f"{int(np.sum(sk.labels_ != mine['labels']))} labels differ from sklearn's")
    if sk.n_iter_ != mine["n_iter"]:
        problems.append(f"n_iter {mine['n_iter']} against sklearn's {sk.n_iter_}")
    if mine["counts"].min() == 0:
        problems.append("an empty cluster")
    if not mine["gap"] >= MIN_GAP:
        problems.append(f"distance gap {mine['gap']:.3g} < {MIN_GAP}")
    if not margin >= MIN_MARGIN:
        problems.append(f"k-means++ margin {margin:.3g} < {MIN_MARGIN}")
    if problems:
        raise SystemExit(f"{name}: not written: " + "; ".join(problems))
    path = os.path.join(HERE, f"kmeans_{name}.npz")
    np.savez_compressed(path, points=x32, u=u, data_seed=data_seed, u_seed=u_seed, seeds=seeds,
                        labels=sk.labels_.astype(np.int32), centers=sk.cluster_centers_,
                        inertia=sk.inertia_, n_iter=sk.n_iter_, gap=mine["gap"], margin=margin)
    err = np.abs(sk.cluster_centers_ - mine["centers"]).max()
    print(f"{name}: {n} x {c}, n_iter {sk.n_iter_}, gap {mine['gap']:.3g}, margin {margin:.3g}, "
          f"centres within {err:.3g}, inertia rel "
          f"{abs(sk.inertia_ - mine['inertia']) / sk.inertia_:.3g}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    for name, args in CASES.items():
        make(name, *args)
