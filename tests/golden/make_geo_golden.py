"""Generate tests/golden/kdtree_labels.npz (run in the build container, never on the GPU box).

python tests/golden/make_geo_golden.py

The labels come from the reference's own `kdtree.KDTreeClustering` (kdtree.py:121-151),
imported from /root/reference at generation time with the two shims SURVEY.md §8c names
(`builtins.xrange`, `np.Inf`). Only data is written: the nine inputs, their bucket sizes and
the reference's labels and cluster counts. No reference source is copied.
"""
from __future__ import annotations

import builtins
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

CASE_NAMES = ("uniform", "cities", "identical", "const_lat", "split_eq_max", "bucket_one",
              "n_eq_bucket", "width_tie", "float32")


def cases(seed=77):
    """[(name, locs, bucket_size)]: one generator, drawn from in this order."""
    rng = np.random.default_rng(seed)
    out = []
    out.append((np.column_stack([rng.uniform(25, 50, 3000), rng.uniform(-125, -65, 3000)]), 50))
    cities = np.column_stack([rng.uniform(25, 50, 40), rng.uniform(-125, -65, 40)])
    pts = cities[rng.integers(0, 40, 3000)] + rng.normal(0.0, 0.05, (3000, 2))
    out.append((np.round(pts, 1), 37))
    out.append((np.tile([[37.25, -122.5]], (300, 1)), 10))
    out.append((np.column_stack([np.full(500, 41.0), rng.integers(0, 7, 500).astype(float)]), 20))
    out.append((np.column_stack([np.r_[np.zeros(10), np.ones(40)], np.full(50, 3.0)]), 5))
    out.append((np.column_stack([rng.uniform(25, 50, 257), rng.uniform(-125, -65, 257)]), 1))
    out.append((np.column_stack([rng.uniform(25, 50, 10), rng.uniform(-125, -65, 10)]), 10))
    out.append((np.array([[0, 0], [1, 1], [0, 1], [1, 0], [.5, .25]], dtype=np.float64), 2))
    f32 = np.column_stack([rng.uniform(25, 50, 2000), rng.uniform(-125, -65, 2000)])
    out.append((np.round(f32, 2).astype(np.float32), 64))
    return [(n, l, b) for n, (l, b) in zip(CASE_NAMES, out)]


def main():
    sys.path.insert(0, REF)
    builtins.xrange = range
    np.Inf = np.inf
    import kdtree  # /root/reference/kdtree.py

    out = {"names": np.array(CASE_NAMES)}
    for name, locs, bucket in cases():
        clusterer = kdtree.KDTreeClustering(bucket_size=bucket)
        clusterer.fit(locs)
        out[f"{name}_locs"] = locs
        out[f"{name}_bucket"] = np.int64(bucket)
        out[f"{name}_labels"] = np.asarray(clusterer.get_clusters(), dtype=np.int32)
        out[f"{name}_num"] = np.int64(clusterer.num_clusters)
        print(f"{name}: N={len(locs)} bucket={bucket} clusters={clusterer.num_clusters}")
    np.savez_compressed(os.path.join(HERE, "kdtree_labels.npz"), **out)


if __name__ == "__main__":
    main()
