"""Float64 numpy restatement of the reference's geolocation labels and metrics, used as the
yardstick of graphconvgeo_amd.geo:

  kdtree_labels   KDTreeClustering.fit (kdtree.py:84-151): the k-d-tree region labels
  class_medians   DataLoader.assignClasses' per-class medians (data.py:408-413)
  haversine_km    the `haversine` package's great-circle distance (radius is an argument)
  nearest_class   the brute-force 1-NN of data.py:416-419 (first index on ties)
  geo_eval        tensormain.geo_eval (tensormain.py:38-54)

tests/test_geo_reference.py pins kdtree_labels label for label against the reference's own
output (tests/golden/kdtree_labels.npz).
"""
from __future__ import annotations

import sys

import numpy as np

EARTH_RADIUS_KM = 6371.0088


def kdtree_labels(locs, bucket_size: int):
    """(labels int32[N], num_clusters, depth): the leaves of the reference's tree numbered in
    pre-order, left child first. depth = the number of levels on which some node splits."""
    locs = np.asarray(locs, dtype=np.float64)
    n = locs.shape[0]
    labels = np.zeros(n, np.int32)
    state = {"leaf": 0, "depth": 0}
    if n == 0:
        return labels, 0, 0
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 100_000))

    def split(ids, level):
        if ids.size > bucket_size:
            pts = locs[ids]
            lo, hi = pts.min(axis=0), pts.max(axis=0)
            dim = int(np.argmax(hi - lo))
            value = np.median(pts[:, dim])
            if lo[dim] != hi[dim]:
                if value == hi[dim]:
                    value = lo[dim]
                right = pts[:, dim] > value
                state["depth"] = max(state["depth"], level + 1)
                split(ids[~right], level + 1)
                split(ids[right], level + 1)
                return
        labels[ids] = state["leaf"]
        state["leaf"] += 1

    try:
        split(np.arange(n), 0)
    finally:
        sys.setrecursionlimit(limit)
    return labels, state["leaf"], state["depth"]


def class_medians(locs, labels, num_classes: int):
    locs = np.asarray(locs, dtype=np.float64)
    labels = np.asarray(labels)
    out = np.full((num_classes, 2), np.nan)
    for c in range(num_classes):
        pts = locs[labels == c]
        if pts.shape[0]:
            out[c] = np.median(pts[:, 0]), np.median(pts[:, 1])
    return out


def haversine_km(a, b, earth_radius_km: float = EARTH_RADIUS_KM):
    """Row-wise (broadcasting) distance between [lat, lon] degrees, as the haversine package
    computes it: 2 R asin(sqrt(sin^2(dlat/2) + cos(lat1) cos(lat2) sin^2(dlon/2)))."""
    a = np.radians(np.asarray(a, dtype=np.float64))
    b = np.radians(np.asarray(b, dtype=np.float64))
    lat = b[..., 0] - a[..., 0]
    lng = b[..., 1] - a[..., 1]
    d = np.sin(lat * 0.5) ** 2 + np.cos(a[..., 0]) * np.cos(b[..., 0]) * np.sin(lng * 0.5) ** 2
    return 2 * earth_radius_km * np.arcsin(np.sqrt(d))


def distance_matrix(locs, medians, earth_radius_km: float = EARTH_RADIUS_KM):
    locs = np.asarray(locs, dtype=np.float64)
    medians = np.asarray(medians, dtype=np.float64)
    return haversine_km(locs[:, None, :], medians[None, :, :], earth_radius_km)


def nearest_class(locs, medians, earth_radius_km: float = EARTH_RADIUS_KM):
    """(index int64[M], distance[M]) of the nearest median, the first index on ties."""
    d = distance_matrix(locs, medians, earth_radius_km)
    idx = d.argmin(axis=1)
    return idx, d[np.arange(d.shape[0]), idx]


def geo_eval(pred, locs, medians, earth_radius_km: float = EARTH_RADIUS_KM,
             threshold_km: float = 161.0):
    """(mean, median, acc_at_161, distances) of tensormain.geo_eval."""
    pred = np.asarray(pred)
    d = haversine_km(np.asarray(locs, np.float64), np.asarray(medians, np.float64)[pred],
                     earth_radius_km)
    acc = 100 * int((d < threshold_km).sum()) / float(d.size)
    return float(np.mean(d)), float(np.median(d)), acc, d
