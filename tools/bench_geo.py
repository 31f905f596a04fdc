"""Timings of the geolocation labels and metrics (graphconvgeo_amd.geo) on one MI355X, each
beside the numpy restatement of the reference (tests/geo_reference.py) on the same inputs in
the same run, and checked against it:

  kdtree    KDTreeClustering.fit on N uniform points, bucket 2400: Twitter-World size
            (1.4M -> 1024 regions) and Twitter-US size (450k -> 256 regions). HIP events around
            the call (coordinates resident in HBM) and the host wall time beside them: the build
            synchronizes once per level, so the two differ by the readback latency.
  nearest   nearest_class: 10,000 queries x the resulting classes
  geo_eval  geo_eval at 10,000 rows (kernel + sort + the one host copy of the result)

The restatement is the baseline the issue names, not the reference's own KDTreeClustering (one
deepcopy per point: 1.6 s for 60k points, linear in N). Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geo_reference as ref  # noqa: E402
from graphconvgeo_amd import geo  # noqa: E402


def host_cores() -> int:
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def emit(rec):
    print(json.dumps(rec), flush=True)


def timed(fn, reps):
    """(median HIP-event ms, median wall ms, last result) of fn after one warm-up call."""
    out = fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return float(np.median(ev)), float(np.median(wall)), out


def cpu_timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def uniform_points(n, seed=77):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-60, 70, n), rng.uniform(-180, 180, n)])


def bench(name, n, bucket, dev, reps, queries):
    locs = uniform_points(n)
    x = torch.as_tensor(locs, device=dev)
    tree = geo.KDTreeClustering(bucket)
    ev, wall, _ = timed(lambda: tree.fit(x), reps)
    t_cpu, (want, num, depth) = cpu_timed(lambda: ref.kdtree_labels(locs, bucket))
    t_med, want_med = cpu_timed(lambda: ref.class_medians(locs, want, num))
    emit({"op": "kdtree_fit", "size": name, "points": n, "bucket": bucket,
          "classes": tree.num_clusters, "depth": tree.depth, "readbacks": tree.readbacks,
          "gpu_event_ms": round(ev, 3), "gpu_wall_ms": round(wall, 3),
          "numpy_labels_s": round(t_cpu, 3), "numpy_medians_s": round(t_med, 3),
          "speedup_vs_numpy_labels": round(t_cpu * 1e3 / wall, 1),
          "labels_equal": bool(np.array_equal(tree.clusters.cpu().numpy(), want)),
          "medians_bitwise": bool(np.array_equal(tree.medians.cpu().numpy(), want_med)),
          "host_cores": host_cores()})

    q = uniform_points(queries, seed=78)
    qd = torch.as_tensor(q, device=dev)
    ev, wall, idx = timed(lambda: geo.nearest_class(qd, tree.medians), reps)
    t_cpu, (want_idx, _) = cpu_timed(lambda: ref.nearest_class(q, want_med))
    emit({"op": "nearest_class", "size": name, "queries": queries, "classes": num,
          "gpu_event_ms": round(ev, 3), "gpu_wall_ms": round(wall, 3),
          "numpy_s": round(t_cpu, 3), "speedup_vs_numpy": round(t_cpu * 1e3 / wall, 1),
          "equal": bool(np.array_equal(idx.cpu().numpy(), want_idx)), "host_cores": host_cores()})

    pred = np.random.default_rng(79).integers(0, num, queries)
    pd_ = torch.as_tensor(pred, device=dev)
    ev, wall, got = timed(lambda: geo.geo_eval(pd_, qd, tree.medians), reps)
    t_cpu, (mean, median, acc, _) = cpu_timed(lambda: ref.geo_eval(pred, q, want_med))
    emit({"op": "geo_eval", "size": name, "rows": queries, "classes": num,
          "gpu_event_ms": round(ev, 3), "gpu_wall_ms": round(wall, 3),
          "numpy_s": round(t_cpu, 4), "speedup_vs_numpy": round(t_cpu * 1e3 / wall, 1),
          "mean_rel_err": abs(got[0] - mean) / mean, "median_abs_err_km": abs(got[1] - median),
          "acc_equal": bool(got[2] == acc), "host_cores": host_cores()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="twitter-us,twitter-world")
    ap.add_argument("--bucket", type=int, default=2400)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    points = {"small": 60_000, "twitter-us": 450_000, "twitter-world": 1_400_000}
    dev = torch.device("cuda")
    for name in args.sizes.split(","):
        bench(name, points[name], args.bucket, dev, args.reps, args.queries)


if __name__ == "__main__":
    main()
