"""Timings of the k-means initialisation (graphconvgeo_amd.kmeans) on one MI355X, at
N in {100k, 450k, 1.4M} points x C in {100, 500, 1000} clusters, coordinates resident in HBM:

  assign   one gcg_kmeans_assign_f64 beside a torch composition on the same device (row-chunked
           cdist / argmin); the two alternate in one process, medians of HIP-event times. The
           kernel's float64 operations are counted (6 per point-centre pair: 2 subtractions, 2
           products, 1 sum, 1 comparison) and set against the vector rate without fused
           multiply-adds.
  update   one gcg_kmeans_update_f64 beside index_add_ / bincount (which uses atomics, so its
           sums change from run to run)
  seed     kmeans_plusplus: C sequential rounds of two launches
  fit      KMeans.fit from those seeds, with its iteration count
  stats    cluster_stats beside the host loop mdn.cluster_params

and, where scikit-learn is installed, sklearn's KMeans (from the same seeds, tol=0, up to
--sklearn-full-points points) and MiniBatchKMeans(batch_size=1000) on the host. One JSON line
per measurement, appended to --out (profiles/kmeans/bench.jsonl).
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
from graphconvgeo_amd import kmeans as K  # noqa: E402
from graphconvgeo_amd import mdn  # noqa: E402

# MI355X: 256 CUs x 4 SIMDs x 16 float64 lanes x 2.4 GHz, one operation per lane and clock
# (the published 78.6 TFLOP/s counts a fused multiply-add as two)
F64_OPS_PER_S = 256 * 4 * 16 * 2.4e9
OPS_PER_PAIR = 6


def host_cores() -> int:
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def alternate(fa, fb, reps):
    """Median HIP-event ms of fa and of fb, run in turn (A B A B ...) after a warm-up of each."""
    fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(event_ms(fa)[0])
        tb.append(event_ms(fb)[0])
    return float(np.median(ta)), float(np.median(tb))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def blob_points(n, seed=77):
    rng = np.random.default_rng(seed)
    mid = np.column_stack([rng.uniform(-60, 70, 2000), rng.uniform(-180, 180, 2000)])
    return (mid[rng.integers(0, 2000, n)] + 1.5 * rng.standard_normal((n, 2))).astype(np.float32)


def torch_assign(x, centers, chunk=65536):
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for s in range(0, x.shape[0], chunk):
        out[s:s + chunk] = torch.cdist(x[s:s + chunk], centers).argmin(dim=1)
    return out


def torch_update(x, labels64, c):
    sums = torch.zeros((c, 2), dtype=torch.float64, device=x.device).index_add_(0, labels64, x)
    return sums / torch.bincount(labels64, minlength=c).clamp(min=1)[:, None]


def bench(n, c, dev, reps, args, emit):
    pts = blob_points(n)
    x = torch.as_tensor(pts, device=dev).to(torch.float64)
    base = {"points": n, "clusters": c, "host_cores": host_cores()}

    t_seed, seeds = wall(lambda: K.kmeans_plusplus(x, c, seed=1))
    t_seed2, _ = wall(lambda: K.kmeans_plusplus(x, c, seed=1))
    emit({"op": "seed", **base, "gpu_wall_ms": round(min(t_seed, t_seed2) * 1e3, 3),
          "us_per_round": round(min(t_seed, t_seed2) * 1e6 / c, 2)})
    centers = x[seeds.long()]

    ours, theirs = alternate(lambda: K._assign(x, centers, None, True),
                             lambda: torch_assign(x, centers), reps)
    lab = K.kmeans_assign(x, centers).labels
    lab64 = lab.long()
    same = float((torch_assign(x, centers) == lab64).double().mean())
    emit({"op": "assign", **base, "hip_ms": round(ours, 4), "torch_ms": round(theirs, 4),
          "speedup_vs_torch": round(theirs / ours, 2),
          "f64_ops_per_s": round(OPS_PER_PAIR * n * c / (ours * 1e-3), -9),
          "fraction_of_f64_vector_rate": round(OPS_PER_PAIR * n * c / (ours * 1e-3) / F64_OPS_PER_S, 3),
          "labels_equal_to_torch": round(same, 6)})

    ours, theirs = alternate(lambda: K._update(x, lab, centers),
                             lambda: torch_update(x, lab64, c), reps)
    emit({"op": "update", **base, "hip_ms": round(ours, 4), "torch_ms": round(theirs, 4),
          "speedup_vs_torch": round(theirs / ours, 2)})

    t_fit, km = wall(lambda: K.KMeans(c, init=centers, max_iter=args.max_iter).fit(x))
    emit({"op": "fit", **base, "gpu_wall_s": round(t_fit, 4), "n_iter": km.n_iter_,
          "ms_per_iter": round(t_fit * 1e3 / km.n_iter_, 3), "inertia": km.inertia_,
          "readbacks": km.readbacks_, "empty_clusters": int((km.counts_ == 0).sum())})

    ours = float(np.median([event_ms(lambda: K.cluster_stats(x, km.labels_, c,
                                                             centers=km.cluster_centers_))[0]
                            for _ in range(reps + 1)][1:]))
    rec = {"op": "stats", **base, "hip_ms": round(ours, 4)}
    if n * c <= args.host_stats_pairs:
        labels_h = km.labels_.cpu().numpy()
        keep = np.flatnonzero(np.bincount(labels_h, minlength=c))  # the host loop refuses empties
        remap = np.full(c, -1)
        remap[keep] = np.arange(len(keep))
        t0 = time.perf_counter()
        mdn.cluster_params(pts, remap[labels_h], len(keep))
        rec["host_cluster_params_s"] = round(time.perf_counter() - t0, 3)
        rec["speedup_vs_host"] = round(rec["host_cluster_params_s"] * 1e3 / ours, 1)
    emit(rec)

    try:
        from sklearn.cluster import KMeans, MiniBatchKMeans
    except ImportError:
        return
    x64 = pts.astype(np.float64)
    t0 = time.perf_counter()
    mb = MiniBatchKMeans(n_clusters=c, batch_size=1000).fit(x64)
    emit({"op": "sklearn_minibatch", **base, "host_s": round(time.perf_counter() - t0, 3),
          "inertia": float(mb.inertia_), "inertia_over_fit": round(float(mb.inertia_) / km.inertia_, 4)})
    if n <= args.sklearn_full_points:
        t0 = time.perf_counter()
        sk = KMeans(n_clusters=c, init=centers.cpu().numpy(), n_init=1, tol=0, algorithm="lloyd",
                    max_iter=args.max_iter).fit(x64)
        t_sk = time.perf_counter() - t0
        emit({"op": "sklearn_kmeans", **base, "host_s": round(t_sk, 3),
              "n_iter": int(sk.n_iter_), "inertia": float(sk.inertia_),
              "speedup_of_fit": round(t_sk / t_fit, 1),
              "labels_equal": bool(np.array_equal(sk.labels_, km.labels_.cpu().numpy()))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="100000,450000,1400000")
    ap.add_argument("--clusters", default="100,500,1000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--sklearn-full-points", type=int, default=100_000,
                    help="largest N at which sklearn's full KMeans is timed on the host")
    ap.add_argument("--host-stats-pairs", type=int, default=1_500_000_000,
                    help="largest N x C at which the host cluster_params loop is timed")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans", "bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dev = torch.device("cuda")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    for n in (int(v) for v in args.points.split(",")):
        for c in (int(v) for v in args.clusters.split(",")):
            bench(n, c, dev, args.reps, args, emit)


if __name__ == "__main__":
    main()
