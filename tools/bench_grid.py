"""Timings of the grid representation (graphconvgeo_amd.grid) on one MI355X.

  windowed     grid_representation of N uniform points over the US box widened by 3 degrees, US
               grid at 0.5 degrees (5,800 columns), radius 161 km: Twitter-US size (450k rows).
               HIP events around the call (coordinates resident in HBM) and the host wall time:
               the call synchronizes once, for the entry count.
  exhaustive   the same rows with every column a candidate (exhaustive=True): what the window
               saves. Checked bitwise against the windowed result.
  numpy        the broadcast float64 restatement (tests/grid_reference.py) on the first
               --numpy-rows rows in the same run, checked against the device (structure exactly,
               values within one float32 ulp) and scaled to N for the comparison. The reference's
               own double loop makes one interpreted haversine call per (row, column) pair; it is
               timed on --loop-rows rows.

Prints one JSON line per measurement.
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
import grid_reference as ref  # noqa: E402
from graphconvgeo_amd import grid  # noqa: E402


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


def us_points(n, seed=77):
    rng = np.random.default_rng(seed)
    lllat, lllon, urlat, urlon = ref.US_BBOX
    return np.column_stack([rng.uniform(lllat - 3, urlat + 3, n), rng.uniform(lllon - 3, urlon + 3, n)])


def same(A, B):
    return all(torch.equal(a, b) for a, b in ((A.indptr, B.indptr), (A.indices, B.indices),
                                              (A.data.view(torch.int32), B.data.view(torch.int32))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=450_000)
    ap.add_argument("--grid-size", type=float, default=0.5)
    ap.add_argument("--radius", type=float, default=161.0)
    ap.add_argument("--numpy-rows", type=int, default=2_000)
    ap.add_argument("--loop-rows", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda")
    locs = us_points(args.rows)
    x = torch.as_tensor(locs, device=dev)
    kw = dict(grid_size=args.grid_size, bbox=ref.US_BBOX, radius_km=args.radius)
    g = grid.LatLonGrid(ref.US_BBOX, args.grid_size)
    base = {"rows": args.rows, "columns": g.n_points, "grid_size": args.grid_size,
            "radius_km": args.radius}

    ev, wall, X = timed(lambda: grid.grid_representation(x, **kw), args.reps)
    emit({"op": "grid_windowed", **base, "entries": X.nnz, "gpu_event_ms": round(ev, 3),
          "gpu_wall_ms": round(wall, 3), "ns_per_row": round(ev * 1e6 / args.rows, 1)})
    ev_x, wall_x, Xx = timed(lambda: grid.grid_representation(x, exhaustive=True, **kw), args.reps)
    emit({"op": "grid_exhaustive", **base, "entries": Xx.nnz, "gpu_event_ms": round(ev_x, 3),
          "gpu_wall_ms": round(wall_x, 3), "window_speedup": round(ev_x / ev, 1),
          "bitwise_equal_to_windowed": same(X, Xx)})

    m = min(args.numpy_rows, args.rows)
    t0 = time.perf_counter()
    want = ref.grid_representation(locs[:m], **kw)
    t_np = time.perf_counter() - t0
    got = X.row_slice(0, m)
    structure = bool(np.array_equal(got.indptr.cpu().numpy(), want.indptr) and
                     np.array_equal(got.indices.cpu().numpy(), want.indices))
    ulp = int(ref.ulp_distance(got.data.cpu().numpy(), want.data).max()) if structure else -1
    emit({"op": "numpy_restatement", "rows": m, "columns": g.n_points, "numpy_s": round(t_np, 3),
          "numpy_s_scaled_to_rows": round(t_np * args.rows / m, 1),
          "speedup_vs_numpy": round(t_np * args.rows / m * 1e3 / wall, 1),
          "structure_equal": structure, "max_ulp": ulp})
    k = min(args.loop_rows, m)
    t0 = time.perf_counter()
    ref.reference_loop(locs[:k], args.grid_size, ref.US_BBOX, args.radius)
    t_loop = time.perf_counter() - t0
    emit({"op": "reference_double_loop", "rows": k, "columns": g.n_points,
          "loop_s": round(t_loop, 3), "loop_s_scaled_to_rows": round(t_loop * args.rows / k, 0)})


if __name__ == "__main__":
    main()
