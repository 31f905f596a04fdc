"""Timings of the dialect-embedding evaluation (graphconvgeo_amd.dialect) on one MI355X, with
the embeddings resident in HBM: V = 400 000 words, D in {300, 2048}, Q in {8, 256} queries with
about 100 gold words each, and one small shape where the launches are the cost.

  ranks       one gcg_neighbour_ranks_f32 beside a torch composition on the same device
              (torch.cdist in row chunks, then comparison counts against every pair's own
              distance: it writes and re-reads Q x chunk distances); the two alternate in one
              process, medians and spreads of HIP-event times. The kernel's work is counted from
              the shape: 2 float32 vector instructions (a subtraction, a fused multiply-add) per
              element of every (query, word) pair, and the bytes of E once per query tile. The
              bound is the larger of the two over their rates; the row says which.
  kneighbors  gcg_kneighbors_f32 at k = 50 beside cdist + topk per chunk + a final topk
  scale       gcg_minmax_l1_rows_f32 beside (x - min) / (max - min) and a row division in
              torch; the floor is two reads and one write of E
  host        sklearn's NearestNeighbors(algorithm='brute').kneighbors of full length where it
              is importable, else numpy, at --host-words words x 300 dimensions and --host-queries
              queries (a size it finishes)

One JSON line per measurement, appended to --out (profiles/dialect/bench.jsonl).
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
from graphconvgeo_amd import dialect as dl  # noqa: E402

# MI355X: 256 CUs x 4 SIMDs x 16 float32 lanes x 2.4 GHz, one unpacked vector instruction per
# lane and clock; HBM3E at the 6.3 TB/s a streaming copy reaches (8 TB/s on paper)
F32_OPS_PER_S = 256 * 4 * 16 * 2.4e9
HBM_BYTES_PER_S = 6.3e12
OPS_PER_ELEMENT = 2


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fa, fb, reps):
    """(median, min, max) HIP-event ms of fa and of fb, run in turn (A B A B ...) after a
    warm-up of each; fb may be None."""
    fa()
    if fb is not None:
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(event_ms(fa))
        if fb is not None:
            tb.append(event_ms(fb))
    stat = lambda t: (float(np.median(t)), float(min(t)), float(max(t))) if t else None
    return stat(ta), stat(tb)


def spread(name, s):
    return {f"{name}_ms": round(s[0], 4), f"{name}_min_ms": round(s[1], 4),
            f"{name}_max_ms": round(s[2], 4)}


def torch_ranks(e, q, ptr, word, gold, budget=1 << 28):
    """cdist in row chunks + comparison counts; ties by index. Every query has `gold` pairs."""
    nq, v = q.shape[0], e.shape[0]
    w = word.view(nq, gold).long()
    thr = torch.cdist(q[:, None, :], e[w]).squeeze(1)                     # [Q, G]
    counts = torch.zeros((nq, gold), dtype=torch.int64, device=e.device)
    chunk = max(256, min(v, budget // (nq * gold)))
    for s in range(0, v, chunk):
        d = torch.cdist(q, e[s:s + chunk])                                # [Q, chunk]
        ids = torch.arange(s, s + d.shape[1], device=e.device)
        below = (d[:, None, :] < thr[:, :, None]) | \
                ((d[:, None, :] == thr[:, :, None]) & (ids[None, None, :] < w[:, :, None]))
        counts += below.sum(dim=2)
    return counts.view(-1)


def torch_kneighbors(e, q, k, chunk=65536):
    best_d, best_i = None, None
    for s in range(0, e.shape[0], chunk):
        d = torch.cdist(q, e[s:s + chunk])
        dk, ik = torch.topk(d, min(k, d.shape[1]), dim=1, largest=False)
        ik = ik + s
        if best_d is not None:
            dk, ik = torch.cat([best_d, dk], dim=1), torch.cat([best_i, ik], dim=1)
        best_d, sel = torch.topk(dk, min(k, dk.shape[1]), dim=1, largest=False)
        best_i = torch.gather(ik, 1, sel)
    return best_d, best_i


def torch_scale(e):
    lo, hi = e.min(dim=0).values, e.max(dim=0).values
    rng = hi - lo
    y = (e - lo) / torch.where(rng == 0, torch.ones_like(rng), rng)
    norm = y.abs().sum(dim=1, keepdim=True)
    return y / torch.where(norm == 0, torch.ones_like(norm), norm)


def problem(v, d, nq, gold, dev, seed=5):
    gen = torch.Generator(device=dev).manual_seed(seed)
    raw = torch.randn((v, d), generator=gen, device=dev)
    rows = torch.randperm(v, generator=gen, device=dev)[:nq]
    word = torch.randint(0, v, (nq * gold,), generator=gen, device=dev, dtype=torch.int32)
    ptr = torch.arange(0, nq * gold + 1, gold, device=dev, dtype=torch.int32)
    return raw, rows, ptr, word


def bench(v, d, nq, gold, k, dev, reps, emit, with_torch=True):
    raw, rows, ptr, word = problem(v, d, nq, gold, dev)
    base = {"words": v, "dims": d, "queries": nq, "gold_per_query": gold}
    e_bytes = v * d * 4

    ours, theirs = alternate(lambda: dl._scale(raw), (lambda: torch_scale(raw)) if with_torch else None, reps)
    rec = {"op": "scale", **base, **spread("hip", ours), "floor_ms": round(3 * e_bytes / HBM_BYTES_PER_S * 1e3, 4),
           "fraction_of_hbm_rate": round(3 * e_bytes / HBM_BYTES_PER_S / (ours[0] * 1e-3), 3)}
    if theirs:
        rec.update(**spread("torch", theirs), speedup_vs_torch=round(theirs[0] / ours[0], 2))
    emit(rec)
    e = dl.scale_embeddings(raw)
    del raw
    q = e[rows].contiguous()

    tile = dl.tile("query_small") if nq <= dl.tile("query_small") else dl.tile("query")
    passes = -(-nq // tile)
    ops = OPS_PER_ELEMENT * passes * tile * v * d      # the tile's idle query slots are computed too
    t_valu, t_hbm = ops / F32_OPS_PER_S, passes * e_bytes / HBM_BYTES_PER_S
    ours, theirs = alternate(lambda: dl._ranks(e, q, ptr, word),
                             (lambda: torch_ranks(e, q, ptr, word, gold)) if with_torch else None, reps)
    rec = {"op": "ranks", **base, **spread("hip", ours), "passes_over_E": passes,
           "bound": "f32 vector rate" if t_valu >= t_hbm else "HBM rate",
           "bound_ms": round(max(t_valu, t_hbm) * 1e3, 4),
           "fraction_of_bound": round(max(t_valu, t_hbm) / (ours[0] * 1e-3), 3),
           "useful_f32_ops_per_s": round(OPS_PER_ELEMENT * nq * v * d / (ours[0] * 1e-3), -9),
           "e_bytes_floor_ms": round(e_bytes / HBM_BYTES_PER_S * 1e3, 4)}
    if theirs:
        same = float((torch_ranks(e, q, ptr, word, gold) == dl._ranks(e, q, ptr, word)[0]).double().mean())
        rec.update(**spread("torch", theirs), speedup_vs_torch=round(theirs[0] / ours[0], 2),
                   ranks_equal_to_torch=round(same, 6))
    emit(rec)

    kk = min(k, v)
    ours, theirs = alternate(lambda: dl.kneighbors(e, q, kk),
                             (lambda: torch_kneighbors(e, q, kk)) if with_torch else None, reps)
    rec = {"op": "kneighbors", **base, "k": kk, **spread("hip", ours)}
    if theirs:
        same = float((torch_kneighbors(e, q, kk)[1] == dl.kneighbors(e, q, kk)[1]).double().mean())
        rec.update(**spread("torch", theirs), speedup_vs_torch=round(theirs[0] / ours[0], 2),
                   indices_equal_to_torch=round(same, 6))
    emit(rec)


def host(v, d, nq, gold, dev, emit):
    """The reference's path at a size it finishes: scaling, a brute-force kneighbors of full
    length in float64 and the ranks read off it; beside the device at the same size."""
    raw, rows, ptr, word = problem(v, d, nq, gold, dev)
    x = raw.cpu().numpy().astype(np.float64)
    rows_h, word_h = rows.cpu().numpy(), word.cpu().numpy().reshape(nq, gold)
    try:
        from sklearn.neighbors import NearestNeighbors
        from sklearn.preprocessing import MinMaxScaler, normalize
        how = "sklearn"
    except ImportError:
        how = "numpy"
    t0 = time.perf_counter()
    if how == "sklearn":
        s = normalize(MinMaxScaler(feature_range=(0, 1)).fit_transform(x), norm="l1")
        t1 = time.perf_counter()
        _, idx = NearestNeighbors(n_neighbors=v, algorithm="brute").fit(s).kneighbors(s[rows_h])
    else:
        rng = x.max(axis=0) - x.min(axis=0)
        s = (x - x.min(axis=0)) / np.where(rng == 0, 1, rng)
        s /= np.abs(s).sum(axis=1, keepdims=True)
        t1 = time.perf_counter()
        idx = np.stack([np.argsort(((s - s[r]) ** 2).sum(axis=1), kind="stable") for r in rows_h])
    rank = np.empty_like(idx)
    np.put_along_axis(rank, idx, np.arange(v)[None, :], axis=1)
    host_ranks = np.take_along_axis(rank, word_h, axis=1).reshape(-1)
    t2 = time.perf_counter()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    e = dl.scale_embeddings(raw)
    got = dl.neighbour_ranks(e, rows, ptr, word).cpu().numpy()
    t4 = time.perf_counter()
    emit({"op": "host", "how": how, "words": v, "dims": d, "queries": nq, "gold_per_query": gold,
          "host_scale_s": round(t1 - t0, 3), "host_neighbours_s": round(t2 - t1, 3),
          "device_wall_s": round(t4 - t3, 4), "speedup": round((t2 - t0) / (t4 - t3), 1),
          "ranks_equal_to_host": round(float(np.mean(got == host_ranks)), 6)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--words", type=int, default=400_000)
    ap.add_argument("--dims", default="300,2048")
    ap.add_argument("--queries", default="8,256")
    ap.add_argument("--gold", type=int, default=100)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", default="3000,64,6", help="words,dims,queries of the launch-bound shape")
    ap.add_argument("--host-words", type=int, default=100_000)
    ap.add_argument("--host-queries", type=int, default=32)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dialect", "bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dev = torch.device("cuda")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    sv, sd, sq = (int(x) for x in args.small.split(","))
    bench(sv, sd, sq, min(args.gold, sv), args.k, dev, args.reps, emit, not args.no_torch)
    for d in (int(x) for x in args.dims.split(",")):
        for nq in (int(x) for x in args.queries.split(",")):
            bench(args.words, d, nq, args.gold, args.k, dev, args.reps, emit, not args.no_torch)
    if args.host_words > 0:
        host(args.host_words, 300, args.host_queries, args.gold, dev, emit)


if __name__ == "__main__":
    main()
