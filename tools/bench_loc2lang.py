#!/usr/bin/env python
"""The location-to-language model's three kernels against their torch compositions, and one
trainer step (one JSON line per measurement; B = 1000 rows, C = 500 components, hid = 500,
V = 10,000 / 50,000 / 100,000 words, 64 words per row).

  xent     gcg_softmax_xent_csr_f32 (row losses and the logits' gradient, one launch, the target
           read as CSR rows through their ids) against the torch composition the reference
           implies: the batch's target rows densified into a B x V matrix, log_softmax, product,
           sum, and autograd's backward. Device events around back-to-back calls and the host
           clock around a synchronise. Beside the fused time: the fraction of the byte model
           3 * M * N * 4 (the logits read twice, the gradient written once) it reaches at the
           given HBM rate (GB/s = bytes / time).
  layer    gcg_bigaus_layer_f32 + gcg_bigaus_layer_backward_f32 against torch autograd of the
           reference's formulas (forward + backward from a given dG).
  adamax   gcg_adamax_step_f32 on a hid x V weight against the elementwise torch form.
  step     one NNModel_loc2lang training step; host clock per step over an epoch of 10.
The analyses (n = 4096 coordinates, the logits in the layout the model's GEMM writes):
  lse      gcg_row_lse_f64 against torch.logsumexp.
  colstats gcg_softmax_column_stats_f64 against the torch form: softmax, then the two column sums
           (sum p, sum p log p) in float64. Both kernels' times are also given under the byte
           model M * N * 4 (one read of the chunk) as a rate, and as a share of 6.3 TB/s.
  local    model.local_words(X) (the scan: logits, lse, column sums; V numbers come back) against
           local_words(model.predict(X)) (the n x V probabilities copied to the host, float64
           torch there); host clock, medians of --steps, the parent path's interquartile range,
           and whether the device path's median is below the parent's by more than that range.
Every pair alternates A and B in one process; medians of --steps (>= 20) after --warmup.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import scipy.sparse as sps
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from graphconvgeo_amd import loc2lang as L  # noqa: E402
from graphconvgeo_amd import sparse as gs  # noqa: E402

B, C, HID, WORDS = 1000, 500, 500, 64
N_GRID = 4096       # coordinates of the analyses' rows
STREAM_GBPS = 6300  # what a streaming kernel achieves on one MI355X


def device_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(xs):
    return round(float(np.median(xs)), 4)


def alternate(fa, fb, steps, warmup, timer):
    ta, tb = [], []
    for i in range(warmup + steps):
        a, b = timer(fa), timer(fb)
        if i >= warmup:
            ta.append(a)
            tb.append(b)
    return med(ta), med(tb)


def bag_of_words(n, V, rng):
    """n rows of WORDS distinct words each, l1-normalised, as scipy CSR float32."""
    indices = np.concatenate([np.sort(rng.choice(V, size=WORDS, replace=False)) for _ in range(n)])
    data = rng.random(n * WORDS).astype(np.float32) + 0.05
    data /= np.repeat(data.reshape(n, WORDS).sum(axis=1), WORDS)
    return sps.csr_matrix((data, indices.astype(np.int32), np.arange(0, n * WORDS + 1, WORDS,
                                                                      dtype=np.int32)), shape=(n, V))


def bench_xent(dev, V, steps, warmup, n_rows=4 * B):
    rng = np.random.default_rng(1)
    Y = L.target_csr(bag_of_words(n_rows, V, rng), dev)
    rows = torch.from_numpy(rng.permutation(n_rows)[:B].astype(np.int32)).to(dev)
    Z = torch.randn(B, V, generator=torch.Generator().manual_seed(1)).to(dev)
    indptr, idx64 = Y.indptr.to(torch.int64), Y.indices.to(torch.int64)

    def fused():
        L.xent_csr_forward_backward(Z, Y, rows, scale=1.0 / B)

    def composed():
        # loc2lang.py:253 on the device: the batch's rows densified, then the loss and autograd
        r = rows.to(torch.int64)
        counts = indptr[r + 1] - indptr[r]
        row_of = torch.repeat_interleave(torch.arange(B, device=dev), counts, output_size=B * WORDS)
        src = (indptr[r][:, None] + torch.arange(WORDS, device=dev)[None, :]).reshape(-1)
        Yd = torch.zeros((B, V), dtype=torch.float32, device=dev)
        Yd[row_of, idx64[src]] = Y.data[src]
        Zg = Z.detach().requires_grad_(True)
        (-(Yd * torch.log_softmax(Zg, dim=1)).sum(dim=1)).mean().backward()

    d = alternate(fused, composed, steps, warmup, lambda f: device_ms(f, 5))
    w = alternate(fused, composed, steps, warmup, wall_ms)
    model_bytes = 3 * B * V * 4
    return {"what": "softmax_xent_csr_fwd_bwd", "B": B, "V": V, "words_per_row": WORDS,
            "fused_device_ms": d[0], "torch_device_ms": d[1], "fused_wall_ms": w[0],
            "torch_wall_ms": w[1], "byte_model_MB": round(model_bytes / 1e6, 1),
            "fused_GBps_of_byte_model": round(model_bytes / (d[0] * 1e-3) / 1e9, 1)}


def torch_bigaus(X, mus, sig, cor):
    """BivariateGaussianLayer.get_output_for, line by line."""
    sigmas = torch.nn.functional.softplus(sig)
    corxy = torch.nn.functional.softsign(cor)
    diff = X[:, None, :] - mus[None, :, :]
    sigmainvs = 1.0 / sigmas
    sigmainvprods = sigmainvs[:, 0] * sigmainvs[:, 1]
    z = (diff ** 2 / sigmas ** 2).sum(dim=-1) - 2 * corxy * diff[:, :, 0] * diff[:, :, 1] * sigmainvprods
    inv = 1.0 / (1.0 - corxy ** 2)
    return torch.exp(math.log(0.5 / math.pi) + torch.log(sigmainvprods) +
                     torch.log(torch.sqrt(inv)) - 0.5 * z * inv)


def bench_layer(dev, V, steps, warmup):
    gen = torch.Generator().manual_seed(2)
    X = (10 * torch.randn(B, 2, generator=gen)).to(dev)
    mus = (10 * torch.randn(C, 2, generator=gen)).to(dev)
    sig = torch.full((C, 2), 10.0, device=dev)
    cor = torch.randn(C, generator=gen).to(dev)
    dG = torch.randn(B, C, generator=gen).to(dev)

    def fused():
        L.bigaus_forward(X, mus, sig, cor)
        L.bigaus_backward(X, mus, sig, cor, dG)

    def composed():
        leaves = [t.detach().requires_grad_(True) for t in (mus, sig, cor)]
        torch_bigaus(X, *leaves).backward(dG)

    d = alternate(fused, composed, steps, warmup, lambda f: device_ms(f, 10))
    w = alternate(fused, composed, steps, warmup, wall_ms)
    return {"what": "bigaus_layer_fwd_bwd", "B": B, "C": C, "fused_device_ms": d[0],
            "torch_device_ms": d[1], "fused_wall_ms": w[0], "torch_wall_ms": w[1]}


def bench_adamax(dev, V, steps, warmup):
    gen = torch.Generator(device=dev).manual_seed(3)
    p = torch.nn.Parameter(torch.randn(HID, V, generator=gen, device=dev))
    p.grad = torch.randn(HID, V, generator=gen, device=dev)
    opt = L.LasagneAdamax([p])
    q, g = p.detach().clone(), p.grad
    m, u = torch.zeros_like(q), torch.zeros_like(q)
    a_t = torch.full((), 2e-3 / (1 - 0.9), device=dev)

    def composed():
        m.mul_(0.9).add_(g, alpha=0.1)
        torch.maximum(u * 0.999, g.abs(), out=u)
        q.sub_(a_t * m / (u + 1e-8))

    d = alternate(opt.step, composed, steps, warmup, lambda f: device_ms(f, 5))
    n_bytes = 7 * HID * V * 4  # p, m, u read and written, g read
    return {"what": "adamax_step", "n": HID * V, "fused_device_ms": d[0], "torch_device_ms": d[1],
            "fused_GBps_of_7n_bytes": round(n_bytes / (d[0] * 1e-3) / 1e9, 1)}


def bench_step(dev, V, steps, warmup, n_batches=10):
    n = n_batches * B
    rng = np.random.default_rng(4)
    X = np.stack([rng.uniform(25, 49, n + B), rng.uniform(-124, -67, n + B)], axis=1).astype(np.float32)
    Y = bag_of_words(n + B, V, rng)
    np.random.seed(0)
    clf = L.NNModel_loc2lang(n_epochs=0, batch_size=B, hid_size=HID, n_gaus_comp=C, device=dev)
    clf.fit(X[:n], Y[:n], X[n:], Y[n:], X[n:], Y[n:])
    times = []
    for i in range(warmup + steps):
        order = rng.permutation(n)
        t = wall_ms(lambda: clf._train_epoch(order)) / n_batches
        if i >= warmup:
            times.append(t)
    return {"what": "train_step", "B": B, "C": C, "hid": HID, "V": V, "words_per_row": WORDS,
            "steps_per_epoch": n_batches, "ms_per_step": med(times)}


def grid_logits(dev, V):
    """N_GRID x V logits ~ N(0, 1) in empty_dense's layout, as the model's GEMM leaves them."""
    Z = gs.empty_dense(N_GRID, V, dev)
    Z.copy_(torch.randn(N_GRID, V, device=dev, generator=torch.Generator(device=dev).manual_seed(5)))
    return Z


def read_once(what, V, d, w):
    """A kernel that reads the chunk once against its torch form: the times, and the kernel's
    under the byte model M * N * 4."""
    model_bytes = N_GRID * V * 4
    rate = model_bytes / (d[0] * 1e-3) / 1e9
    return {"what": what, "M": N_GRID, "V": V, "fused_device_ms": d[0], "torch_device_ms": d[1],
            "fused_wall_ms": w[0], "torch_wall_ms": w[1],
            "byte_model_MB": round(model_bytes / 1e6, 1),
            "fused_GBps_of_byte_model": round(rate, 1),
            "share_of_streaming_rate": round(rate / STREAM_GBPS, 3)}


def bench_lse(dev, V, steps, warmup):
    Z = grid_logits(dev, V)

    def fused():
        L.row_lse(Z)

    def composed():
        torch.logsumexp(Z, dim=1)

    d = alternate(fused, composed, steps, warmup, lambda f: device_ms(f, 5))
    w = alternate(fused, composed, steps, warmup, wall_ms)
    return read_once("row_lse", V, d, w)


def bench_colstats(dev, V, steps, warmup):
    Z = grid_logits(dev, V)
    lse = L.row_lse(Z)
    S = torch.zeros(V, dtype=torch.float64, device=dev)
    T = torch.zeros_like(S)

    def fused():
        L.softmax_column_stats(Z, lse, S, T)

    def composed():
        P = torch.softmax(Z, dim=1).to(torch.float64)
        P.sum(dim=0), torch.special.xlogy(P, P).sum(dim=0)

    d = alternate(fused, composed, steps, warmup, lambda f: device_ms(f, 3))
    w = alternate(fused, composed, steps, warmup, wall_ms)
    return read_once("softmax_column_stats", V, d, w)


def bench_local(dev, V, steps, warmup):
    rng = np.random.default_rng(6)
    X = np.stack([rng.uniform(25, 49, N_GRID), rng.uniform(-124, -67, N_GRID)],
                 axis=1).astype(np.float32)
    np.random.seed(0)
    clf = L.NNModel_loc2lang(output_size=V, hid_size=HID, n_gaus_comp=C, device=dev)
    ta, tb = [], []
    for i in range(warmup + steps):
        a = wall_ms(lambda: clf.local_words(X))
        b = wall_ms(lambda: L.local_words(clf.predict(X)))
        if i >= warmup:
            ta.append(a)
            tb.append(b)
    q1, q3 = np.percentile(tb, [25, 75])
    return {"what": "local_words", "n": N_GRID, "C": C, "hid": HID, "V": V,
            "device_wall_ms": med(ta), "predict_then_host_wall_ms": med(tb),
            "predict_then_host_iqr_ms": round(float(q3 - q1), 4),
            "device_below_by_more_than_iqr": bool(med(ta) < med(tb) - (q3 - q1))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--vocab", type=int, nargs="+", default=[10_000, 50_000, 100_000])
    whats = ["xent", "layer", "adamax", "step", "lse", "colstats", "local"]
    ap.add_argument("--only", choices=whats, nargs="+", default=whats)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (medians of 20)")
    dev = torch.device("cuda:0")
    benches = {"xent": bench_xent, "layer": bench_layer, "adamax": bench_adamax, "step": bench_step,
               "lse": bench_lse, "colstats": bench_colstats, "local": bench_local}
    for what in args.only:
        for V in (args.vocab if what != "layer" else args.vocab[:1]):  # the layer has no V
            line = json.dumps(benches[what](dev, V, args.steps, args.warmup))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
