#!/usr/bin/env python
"""The mini-batch MLP's W1 step, epoch segmentation and whole epoch, against the composition of
the kernels the project had before it (one JSON line per measurement).

  step      gcg_minibatch_w1_step_f32 alone against the per-step composition built from the
            public API: DeviceCSR.rows_transpose(batch) (torch index ops, a host sync, a radix
            sort, a launch plan), sparse.spmm into an F x K gradient, gcg_l1l2_grad_f32, the sum
            of the two, gcg_adam_step_f32. Three numbers per shape: the fused kernel (device
            events around one call per batch, enqueued back to back), the composition's kernels
            alone with the transposed batches already built (the same way), and the composition as a trainer would pay for it (host clock
            around a synchronise, the transposition's host work included) beside the fused step
            timed the same way.
  segment   gcg_minibatch_segment over one epoch's batches (device events).
  epoch     one whole epoch of MLP at the config's size, the fused step against the same
            trainer stepping through the composition (host clock around a synchronise).
  --dropout [--hidden-dropout] [--hidden K]
            one whole epoch of DropoutMLP beside one of MLP, and the segmentation with and
            without the input mask.
  --only wide
            the rectify / dropout backward at 500 x 2048 and 10000 x 2048
            (gcg_rectify_backward_wide_f32) against the torch composition it stands in for.
Every pair alternates A and B in one process; medians of --steps (>= 20) after --warmup.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from graphconvgeo_amd import mlp as M  # noqa: E402
from graphconvgeo_amd import sparse as gs  # noqa: E402
from graphconvgeo_amd._native import call  # noqa: E402
from graphconvgeo_amd.sparse import _ptr, _stream_handle  # noqa: E402
from graphconvgeo_amd.synth import CONFIGS, glorot_uniform, synthetic_features  # noqa: E402

BETAS = (0.9, 0.999, 1e-8)


def composed_kernels(T, G, W, m, v, a_t, l1, l2, mode="auto"):
    """The composition's device work for one batch, its (X[batch])^T = T given: ~13 F x K
    streams (write dW; read W, write the penalty gradient; read both, write their sum; Adam
    reads p, g, m, v and writes p, m, v)."""
    stream = _stream_handle(W.device)
    dW = gs.spmm(T, G, mode=mode)  # F x K: zero rows and the touched rows' sums
    pen = torch.empty_like(W)
    call("gcg_l1l2_grad_f32", W.numel(), _ptr(W), l1, l2, None, _ptr(pen), stream)
    g = dW + pen
    call("gcg_adam_step_f32", W.numel(), _ptr(W), _ptr(g), _ptr(m), _ptr(v), _ptr(a_t), *BETAS,
         stream)


def composed_step(X, rows_host, G, W, m, v, a_t, l1, l2, mode="auto"):
    """The same with the transposition a new batch needs (nothing cached from other batches).
    mode: the SpMM's ('auto' as a user would run it; 'rowwise' never splits a row's sum, so the
    step is then bitwise the fused kernel's)."""
    X.__dict__.pop("_rows_t", None)
    T = X.rows_transpose(gs.RowSelection(rows_host, X.device))
    composed_kernels(T, G, W, m, v, a_t, l1, l2, mode)


def device_ms(fn, calls=1):
    """Device time per call of `calls` back-to-back calls fn(i): enqueued without a gap, so a
    kernel shorter than its own launch path is not timed by the host."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(i)
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


def bench_step(dev, F, K, B, nnz_per_row, steps, warmup, n_batches=20):
    X = synthetic_features(n_batches * B, F, nnz_per_row=nnz_per_row)
    Xd = gs.DeviceCSR.from_scipy(X, dev)
    perm = np.random.default_rng(1).permutation(X.shape[0]).astype(np.int32)
    seg = M.BatchSegments(Xd, torch.from_numpy(perm).to(dev), B, X.nnz)
    W = torch.from_numpy(glorot_uniform(F, K)).to(dev)
    Wc = W.clone()
    m, v, mc, vc = (torch.zeros_like(W) for _ in range(4))
    G = gs.empty_dense(B, K, dev).normal_().mul_(1e-3)
    a_t = torch.full((), 2e-3, dtype=torch.float32, device=dev)
    l1 = l2 = 5e-7
    rows = [perm[b * B:(b + 1) * B] for b in range(n_batches)]
    Ts = []
    for r in rows:  # the transposed batches, for the kernels-only figure
        Xd.__dict__.pop("_rows_t", None)
        Ts.append(Xd.rows_transpose(gs.RowSelection(r, dev)))
    t = {"fused_kernel": [], "composed_kernels": [], "fused_wall": [], "composed_wall": []}
    for i in range(warmup + steps):
        b = i % n_batches
        fused = lambda: M.w1_step(W, m, v, G, seg, b, l1, l2, a_t)  # noqa: E731
        x = (device_ms(lambda j: M.w1_step(W, m, v, G, seg, j, l1, l2, a_t), n_batches),
             device_ms(lambda j: composed_kernels(Ts[j], G, Wc, mc, vc, a_t, l1, l2), n_batches),
             wall_ms(fused),
             wall_ms(lambda: composed_step(Xd, rows[b], G, Wc, mc, vc, a_t, l1, l2)))
        if i >= warmup:
            for k, val in zip(t, x):
                t[k].append(val)
    seg_len = np.diff(Ts[0].indptr.cpu().numpy())
    rec = {"metric": "mlp W1 step, median ms", "F": F, "K": K, "B": B,
           "nnz_per_row": round(X.nnz / X.shape[0], 1), "touched_rows": int((seg_len > 0).sum()),
           "longest_segment": int(seg_len.max()), "steps": steps, "warmup": warmup,
           **{k + "_ms": med(x) for k, x in t.items()}}
    rec["fxk_stream_mb"] = round(F * K * 4 / 1e6, 2)
    rec["fused_kernel_gbps_of_6_streams"] = round(6 * F * K * 4 / rec["fused_kernel_ms"] / 1e6, 1)
    rec["ratio_kernels"] = round(rec["composed_kernels_ms"] / rec["fused_kernel_ms"], 3)
    rec["ratio_wall"] = round(rec["composed_wall_ms"] / rec["fused_wall_ms"], 3)
    print(json.dumps(rec), flush=True)


def composed_w1_update(clf, b, G, l1, l2, mode="auto"):
    """MLP._w1_update hook: the trainer's W1 update through the composition."""
    B, opt = clf.batch_size, clf.optimizer
    composed_step(clf.Xd, clf._perm_host[b * B:(b + 1) * B].astype(np.int32), G, clf.W1, clf.m1,
                  clf.v1, opt.a_t, l1, l2, mode)


def composed_w1_update_rowwise(clf, b, G, l1, l2):
    composed_w1_update(clf, b, G, l1, l2, mode="rowwise")


def bench_epoch(dev, cfg, n_train, B, nnz_per_row, steps, warmup, seg_steps):
    F, K, Cn = cfg.n_features, cfg.hidden, cfg.n_classes
    n_dev = 2 * B
    X = synthetic_features(n_train + n_dev, F, nnz_per_row=nnz_per_row)
    rng = np.random.default_rng(0)
    Y = rng.integers(0, Cn, size=n_train + n_dev)
    Y[:Cn] = np.arange(Cn)  # every class present: out_size = C
    init = (glorot_uniform(F, K), np.zeros(K, np.float32), glorot_uniform(K, Cn, seed=3),
            np.zeros(Cn, np.float32))
    Xtr = gs.DeviceCSR.from_scipy(X[:n_train], dev)
    Xdev = gs.DeviceCSR.from_scipy(X[n_train:], dev)

    def trainer(hook):
        clf = M.MLP(n_epochs=0, batch_size=B, hidden_layer_size=K, init_parameters=init,
                    regul_coefs=(1e-6, 1e-6), device=dev)
        clf.fit(Xtr, Y[:n_train], Xdev, Y[n_train:])
        clf._w1_update = hook
        return clf

    a, b = trainer(None), trainer(composed_w1_update)
    orders = [rng.permutation(n_train) for _ in range(warmup + steps)]
    # Faster must not be different: the same first epoch through the fused step and through the
    # composition with the never-split ('rowwise') SpMM gives the same bits in every parameter.
    # ('auto' may split the Zipf head's long rows: another summation order, and Adam's
    # m / sqrt(v) turns a last-bit difference of a near-zero gradient into a full step, so the
    # distance to that run says nothing; it is reported for completeness.)
    c = trainer(composed_w1_update_rowwise)
    a._train_epoch(orders[0])
    b._train_epoch(orders[0])
    c._train_epoch(orders[0])
    bitwise = all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                  for x, y in zip(a.params, c.params))
    diff = float((a.W1 - b.W1).abs().max())
    del c
    ta, tb = [], []
    for i in range(warmup + steps):
        x = (wall_ms(lambda: a._train_epoch(orders[i])), wall_ms(lambda: b._train_epoch(orders[i])))
        if i >= warmup:
            ta.append(x[0])
            tb.append(x[1])
    nb = M.n_batches(n_train, B)
    rec = {"metric": "mlp epoch, median ms", "config": cfg.name, "n_train": n_train, "F": F,
           "K": K, "C": Cn, "B": B, "batches": nb, "nnz_per_row": round(X.nnz / X.shape[0], 1),
           "steps": steps, "warmup": warmup, "epoch_fused_ms": med(ta),
           "epoch_composed_ms": med(tb), "ratio": round(med(tb) / med(ta), 3),
           "step_fused_ms": round(med(ta) / nb, 4), "step_composed_ms": round(med(tb) / nb, 4),
           "epoch_bitwise_equal_to_rowwise_composition": bitwise,
           "w1_max_abs_diff_to_auto_composition_after_one_epoch": diff}
    print(json.dumps(rec), flush=True)
    # the epoch segmentation alone
    perm = torch.from_numpy(orders[0][:nb * B].astype(np.int32)).to(dev)
    nnz_sel = int(np.diff(X[:n_train].indptr)[orders[0][:nb * B]].sum())
    ts = [device_ms(lambda _i: M.BatchSegments(Xtr, perm, B, nnz_sel))
          for _ in range(warmup + seg_steps)][warmup:]
    print(json.dumps({"metric": "mlp epoch segmentation, median ms", "config": cfg.name,
                      "rows": nb * B, "batches": nb, "entries": nnz_sel, "steps": seg_steps,
                      "segment_ms": med(ts),
                      "ns_per_entry": round(med(ts) * 1e6 / max(nnz_sel, 1), 3)}), flush=True)


def bench_dropout_epoch(dev, cfg, K, n_train, B, nnz_per_row, steps, warmup, hidden_dropout):
    """--dropout: one epoch of DropoutMLP beside one of MLP (the same class the parent commit
    has: its results are bitwise unchanged) on the same data, parameters and orders, alternated
    in one process; host clock around a synchronise."""
    F, Cn = cfg.n_features, cfg.n_classes
    n_dev = 2 * B
    X = synthetic_features(n_train + n_dev, F, nnz_per_row=nnz_per_row)
    rng = np.random.default_rng(0)
    Y = rng.integers(0, Cn, size=n_train + n_dev)
    Y[:Cn] = np.arange(Cn)  # every class present: out_size = C
    init = (glorot_uniform(F, K), np.zeros(K, np.float32), glorot_uniform(K, Cn, seed=3),
            np.zeros(Cn, np.float32))
    Xtr = gs.DeviceCSR.from_scipy(X[:n_train], dev)
    Xdev = gs.DeviceCSR.from_scipy(X[n_train:], dev)
    kw = dict(n_epochs=0, batch_size=B, hidden_layer_size=K, init_parameters=init,
              regul_coefs=(1e-6, 1e-6), device=dev)
    a = M.MLP(**kw).fit(Xtr, Y[:n_train], Xdev, Y[n_train:])
    b = M.DropoutMLP(hidden_dropout=hidden_dropout, **kw).fit(Xtr, Y[:n_train], Xdev, Y[n_train:])
    orders = [rng.permutation(n_train) for _ in range(warmup + steps)]
    ta, tb = [], []
    for i in range(warmup + steps):
        x = (wall_ms(lambda: a._train_epoch(orders[i])), wall_ms(lambda: b._train_epoch(orders[i])))
        if i >= warmup:
            ta.append(x[0])
            tb.append(x[1])
    nb = M.n_batches(n_train, B)
    nnz_sel = int(np.diff(X[:n_train].indptr)[orders[0][:nb * B]].sum())
    perm = torch.from_numpy(orders[0][:nb * B].astype(np.int32)).to(dev)
    seg_steps = max(steps, 5)
    ts = [device_ms(lambda _i: M.BatchSegments(Xtr, perm, B, nnz_sel))
          for _ in range(warmup + seg_steps)][warmup:]
    td = [device_ms(lambda _i: M.BatchSegments(Xtr, perm, B, nnz_sel, b._drop_in, b._vals_drop))
          for _ in range(warmup + seg_steps)][warmup:]
    rec = {"metric": "mlp epoch with dropout, median ms", "config": cfg.name, "n_train": n_train,
           "F": F, "K": K, "C": Cn, "B": B, "batches": nb, "entries": nnz_sel,
           "hidden_dropout": bool(hidden_dropout), "steps": steps, "warmup": warmup,
           "epoch_mlp_ms": med(ta), "epoch_dropout_ms": med(tb),
           "ratio": round(med(tb) / med(ta), 3), "step_mlp_ms": round(med(ta) / nb, 4),
           "step_dropout_ms": round(med(tb) / nb, 4), "segment_ms": med(ts),
           "segment_dropout_ms": med(td),
           "mask_ns_per_entry": round((med(td) - med(ts)) * 1e6 / max(nnz_sel, 1), 3)}
    print(json.dumps(rec), flush=True)


def bench_wide_backward(dev, Mr, K, steps, warmup, calls=20):
    """--only wide: the hidden layer's backward beyond 1024 columns alone, device events around
    `calls` back-to-back calls: gcg_rectify_backward_wide_f32 with the gate and with gate +
    mask, against the torch composition of sparse.epilogue_backward (three elementwise passes, a
    temporary and a sum) -- the only thing it can stand in for. Byte model: 9 B per element
    (gradient in, gate in, gradient out); the operands are re-read every call, so up to the
    Infinity Cache's size they may come from it."""
    from graphconvgeo_amd import dropout as D

    gY = gs.empty_dense(Mr, K, dev).normal_()
    gate = gs.empty_gate(Mr, K, dev)
    gate.copy_(torch.randint(0, 3, (Mr, K), device=dev, dtype=torch.uint8))
    stream = D.DropoutStream(7, 1, dev)
    stream.set_step(0)
    spec = D.DropoutSpec(stream, 0.5)
    legs = {"wide_gate": lambda _i: gs.relu_backward(gY, gate=gate),
            "wide_gate_dropout": lambda _i: D.dropout_relu_backward(gY, spec, gate=gate),
            "torch_composition": lambda _i: gs.epilogue_backward(gY, gate, True)}
    g0, db0 = legs["wide_gate"](0)
    g1, db1 = legs["torch_composition"](0)
    t = {k: [] for k in legs}
    for i in range(warmup + steps):
        for k, fn in legs.items():
            x = device_ms(fn, calls)
            if i >= warmup:
                t[k].append(x)
    nbytes = 9 * Mr * K
    rec = {"metric": "wide rectify backward, median ms", "M": Mr, "K": K, "steps": steps,
           "warmup": warmup, "calls_per_sample": calls, "mbytes_model": round(nbytes / 1e6, 2),
           "g_equal_to_composition": bool(torch.equal(g0, g1)),
           "db_max_abs_diff_to_composition": float((db0 - db1).abs().max())}
    for k, xs in t.items():
        rec[k + "_ms"] = med(xs)
        rec[k + "_gbps"] = round(nbytes / med(xs) / 1e6, 1)
        rec[k + "_share_of_8tbps"] = round(nbytes / med(xs) / 1e6 / 8000.0, 4)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--epoch-steps", type=int, default=20)
    ap.add_argument("--epoch-warmup", type=int, default=1)
    ap.add_argument("--config", default="twitter-us", choices=sorted(CONFIGS))
    ap.add_argument("--train-rows", type=int, default=0,
                    help="training rows of the epoch (0: 60 %% of the config's nodes)")
    ap.add_argument("--batch", type=int, default=500)
    ap.add_argument("--only", choices=["step", "epoch", "wide"], default=None)
    ap.add_argument("--dropout", action="store_true",
                    help="time the epoch and the step with DropoutMLP beside MLP")
    ap.add_argument("--hidden-dropout", action="store_true",
                    help="with --dropout: the hidden mask too")
    ap.add_argument("--hidden", type=int, default=0,
                    help="hidden units of the --dropout epoch (0: the config's)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mlp.py measures on a HIP device; none is visible")
    dev = torch.device("cuda:0")
    B = args.batch
    if args.only == "wide":  # the backward of a 2048-unit hidden layer at main.py's two batches
        for rows in (500, 10000):
            bench_wide_backward(dev, rows, 2048, args.steps, args.warmup)
        return
    if args.dropout or args.hidden_dropout:
        cfg = CONFIGS[args.config]
        n_train = args.train_rows or int(0.6 * cfg.n_nodes)
        bench_dropout_epoch(dev, cfg, args.hidden or cfg.hidden, n_train, B, 64, args.epoch_steps,
                            args.epoch_warmup, args.hidden_dropout)
        return
    if args.only in (None, "step"):
        bench_step(dev, 10_000, 500, B, 64, args.steps, args.warmup)
        bench_step(dev, 50_000, 300, B, 64, args.steps, args.warmup)
        bench_step(dev, 10_000, 500, B, 1000, args.steps, args.warmup, n_batches=8)
    if args.only in (None, "epoch"):
        cfg = CONFIGS[args.config]
        n_train = args.train_rows or int(0.6 * cfg.n_nodes)
        bench_epoch(dev, cfg, n_train, B, 64, args.epoch_steps, args.epoch_warmup, args.steps)


if __name__ == "__main__":
    main()
