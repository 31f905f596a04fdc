#!/usr/bin/env python
"""The three dropout kernels against their same-bytes twins, at one config's sizes.

  gcg_dropout_f32 (p = 0.5)            vs the same kernel at threshold 0 (same loads/stores,
                                          same Philox: is the pass ALU-bound?) and vs a copy
  gcg_dropout_relu_backward_f32        vs gcg_relu_backward_gate_f32 (same bytes, no Philox)
  gcg_csr_dropout_f32 on X and on X^T  (12 B per stored entry each)

Median of --steps device-event times after --warmup calls; one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from graphconvgeo_amd import dropout as D  # noqa: E402
from graphconvgeo_amd import sparse as gs  # noqa: E402
from graphconvgeo_amd.synth import CONFIGS, synthetic_features  # noqa: E402


def median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    marks[0].record()
    for i in range(steps):
        fn()
        marks[i + 1].record()
    torch.cuda.synchronize()
    return round(float(np.median([marks[i].elapsed_time(marks[i + 1]) for i in range(steps)])), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="twitter-world", choices=sorted(CONFIGS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nnz-per-row", type=int, default=64)
    ap.add_argument("--no-csr", action="store_true", help="skip the CSR passes (no X is built)")
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    dev = torch.device("cuda:0")
    n, K = cfg.n_nodes, cfg.hidden
    stream = D.DropoutStream(77, 1, dev)
    stream.advance()
    half, none = D.DropoutSpec(stream, 0.5), D.DropoutSpec(stream, 0.0)
    Y = gs.empty_dense(n, K, dev).normal_()
    G = gs.empty_dense(n, K, dev).normal_()
    out = gs.empty_dense(n, K, dev)
    gate = gs.empty_gate(n, K, dev)
    gate.copy_(torch.randint(0, 3, (n, K), dtype=torch.uint8, device=dev))
    t = lambda fn: median_ms(fn, args.steps, args.warmup)  # noqa: E731
    rec = {"metric": "dropout kernels, median ms", "config": cfg.name, "rows": n, "K": K,
           "ld": Y.stride(0), "steps": args.steps, "warmup": args.warmup,
           "dropout_f32_p0.5_in_place": t(lambda: D.dropout_dense(Y, half, out=Y)),
           "dropout_f32_threshold0_in_place": t(lambda: D.dropout_dense(Y, none, out=Y)),
           "dropout_f32_p0.5_out_of_place": t(lambda: D.dropout_dense(Y, half, out=out)),
           "copy_out_of_place": t(lambda: out.copy_(Y)),
           "dropout_relu_backward_f32": t(lambda: D.dropout_relu_backward(G, half, gate=gate,
                                                                          out=out)),
           "relu_backward_gate_f32": t(lambda: gs.relu_backward(G, gate=gate, out=out))}
    # the dense Zipf-head block of X (DeviceCSR._dense_column_split): scattered logical columns,
    # one Philox call per element
    fh = min(gs.HYBRID_MAX_COLS, cfg.n_features)
    Xh, Xh_out = gs.empty_dense(n, fh, dev).normal_(), gs.empty_dense(n, fh, dev)
    cols = torch.sort(torch.randperm(cfg.n_features, device=dev)[:fh]).values.to(torch.int32)
    rec["head_cols"] = fh
    rec["dropout_f32_head_col_ids"] = t(lambda: D.dropout_dense(Xh, half, out=Xh_out,
                                                                col_ids=cols))
    rec["dropout_f32_head_no_col_ids"] = t(lambda: D.dropout_dense(Xh, half, out=Xh_out))
    rec["ratio_backward_vs_gate_twin"] = round(
        rec["dropout_relu_backward_f32"] / rec["relu_backward_gate_f32"], 3)
    rec["ratio_dropout_vs_threshold0"] = round(
        rec["dropout_f32_p0.5_in_place"] / rec["dropout_f32_threshold0_in_place"], 3)
    if not args.no_csr:
        X = gs.DeviceCSR.from_scipy(
            synthetic_features(n, cfg.n_features, nnz_per_row=args.nnz_per_row), dev)
        T = X.transpose()
        vx, vt = torch.empty_like(X.data), torch.empty_like(T.data)
        rec.update(nnz_X=X.nnz, longest_row_Xt=T.max_row_nnz(),
                   csr_dropout_X=t(lambda: D.csr_dropout(X, X.data, vx, half)),
                   csr_dropout_Xt=t(lambda: D.csr_dropout(T, T.data, vt, half, transposed=True)))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
