#!/usr/bin/env python
"""The mixture-density head's two kernels against their torch compositions, and one trainer
step (one JSON line per measurement; B = 1000 rows, hid = 300, C = 100 / 300 / 900 components).

  nll       gcg_mdn_nll_f32 (loss and gradient, one launch plus the one-workgroup mean) against
            the torch composition of the same formulas with autograd (forward + backward),
            device events around back-to-back calls and the host clock around a synchronise.
  predict   gcg_mdn_predict_f32 ("mixture") against a torch broadcast form of the same C x C
            scores, rows taken in chunks that keep the intermediates under 1 GB.
  step      one NNModel_lang2loc training step (forward over the batch's rows, tanh, output
            GEMM, NLL, backward GEMMs, tanh backward, W1 step) at F = 10,000, 64 nonzeros per
            row, with and without input dropout; host clock per step over an epoch of 20.
The shared-component model (--only, not in the default set):
  shared          gcg_mdn_shared_nll_f32 (loss, the logits' and the 5 C parameter gradients, one
                  call of four launches) against the torch-autograd composition of the formulas.
  shared_predict  gcg_mdn_shared_predict_f32 ("mixture") against torch.softmax(L) @ Dt and
                  argmax, the C x C density table given to both; the table's time beside them.
  shared_step     one NNModel_lang2locshared training step, beside NNModel_lang2loc's.
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
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from graphconvgeo_amd import mdn as M  # noqa: E402
from graphconvgeo_amd.synth import synthetic_features  # noqa: E402

B, HID = 1000, 300


def torch_unpack(O, C):
    O = O.reshape(-1, 6, C)
    scale = torch.tensor([90.0, 180.0], device=O.device)[None, :, None]
    return (scale * torch.tanh(O[:, 0:2]), 10 * torch.nn.functional.softplus(O[:, 2:4]),
            torch.nn.functional.softsign(O[:, 4]), O[:, 5])


def torch_nll(O, Y, C):
    """lang2loc.nll_loss, line by line (log pi as log_softmax), on the device."""
    mus, sigmas, corxy, logits = torch_unpack(O, C)
    diff = Y[:, :, None] - mus
    sigmainvs = 1.0 / sigmas
    sigmainvprods = sigmainvs[:, 0] * sigmainvs[:, 1]
    z = (diff ** 2 * sigmainvs ** 2).sum(dim=1) - 2 * corxy * diff[:, 0] * diff[:, 1] * sigmainvprods
    inv = 1.0 / (1.0 - corxy ** 2)
    e = -0.5 * z * inv + math.log(0.5 / math.pi) + torch.log(sigmainvprods) + \
        torch.log(torch.sqrt(inv)) + torch.log_softmax(logits, dim=1)
    return -torch.logsumexp(e, dim=1).mean()


def torch_predict(O, C, rows_per_chunk):
    out = []
    for s in range(0, O.shape[0], rows_per_chunk):
        mus, sigmas, corxy, logits = torch_unpack(O[s:s + rows_per_chunk], C)
        pis = torch.softmax(logits, dim=1)
        diff = mus[:, :, :, None] - mus[:, :, None, :]          # [b, 2, candidate, k]
        inv_s = 1.0 / sigmas[:, :, None, :]
        u = diff * inv_s
        rho = corxy[:, None, :]
        inv = 1.0 / (1.0 - rho ** 2)
        z = (u ** 2).sum(dim=1) - 2 * rho * u[:, 0] * u[:, 1]
        probs = (0.5 / math.pi) * inv_s[:, 0] * inv_s[:, 1] * torch.sqrt(inv) * torch.exp(-0.5 * z * inv)
        idx = (pis[:, None, :] * probs).sum(dim=2).argmax(dim=1)
        out.append(mus[torch.arange(mus.shape[0], device=O.device), :, idx])
    return torch.cat(out)


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


def bench_nll(dev, C, steps, warmup):
    gen = torch.Generator().manual_seed(1)
    O = torch.randn(B, 6 * C, generator=gen).to(dev)
    Y = ((torch.rand(B, 2, generator=gen) * 2 - 1) * torch.tensor([60.0, 170.0])).to(dev)

    def fused():
        M.nll_forward_backward(O, Y)

    def composed():
        Og = O.detach().requires_grad_(True)
        torch_nll(Og, Y, C).backward()

    d = alternate(fused, composed, steps, warmup, lambda f: device_ms(f, 10))
    w = alternate(fused, composed, steps, warmup, wall_ms)
    return {"what": "nll_fwd_bwd", "B": B, "C": C, "fused_device_ms": d[0], "torch_device_ms": d[1],
            "fused_wall_ms": w[0], "torch_wall_ms": w[1]}


def bench_predict(dev, C, steps, warmup):
    O = torch.randn(B, 6 * C, generator=torch.Generator().manual_seed(2)).to(dev)
    chunk = max(1, (1 << 25) // (C * C))  # [chunk, 2, C, C] float32 intermediates under 1 GB
    same = bool((M.mdn_predict(O, C) == torch_predict(O, C, chunk)).all(dim=1).float().mean() > 0.99)
    d = alternate(lambda: M.mdn_predict(O, C), lambda: torch_predict(O, C, chunk), steps, warmup,
                  lambda f: device_ms(f, 3))
    return {"what": "predict_mixture", "B": B, "C": C, "fused_device_ms": d[0],
            "torch_device_ms": d[1], "torch_rows_per_chunk": chunk, "agree_99pct": same}


def bench_step(dev, C, steps, warmup, F=10_000, nnz=64, n_batches=20):
    n = n_batches * B
    X = synthetic_features(n + B, F, nnz_per_row=nnz)
    rng = np.random.default_rng(3)
    Y = np.stack([rng.uniform(-60, 60, n + B), rng.uniform(-170, 170, n + B)], axis=1).astype(np.float32)
    out = {"what": "train_step", "B": B, "C": C, "F": F, "hid": HID, "nnz_per_row": nnz,
           "steps_per_epoch": n_batches}
    models = {}
    for name, drop in (("plain", False), ("dropout", True)):
        np.random.seed(0)
        clf = M.NNModel_lang2loc(n_epochs=0, batch_size=B, hid_size=HID, ncomp=C, drop_out=drop,
                                 device=dev)
        clf.fit(X[:n], Y[:n], X[n:], Y[n:])
        models[name] = clf
    times = {k: [] for k in models}
    for i in range(warmup + steps):
        order = rng.permutation(n)
        for name, clf in models.items():
            t = wall_ms(lambda: clf._train_epoch(order)) / n_batches
            if i >= warmup:
                times[name].append(t)
    for name in models:
        out[f"{name}_ms_per_step"] = med(times[name])
    return out


# -- the shared-component model (lang2loc_mdnshared.py) ----------------------------------------
def shared_inputs(dev, C, seed):
    """Logits, targets and the default initialisation's components (sigmas_raw in [10, 20])."""
    gen = torch.Generator().manual_seed(seed)
    span = torch.tensor([60.0, 170.0])
    L = torch.randn(B, C, generator=gen)
    Y = (torch.rand(B, 2, generator=gen) * 2 - 1) * span
    mus = (torch.rand(C, 2, generator=gen) * 2 - 1) * span
    sig = 10 + 10 * torch.rand(C, 2, generator=gen)
    cor = torch.randn(C, generator=gen)
    return tuple(t.to(dev) for t in (L, Y, mus, sig, cor))


def torch_shared_nll(L, Y, mus, sig, cor):
    """lang2loc_mdnshared.nll_loss_sharedparams, line by line (log pi as log_softmax)."""
    sigmas = torch.nn.functional.softplus(sig)
    corxy = torch.nn.functional.softsign(cor)
    diff = Y[:, None, :] - mus[None, :, :]
    sigmainvs = 1.0 / sigmas
    sigmainvprods = sigmainvs[:, 0] * sigmainvs[:, 1]
    z = (diff ** 2 / sigmas ** 2).sum(dim=-1) - 2 * corxy * diff[:, :, 0] * diff[:, :, 1] * sigmainvprods
    inv = 1.0 / (1.0 - corxy ** 2)
    e = math.log(0.5 / math.pi) + torch.log(sigmainvprods) + torch.log(torch.sqrt(inv)) + \
        -0.5 * z * inv + torch.log_softmax(L, dim=1)
    return -torch.logsumexp(e, dim=1).mean()


def bench_shared(dev, C, steps, warmup):
    L, Y, mus, sig, cor = shared_inputs(dev, C, 1)

    def fused():
        M.shared_nll_forward_backward(L, Y, mus, sig, cor)

    def composed():
        leaves = [t.detach().requires_grad_(True) for t in (L, mus, sig, cor)]
        torch_shared_nll(leaves[0], Y, *leaves[1:]).backward()

    d = alternate(fused, composed, steps, warmup, lambda f: device_ms(f, 10))
    w = alternate(fused, composed, steps, warmup, wall_ms)
    return {"what": "shared_nll_fwd_bwd", "B": B, "C": C, "fused_device_ms": d[0],
            "torch_device_ms": d[1], "fused_wall_ms": w[0], "torch_wall_ms": w[1]}


def bench_shared_predict(dev, C, steps, warmup):
    """pis . Dt and the arg-max, the C x C table given to both (it is per parameter set); the
    table's own time is reported beside them."""
    L, _, mus, sig, cor = shared_inputs(dev, C, 2)
    Dt = M.shared_density(mus, sig, cor)

    def fused():
        return M.shared_predict(L, mus, sig, cor, density=Dt)

    def composed():
        return mus[(torch.softmax(L, dim=1) @ Dt).argmax(dim=1)]

    same = bool((fused() == composed()).all(dim=1).float().mean() > 0.99)
    d = alternate(fused, composed, steps, warmup, lambda f: device_ms(f, 10))
    t, _ = alternate(lambda: M.shared_density(mus, sig, cor), lambda: None, steps, warmup,
                     lambda f: device_ms(f, 10))
    return {"what": "shared_predict_mixture", "B": B, "C": C, "fused_device_ms": d[0],
            "torch_device_ms": d[1], "density_table_device_ms": t, "agree_99pct": same}


def bench_shared_step(dev, C, steps, warmup, F=10_000, nnz=64, n_batches=20):
    """One NNModel_lang2locshared training step beside NNModel_lang2loc's, the same data."""
    n = n_batches * B
    X = synthetic_features(n + B, F, nnz_per_row=nnz)
    rng = np.random.default_rng(3)
    Y = np.stack([rng.uniform(-60, 60, n + B), rng.uniform(-170, 170, n + B)], axis=1).astype(np.float32)
    out = {"what": "shared_train_step", "B": B, "C": C, "F": F, "hid": HID, "nnz_per_row": nnz,
           "steps_per_epoch": n_batches}
    models = {}
    for name, cls, drop in (("shared_plain", M.NNModel_lang2locshared, False),
                            ("shared_dropout", M.NNModel_lang2locshared, True),
                            ("per_row_plain", M.NNModel_lang2loc, False)):
        np.random.seed(0)
        clf = cls(n_epochs=0, batch_size=B, hid_size=HID, ncomp=C, drop_out=drop, device=dev)
        clf.fit(X[:n], Y[:n], X[n:], Y[n:])
        models[name] = clf
    times = {k: [] for k in models}
    for i in range(warmup + steps):
        order = rng.permutation(n)
        for name, clf in models.items():
            t = wall_ms(lambda: clf._train_epoch(order)) / n_batches
            if i >= warmup:
                times[name].append(t)
    for name in models:
        out[f"{name}_ms_per_step"] = med(times[name])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--components", type=int, nargs="+", default=[100, 300, 900])
    ap.add_argument("--only", choices=["nll", "predict", "step", "shared", "shared_predict",
                                       "shared_step"], nargs="+",
                    default=["nll", "predict", "step"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (medians of 20)")
    dev = torch.device("cuda:0")
    benches = {"nll": bench_nll, "predict": bench_predict, "step": bench_step,
               "shared": bench_shared, "shared_predict": bench_shared_predict,
               "shared_step": bench_shared_step}
    for what in args.only:
        for C in args.components:
            line = json.dumps(benches[what](dev, C, args.steps, args.warmup))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
