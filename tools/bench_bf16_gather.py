#!/usr/bin/env python
"""H.Z with a float32 against a bfloat16 dense operand (sparse.spmm with a bfloat16 Z), timed in
alternating blocks on one device: the f32 SpMM, the bf16 SpMM alone per row stride, the bf16
SpMM plus its conversion pass (sparse.to_bf16_rows), and the conversion alone. HIP events, WARM
warm-up launches then REPS timed ones per block, ROUNDS interleaved rounds; one JSON line per
(graph, K) with every block's ms and the achieved bytes against the byte models

    f32 : 4 (N + 1) + 8 nnz + 4 K nnz + 4 K N
    bf16: 4 (N + 1) + 8 nnz + 2 K nnz + 4 K N      (+ 4 K N read, 2 ld N written by the conversion)

  python tools/bench_bf16_gather.py --config twitter-world --graphs powerlaw,uniform \
      --K 300 --strides 304,320 [--variant u16=tools/varlibs/libgcg_u16.so ...]

--variant NAME=LIB times the bf16 launch of another build of the library (tools/build_variant.py
with -DGCG_BF16_U_PLAN=.. -DGCG_BF16_U_ROW=.., or a patched kernel) on the same plan and
buffers, in the same rounds: the rows-in-flight and lane-layout A/Bs. --only-bf16 runs the bf16
launch alone (a counter pass)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphconvgeo_amd import _native, sparse as gs  # noqa: E402
from graphconvgeo_amd.synth import CONFIGS, synthetic_graph  # noqa: E402

WARM, REPS, ROUNDS = 3, 10, 3


def load_variant(path):
    lib = C.CDLL(path)
    for name in ("gcg_spmm_csr_bf16z_f32", "gcg_spmm_csr_bf16z_f32_planned"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _native.SIGNATURES[name]
    return lib


def bf16_launch(lib, A, Zb, out, mode):
    """sparse.spmm's bf16 dispatch through an explicit library (plans are plain device data)."""
    p, K = gs._ptr, Zb.shape[1]
    stream = gs._stream_handle(A.device)
    if mode == "rowwise":
        st = lib.gcg_spmm_csr_bf16z_f32(A.n_rows, A.n_cols, A.nnz, p(A.indptr), p(A.indices),
                                        p(A.data), p(Zb), Zb.stride(0), K, p(out), out.stride(0),
                                        None, 0, None, A.n_rows, None, 0, stream)
    else:
        plan = A.plan(None, ordered=gs.ORDERED_PLAN if mode == "ordered" else 0)
        ws = plan.workspace(K)
        hint = A.gather_hint(2 * min(Zb.stride(0), 512))
        st = lib.gcg_spmm_csr_bf16z_f32_planned(
            plan.handle, p(A.indptr), p(A.indices), p(A.data), p(Zb), Zb.stride(0), K, p(out),
            out.stride(0), None, 0, None, 0, p(ws), 0 if ws is None else ws.numel() * 4, p(hint),
            stream)
    if st != 0:
        raise RuntimeError(f"variant launch failed with status {st}")


def timed(fn):
    for _ in range(WARM):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return round(s.elapsed_time(e) / REPS, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="twitter-world", choices=sorted(CONFIGS))
    ap.add_argument("--graphs", default="powerlaw,uniform")
    ap.add_argument("--K", default="300")
    ap.add_argument("--strides", default="", help="bf16 row strides to compare (elements); "
                    "default: sparse.row_stride_bf16(K) alone")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIB")
    ap.add_argument("--only-bf16", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = CONFIGS[args.config]
    variants = {v.split("=", 1)[0]: load_variant(v.split("=", 1)[1]) for v in args.variant}
    for kind in args.graphs.split(","):
        H = synthetic_graph(cfg.n_nodes, cfg.n_edges, kind=kind)
        A = gs.DeviceCSR.from_scipy(H, dev, symmetric=True)
        n, nnz = H.shape[0], H.nnz
        del H
        mode = gs.resolve_auto(A)
        for K in (int(k) for k in args.K.split(",")):
            ld0 = gs.row_stride_bf16(K)
            strides = [int(x) for x in args.strides.split(",")] if args.strides else [ld0]
            src = gs.empty_dense(n, K, dev)
            src.copy_(torch.randn((n, K), device=dev))
            Y = gs.empty_dense(n, K, dev)
            Yb = gs.empty_dense(n, K, dev)
            zb = {}
            for ld in strides:
                buf = torch.empty((n, ld), dtype=torch.bfloat16, device=dev)
                zb[ld] = gs.to_bf16_rows(src, out=buf[:, :K] if ld != K else buf)
            blocks = {}
            if not args.only_bf16:
                blocks["f32"] = lambda: gs.spmm(A, src, out=Y, mode=mode)
                blocks["convert"] = lambda: gs.to_bf16_rows(src, out=zb[strides[0]])
            for ld in strides:
                blocks[f"bf16_ld{ld}"] = lambda ld=ld: gs.spmm(A, zb[ld], out=Yb, mode=mode)
            if not args.only_bf16:
                def both(ld=strides[0]):
                    gs.spmm(A, gs.to_bf16_rows(src, out=zb[ld]), out=Yb, mode=mode)
                blocks[f"bf16_ld{strides[0]}_plus_convert"] = both
            for name, lib in variants.items():
                blocks[f"bf16_ld{strides[0]}_{name}"] = \
                    lambda lib=lib: bf16_launch(lib, A, zb[strides[0]], Yb, mode)
            # every bf16 block computes the same bits
            ref = gs.spmm(A, zb[strides[0]], mode=mode)
            for name, fn in blocks.items():
                if name.startswith("bf16"):
                    Yb.zero_()
                    fn()
                    assert torch.equal(Yb, ref), f"{name} changed the result"
            res = {name: [] for name in blocks}
            for _ in range(ROUNDS):
                for name, fn in blocks.items():
                    res[name].append(timed(fn))
            b32 = 4 * (n + 1) + 8 * nnz + 4 * K * nnz + 4 * K * n
            b16 = 4 * (n + 1) + 8 * nnz + 2 * K * nnz + 4 * K * n
            rec = {"config": cfg.name, "graph": kind, "mode": mode, "K": K, "nodes": n, "nnz": nnz,
                   "row_stride_bf16": ld0, "row_stride_f32": src.stride(0), "ms": res,
                   "bytes_f32_model": b32, "bytes_bf16_model": b16,
                   "gather_hint_rows": getattr(A, "_hint_hot_rows", None),
                   "GBps": {k: round((b16 if k.startswith("bf16") else b32) / min(v) / 1e6, 1)
                            for k, v in res.items() if k != "convert"},
                   "convert_GBps": round((4 * K * n + 2 * strides[0] * n) / min(res["convert"])
                                         / 1e6, 1) if "convert" in res else None,
                   "warm": WARM, "reps": REPS, "rounds": ROUNDS}
            print(json.dumps(rec), flush=True)
            del src, Y, Yb, zb, ref, blocks
            torch.cuda.empty_cache()
        del A


if __name__ == "__main__":
    main()
