"""Dense side of the output layer on the MI355X matrix cores (host mirror of T.dot + softmax +
categorical_crossentropy).

Reference (Theano, host BLAS / CPU):
    ConvolutionDenseLayer.get_output_for   T.dot(h, W), (... + b), softmax   mlpconv.py:86-95
    MLPCONV loss / accuracy                categorical_crossentropy(out, y).mean(),
                                           T.mean(T.eq(out.argmax(-1), y))    mlpconv.py:227-253
    predict_proba                          softmax rows                       mlpconv.py:329-335

Here every product runs in libgcg_spmm.so's MFMA kernels (csrc/dense_*.hip):
  matmul(A, W)                    C = A . W          gcg_gemm_nt on W^T (grad A: g . W^T,
                                  the same kernel on W); grad W on gemm_tn
  gemm(A, B) / gemm_nt(A, Bt)     the plain products (register-B / LDS-DMA kernels)
  project_softmax_xent(P, W, b, y)  loss, acc of softmax(P . W + b) against y, one fused
                                  kernel that never writes the logits; its gradient
                                  (softmax - onehot)/T is produced in the same pass
  softmax_xent(logits, y)         loss, acc of logits that already exist (reference order)
  softmax(logits)                 predict_proba
  gemm_tn(A, B)                   C = A^T . B, the weight gradient h^T . g: a split-K MFMA kernel
                                  (reduction over ~10^6 rows; bf16x6 by default, TN_MATH),
                                  deterministic
No product of the layer path goes to hipBLASLt / rocBLAS. There is no CPU path: CPU tensors
raise. Round 4: gemm_nt (NT_MATH) and the fused layer (FUSED_MATH) run their products on the
bf16 matrix cores at f32 accuracy -- every f32 operand split into three bf16 planes, the six
plane products of order <= 2^-16 accumulated in f32 ("bf16x6"; error against float64 at or
below the f32 MFMA kernels', tests/test_dense_gpu.py; a tile whose result is not finite is
recomputed on the f32 MFMA, so Inf / NaN follow f32 semantics); gemm_tn stays on the f32 MFMA.
Round 5: the arithmetic and the tile are arguments of every C call (gcg_gemm_nt,
gcg_project_softmax_xent, gcg_gemm, gcg_gemm_tn: `math`, `tile`), never the environment.
"""
from __future__ import annotations

from typing import Optional, Tuple

import ctypes as C

import torch

from . import ops as _ops  # registers torch.ops.gcg.* (the compiled path)
from ._native import GCG_ACT_NONE, GCG_ACT_RELU, call, device_scalar, load
# _colsum: the bias gradients' column sums (sparse.colsum), under the name this module uses
from .sparse import _ptr, _require_cuda, _stream_handle, colsum as _colsum, empty_dense

MATHS = {"f32": 0, "bf16x6": 1}  # gcg_spmm.h GCG_MATH_F32 / GCG_MATH_BF16X6


def _math_code(math: str) -> int:
    if math not in MATHS:
        raise ValueError(f"math must be one of {tuple(MATHS)}")
    return MATHS[math]


def tile_count(op: str, math: str = "f32") -> int:
    """Alternative tiles (indices 1..n) of product op ("gemm", "gemm_nt", "fused", "gemm_tn")
    in arithmetic `math` (gcg_dense_tile_count; -1 when the arithmetic does not exist there)."""
    ops = {"gemm": 0, "gemm_nt": 1, "fused": 2, "gemm_tn": 3}
    return int(load().gcg_dense_tile_count(ops[op], _math_code(math)))


_WS_SIZES: dict = {}


def _ws_bytes(fn: str, N: int, K: int, math: int) -> int:
    """Workspace bytes of a bf16x6 entry (cached per shape: a host call per step otherwise)."""
    key = (fn, N, K, math)
    nb = _WS_SIZES.get(key)
    if nb is None:
        nb = _WS_SIZES[key] = int(getattr(load(), fn)(N, K, math))
    return nb


FUSED_MAX_COLS = 1024
ROWS_MAX_COLS = 4096


def _ld(t: torch.Tensor) -> int:
    """Row stride in elements; a single row's stride is never used, so report round4(cols)."""
    return t.stride(0) if t.shape[0] > 1 else (max(t.shape[1], 1) + 3) // 4 * 4


def _aligned_operand(t: torch.Tensor, name: str) -> torch.Tensor:
    """A row-major fp32 operand with a 16-B aligned base and ld % 4 == 0 (copied if not)."""
    _require_cuda(t, name)
    if t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError(f"{name} must be a 2-D float32 tensor")
    ok = (t.shape[1] <= 1 or t.stride(1) == 1) and _ld(t) % 4 == 0 and t.data_ptr() % 16 == 0
    if ok:
        return t
    out = empty_dense(t.shape[0], t.shape[1], t.device)
    out.copy_(t)
    return out


class _WeightCache:
    """Padded [K, round4(N)] (or transposed [N, round4(K)]) copy of a weight, rebuilt only
    when the parameter changes (its in-place version counter moves, e.g. after Adam)."""

    def __init__(self):
        self._key = None
        self._buf = None

    def get(self, W: torch.Tensor, transpose: bool, scale: Optional[torch.Tensor] = None):
        key = (W.data_ptr(), W._version, tuple(W.shape), transpose)
        capturing = torch.cuda.is_current_stream_capturing()
        if scale is None and key == self._key and not capturing:
            return self._buf  # a captured graph always re-copies: W moves between replays
        src = W.detach().t() if transpose else W.detach()
        rows, cols = src.shape
        if self._buf is None or self._buf.shape != (rows, cols) or self._buf.device != W.device:
            ldp = (cols + 3) // 4 * 4
            full = torch.zeros((rows, ldp), dtype=torch.float32, device=W.device)
            self._buf = full[:, :cols]
        if scale is not None:
            torch.mul(src, scale, out=self._buf)
            self._key = None
        else:
            self._buf.copy_(src)
            # A copy recorded into a graph runs at every replay, before that replay's Adam
            # update, while W._version never moves on a replay: a key stored here would let
            # the next eager call reuse a copy one update behind. Forget it instead.
            self._key = None if capturing else key
        return self._buf


def gemm(A: torch.Tensor, B: torch.Tensor, bias: Optional[torch.Tensor] = None,
         act: Optional[str] = None, out: Optional[torch.Tensor] = None,
         tile: int = 0) -> torch.Tensor:
    """C = act(A . B + bias) on the MFMA kernel (gcg_gemm, f32; tile 0: B through LDS, 1: B
    straight to registers -- bitwise equal). B must have ld >= round4(N) (see _WeightCache); A
    is copied to an aligned buffer if its rows are not 16-B aligned."""
    A = _aligned_operand(A, "A")
    _require_cuda(B, "B")
    M, K = A.shape
    if B.dim() != 2 or B.shape[0] != K:
        raise ValueError(f"shape mismatch: A is {tuple(A.shape)}, B is {tuple(B.shape)}")
    N = B.shape[1]
    if B.dtype != torch.float32 or (N > 1 and B.stride(1) != 1):
        raise TypeError("B must be float32 with unit column stride")
    ldb = B.stride(0)
    if ldb < (N + 3) // 4 * 4 or ldb % 4 or B.data_ptr() % 16:
        raise ValueError("B needs ld >= round4(N), ld % 4 == 0 and a 16-B aligned base")
    if bias is not None:
        _require_cuda(bias, "bias")
        if bias.numel() != N or bias.dtype != torch.float32:
            raise ValueError(f"bias must be float32[{N}]")
        bias = bias.contiguous()
    if out is None:
        out = empty_dense(M, N, A.device)
    elif out.shape != (M, N) or out.dtype != torch.float32 or (N > 1 and out.stride(1) != 1):
        raise ValueError(f"out must be float32 [{M}, {N}] with unit column stride")
    if M == 0:
        return out
    actc = {None: GCG_ACT_NONE, "relu": GCG_ACT_RELU, "rectify": GCG_ACT_RELU}[act]
    with torch.cuda.device(A.device):
        call("gcg_gemm", M, N, K, _ptr(A), _ld(A), _ptr(B), ldb, _ptr(bias), actc,
             _ptr(out), _ld(out), MATHS["f32"], int(tile), _stream_handle(A.device))
    return out


# gemm_nt's default products: "bf16x6" (round 4: f32 operands split into three bf16 planes on
# the bf16 matrix cores, error against float64 at or below the f32 MFMA kernel's,
# tests/test_dense_gpu.py; 170-179 vs 113-119 TFLOP/s at Twitter-World's shapes) or "f32"
# (v_mfma_f32_16x16x4_f32).
NT_MATH = "bf16x6"
NT_MATHS = ("f32", "bf16x6", "bf16x6_inloop")


def gemm_nt(A: torch.Tensor, Bt: torch.Tensor, bias: Optional[torch.Tensor] = None,
            act: Optional[str] = None, out: Optional[torch.Tensor] = None,
            math: Optional[str] = None, tile: int = 0) -> torch.Tensor:
    """C = act(A . Bt^T + bias) on the MFMA NT kernels (gcg_gemm_nt): both operands
    k-contiguous, 16-B aligned rows (A: M x K, Bt: N x K). The weight side is a transposed
    padded copy (_WeightCache(transpose=True)) for A . W, or W itself (padded) for g . W^T.
    math: "f32" (v_mfma_f32_16x16x4_f32) or "bf16x6" (gcg_gemm_nt_f32_bf16x6: f32-accurate
    products from three bf16 planes per operand on the bf16 matrix cores, Bt's planes split
    once into a workspace; "bf16x6_inloop" splits both operands in the loop); None: NT_MATH.
    tile: 0 = the default for the shape, 1..tile_count("gemm_nt", math) a measured alternative."""
    math = math or NT_MATH
    if math not in NT_MATHS:
        raise ValueError(f"math must be one of {NT_MATHS}")
    A = _aligned_operand(A, "A")
    Bt = _aligned_operand(Bt, "Bt")
    M, K = A.shape
    N = Bt.shape[0]
    if Bt.shape[1] != K:
        raise ValueError(f"shape mismatch: A is {tuple(A.shape)}, Bt is {tuple(Bt.shape)}")
    for t, n in ((A, "A"), (Bt, "Bt")):
        if t.shape[0] > 1 and _ld(t) < (K + 3) // 4 * 4:
            raise ValueError(f"{n} needs a row stride >= round4(K) (empty_dense)")
    if bias is not None:
        _require_cuda(bias, "bias")
        if bias.numel() != N or bias.dtype != torch.float32:
            raise ValueError(f"bias must be float32[{N}]")
        bias = bias.detach().contiguous()
    if out is None:
        out = empty_dense(M, N, A.device)
    elif out.shape != (M, N) or out.dtype != torch.float32 or (N > 1 and out.stride(1) != 1):
        raise ValueError(f"out must be float32 [{M}, {N}] with unit column stride")
    if M == 0:
        return out
    actc = {None: GCG_ACT_NONE, "relu": GCG_ACT_RELU, "rectify": GCG_ACT_RELU}[act]
    code = MATHS["f32" if math == "f32" else "bf16x6"]
    ws, nb = None, 0
    if math == "bf16x6":  # Bt's planes split once per call into a workspace (stream-ordered)
        nb = _ws_bytes("gcg_gemm_nt_workspace", N, K, code)
        ws = torch.empty(nb, dtype=torch.uint8, device=A.device)
    with torch.cuda.device(A.device):
        call("gcg_gemm_nt", M, N, K, _ptr(A), _ld(A), _ptr(Bt), _ld(Bt), _ptr(bias), actc,
             _ptr(out), _ld(out), code, int(tile), _ptr(ws), nb, _stream_handle(A.device))
    return out


_TN_WS: dict = {}


# products of gemm_tn (the weight gradients): "f32" or "bf16x6" (round 6, gemm_tn6_partial_kernel:
# World dW2 840k x 300 x 930 124.7-126.9 -> 140.6-143.5 TFLOP/s, the X-head gradient 1.4M x 256 x
# 300 104-111 -> 139, Twitter-US dW2 98-108 -> 119-126, each closer to float64 than the f32
# kernel: tools/exp_tn_math.py, profiles/r06/tn_math_ab.jsonl)
TN_MATH = "bf16x6"


def gemm_tn(A: torch.Tensor, B: torch.Tensor, scale: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None, tile: int = 0, math: Optional[str] = None
            ) -> torch.Tensor:
    """C = scale * A^T . B (the weight gradient h^T . g) on the split-K MFMA kernel (gcg_gemm_tn);
    deterministic (partials summed in a fixed order). scale: optional device scalar.
    math: "f32" (f32 MFMA) or "bf16x6" (the bf16 matrix cores, f32-accurate; tile 0 only);
    None = TN_MATH at tile 0, f32 at another tile. tile: 0 = the default layout for the shape, 1..tile_count("gemm_tn") another
    one (f32)."""
    if math is None:  # (the alternative tiles are f32 layouts)
        math = "f32" if tile else TN_MATH
    A = _aligned_operand(A, "A")
    B = _aligned_operand(B, "B")
    R, M = A.shape
    if B.shape[0] != R:
        raise ValueError(f"shape mismatch: A is {tuple(A.shape)}, B is {tuple(B.shape)}")
    N = B.shape[1]
    for t, n, cols in ((A, "A", M), (B, "B", N)):
        if R > 1 and _ld(t) < (cols + 3) // 4 * 4:
            t2 = empty_dense(R, cols, t.device)  # row stride must cover round4(cols)
            t2.copy_(t)
            if n == "A":
                A = t2
            else:
                B = t2
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    if R == 0:
        return out.zero_()
    nb = C.c_size_t()
    call("gcg_gemm_tn_workspace_bytes", R, M, N, _math_code(math), int(tile), C.byref(nb))
    key = (A.device, torch.cuda.current_stream(A.device).cuda_stream)
    ws = _TN_WS.get(key)
    if ws is None or ws.numel() * 4 < nb.value:
        ws = torch.empty(max((nb.value + 15) // 16 * 4, 4), dtype=torch.float32, device=A.device)
        _TN_WS[key] = ws
    scale = device_scalar(scale)
    with torch.cuda.device(A.device):
        call("gcg_gemm_tn", R, M, N, _ptr(A), _ld(A), _ptr(B), _ld(B), _ptr(scale),
             _ptr(out), out.stride(0) if M > 1 else N, _math_code(math), int(tile), _ptr(ws),
             ws.numel() * 4, _stream_handle(A.device))
    return out


# -- weight gradients on a side stream -------------------------------------------------------
# A weight gradient (A^T . G, MFMA-bound) has no consumer until the optimizer, while the rest
# of the backward is a chain of HBM-bound CSR gathers: the two overlap on the GPU when the
# weight gradient runs on its own stream. The autograd engine runs each backward on the
# stream its forward ran on, so W enters the consumer through an identity node created on the
# side stream; the consumer's backward leaves (A, G, scale) in a slot and hands the identity
# node a placeholder; the identity node's backward computes the gradient on the side stream.
# The engine joins the streams (event waits) where gradients cross and at the end of
# backward() -- also inside a HIP graph capture. A and G are marked used by the side stream
# (record_stream) before the kernel reads them, so the caching allocator does not recycle them
# for the main stream while it runs, whenever the autograd graph is freed.
_SIDE_STREAMS: dict = {}
SIDE_STREAM_WEIGHT_GRADS = True


# priority of the side stream (torch: lower = higher priority; 0 = the default's)
SIDE_STREAM_PRIORITY = 0


def _side_stream(device) -> torch.cuda.Stream:
    s = _SIDE_STREAMS.get(device)
    if s is None:
        s = torch.cuda.Stream(device=device, priority=SIDE_STREAM_PRIORITY)
        _SIDE_STREAMS[device] = s
    return s


class _Slot:
    __slots__ = ("args",)

    def __init__(self):
        self.args = None


class _SideWeightGrad(torch.autograd.Function):
    """Identity on W; its backward computes scale * A^T . G (gemm_tn) from the slot."""

    @staticmethod
    def forward(ctx, W, slot):
        ctx.slot = slot
        return W.view_as(W)

    @staticmethod
    def backward(ctx, _placeholder):
        if ctx.slot.args is None:  # the consumer produced no weight gradient
            return None, None
        A, G, scale = ctx.slot.args
        ctx.slot.args = None
        # A and G were allocated on the main stream and are read here on the side stream:
        # tell the caching allocator, so their blocks are not handed to a main-stream
        # allocation before this kernel has finished, whenever the autograd graph lets go
        side = torch.cuda.current_stream(A.device)
        for t in (A, G, scale):
            if t is not None:
                t.record_stream(side)
        return gemm_tn(A, G, scale=scale), None


def _weight_on_side_stream(W: torch.Tensor):
    """(W', slot): W' aliases W; the gradient reaching W' is computed on a side stream."""
    if not (SIDE_STREAM_WEIGHT_GRADS and torch.is_grad_enabled() and W.requires_grad
            and W.is_cuda):
        return W, None
    slot = _Slot()
    W._gcg_side_grad = True  # l1l2_penalty puts this weight's penalty node on the side stream
    with torch.cuda.stream(_side_stream(W.device)):
        Wa = _SideWeightGrad.apply(W, slot)
    return Wa, slot


class _SideBiasGrad(torch.autograd.Function):
    """Identity on b; its backward computes scale * colsum(G) from the slot (round 6: the
    output layer's bias gradient, a 2 GB column pass at Twitter-World, leaves the main stream's
    critical path and runs beside the input gradient's GEMM)."""

    @staticmethod
    def forward(ctx, b, slot):
        ctx.slot = slot
        return b.view_as(b)

    @staticmethod
    def backward(ctx, _placeholder):
        if ctx.slot.args is None:  # the consumer produced no bias gradient
            return None, None
        G, scale = ctx.slot.args
        ctx.slot.args = None
        side = torch.cuda.current_stream(G.device)
        for t in (G, scale):  # main-stream memory read on the side stream (as _SideWeightGrad)
            t.record_stream(side)
        return _colsum(G).mul_(scale), None


def _bias_on_side_stream(b: Optional[torch.Tensor]):
    """(b', slot): b' aliases b; the gradient reaching b' is computed on the side stream."""
    if b is None or not (SIDE_STREAM_WEIGHT_GRADS and torch.is_grad_enabled() and b.requires_grad
                         and b.is_cuda):
        return b, None
    slot = _Slot()
    with torch.cuda.stream(_side_stream(b.device)):
        ba = _SideBiasGrad.apply(b, slot)
    return ba, slot


def _placeholder_grad(W: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """A W-shaped gradient that costs no kernel (the real one is computed from the slot)."""
    return like.new_empty(()).expand(W.shape)


class _MatMul(torch.autograd.Function):
    """C = A . W (+ b) (T.dot(h, W), mlpconv.py:88) and its gradients, every product on the
    hand-written MFMA kernels: forward C = A . (W^T)^T and the input gradient
    dA = g . W^T on the LDS-DMA NT GEMM (gemm_nt; W^T / W kept as padded copies in the
    weight's Projection, re-copied when Adam moves W), the weight gradient dW = A^T . g -- a
    reduction over ~10^6 rows into K x C -- on the split-K kernel (gemm_tn)."""

    @staticmethod
    def forward(ctx, A, W, b, slot=None, proj=None):
        proj = proj or Projection()
        C = gemm_nt(A, proj.fwd.get(W, True), bias=b)
        ctx.save_for_backward(A, W)
        ctx.has_b = b is not None
        ctx.slot = slot
        ctx.proj = proj
        return C

    @staticmethod
    def backward(ctx, g):
        A, W = ctx.saved_tensors
        gA = gW = gb = None
        if ctx.has_b and ctx.needs_input_grad[2]:
            gb = _colsum(g)
        if ctx.needs_input_grad[1]:
            if ctx.slot is not None:  # computed on the side stream (_SideWeightGrad)
                ctx.slot.args = (A, g, None)
                gW = _placeholder_grad(W, g)
            else:
                gW = gemm_tn(A, g)
        if ctx.needs_input_grad[0]:
            gA = gemm_nt(g, ctx.proj.bwd.get(W, False))  # g . W^T: Bt = W (padded K x round4(N))
        return gA, gW, gb, None, None


def projection_of(W: torch.Tensor) -> "Projection":
    """The padded-copy cache of a weight, kept on the weight tensor itself (one per weight)."""
    proj = getattr(W, "_gcg_projection", None)
    if proj is None:
        proj = Projection()
        W._gcg_projection = proj
    return proj


def matmul(A: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable A . W (+ b) on the MFMA kernels (forward and input gradient: gemm_nt;
    weight gradient: gemm_tn on a side stream, overlapping the rest of the backward)."""
    if torch.compiler.is_compiling():  # the registered op gcg::dense_matmul (ops.py)
        return _ops.dense_matmul(A, W, b)
    proj = projection_of(W)
    Wa, slot = _weight_on_side_stream(W)
    return _MatMul.apply(A, Wa, b, slot, proj)


class Projection:
    """Holds the padded weight copies of one dense weight W (K x C) for the MFMA kernels."""

    def __init__(self):
        self.fwd = _WeightCache()
        self.bwd = _WeightCache()

    def invalidate(self):
        """Forget the cached copies: W changed without its version counter moving (a graph
        replay's in-place Adam update)."""
        self.fwd._key = None
        self.bwd._key = None

    def matmul(self, A: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor] = None
               ) -> torch.Tensor:
        if torch.compiler.is_compiling():
            return _ops.dense_matmul(A, W, b)
        Wa, slot = _weight_on_side_stream(W)
        return _MatMul.apply(A, Wa, b, slot, self)

    def softmax_xent(self, P, W, b, labels, denom: Optional[int] = None,
                     row_weight: Optional[torch.Tensor] = None):
        """row_weight: optional float32 [M] multiplicity of each row (distinct targets of a
        list drawn with replacement); denom is then the length of the full list."""
        row_weight = _row_weight(row_weight, P.shape[0])
        if torch.compiler.is_compiling():  # gcg::project_softmax_xent (ops.py)
            return _ops.project_softmax_xent(P, W, b, labels, denom, row_weight)
        if not torch.is_grad_enabled():  # evaluation: loss and hits only, no gradient buffer
            P = _aligned_operand(P, "P")
            M = P.shape[0]
            D = float(max(M if denom is None else denom, 1))
            y = _labels_i32(labels, M, W.shape[1])
            loss_rows = torch.empty(M, dtype=torch.float32, device=P.device)
            correct = torch.empty(M, dtype=torch.float32, device=P.device)
            _fused(P, self.fwd.get(W, False), b, y, 1.0, None, None, loss_rows, correct,
                   row_weight)
            return loss_rows.sum() / D, correct.sum() / D
        Wa, slot = _weight_on_side_stream(W)
        ba, bslot = _bias_on_side_stream(b)
        return _ProjectXent.apply(P, Wa, ba, labels, self, denom, slot, row_weight, bslot)

    def probabilities(self, P, W, b) -> torch.Tensor:
        """softmax(P . W + b) rows (predict_proba) in one fused launch."""
        P = _aligned_operand(P, "P")
        M = P.shape[0]
        out = empty_dense(M, W.shape[1], P.device)
        _fused(P, self.fwd.get(W, False), b, None, 1.0, None, out, None, None)
        return out


def _labels_i32(labels: torch.Tensor, M: int, N: int) -> torch.Tensor:
    """int32 device labels. Their range is not checked here (that would synchronize, and the
    call sits inside captured graphs): the kernels give a row whose label is outside [0, N)
    a NaN loss, so the mean loss turns NaN instead of silently using a wrong class, and
    MLPCONV.fit checks the host labels once."""
    _require_cuda(labels, "labels")
    if labels.numel() != M:
        raise ValueError(f"labels has {labels.numel()} entries for {M} rows")
    return labels.to(torch.int32).contiguous()


def _row_weight(w: Optional[torch.Tensor], M: int) -> Optional[torch.Tensor]:
    if w is None:
        return None
    _require_cuda(w, "row_weight")
    if w.numel() != M:
        raise ValueError(f"row_weight has {w.numel()} entries for {M} rows")
    return w.detach().to(torch.float32).contiguous()


# The fused layer's default arithmetic (gcg_project_softmax_xent `math`): "bf16x6" (f32-accurate
# products on the bf16 matrix cores) or "f32" (v_mfma_f32_16x16x4_f32).
FUSED_MATH = "bf16x6"
# bf16x6: W's planes pre-split once per call into a workspace laid out for coalesced loads
# (FX = 1) instead of split in every workgroup's registers; at N > 768 on a 64-row tile -- World
# 840k x 300 x 930 140-147.5 vs 121-128 TFLOP/s f32-equivalent (tools/exp_fused_compose.py,
# test_fused6_row_bands_bitwise)
FUSED_PRESPLIT = True


def _fused(P, Wp, b, labels, scale, scale_dev, out, loss_rows, correct, row_weight=None,
           math: Optional[str] = None, tile: int = 0):
    """gcg_project_softmax_xent with an explicit arithmetic (None: FUSED_MATH) and tile."""
    math = math or FUSED_MATH
    code = _math_code(math)
    P = _aligned_operand(P, "P")
    M, K = P.shape
    N = Wp.shape[1]
    if Wp.shape[0] != K:
        raise ValueError(f"shape mismatch: P is {tuple(P.shape)}, W is {tuple(Wp.shape)}")
    if N > FUSED_MAX_COLS:
        raise ValueError(f"fused softmax projection supports up to {FUSED_MAX_COLS} classes")
    if b is not None:
        _require_cuda(b, "b")
        b = b.detach().contiguous()
    if M == 0:
        return
    ws, nb = None, 0
    if math == "bf16x6" and FUSED_PRESPLIT:  # the weight's bf16 planes, split once per call
        nb = _ws_bytes("gcg_project_softmax_xent_workspace", N, K, code)
        ws = torch.empty(nb, dtype=torch.uint8, device=P.device)
    with torch.cuda.device(P.device):
        call("gcg_project_softmax_xent", M, N, K, _ptr(P), _ld(P), _ptr(Wp), Wp.stride(0),
             _ptr(b), _ptr(labels), float(scale), _ptr(scale_dev), _ptr(out),
             _ld(out) if out is not None else 0, _ptr(loss_rows), _ptr(correct),
             _ptr(row_weight), code, int(tile), _ptr(ws), nb, _stream_handle(P.device))


class _ProjectXent(torch.autograd.Function):
    """(loss, acc) = mean CE / accuracy of softmax(P . W + b) against labels.

    Forward: one fused MFMA launch writes G = (softmax - onehot)/M (the logits gradient),
    per-row losses and hits; no logits in HBM. Backward (upstream g, a device scalar):
    dP = G . (g W)^T (NT MFMA gemm_nt), dW = g P^T . G (split-K MFMA gemm_tn), db = g colsum(G)."""

    @staticmethod
    def forward(ctx, P, W, b, labels, proj: Projection, denom: Optional[int] = None, slot=None,
                row_weight=None, bslot=None):
        P = _aligned_operand(P, "P")
        M, N = P.shape[0], W.shape[1]
        D = float(max(M if denom is None else denom, 1))  # rows the mean is over (all ranks)
        y = _labels_i32(labels, M, N)
        need_grad = any(ctx.needs_input_grad[:3])
        G = empty_dense(M, N, P.device) if need_grad else None
        loss_rows = torch.empty(M, dtype=torch.float32, device=P.device)
        correct = torch.empty(M, dtype=torch.float32, device=P.device)
        _fused(P, proj.fwd.get(W, False), b, y, 1.0 / D, None, G, loss_rows, correct, row_weight)
        ctx.save_for_backward(P, W, G)
        ctx.proj = proj
        ctx.slot = slot
        ctx.bslot = bslot
        ctx.has_b = b is not None
        ctx.b_shape = b.shape if b is not None else None
        loss = loss_rows.sum() / D
        acc = correct.sum() / D
        ctx.mark_non_differentiable(acc)
        return loss, acc

    @staticmethod
    def backward(ctx, g_loss, _g_acc):
        P, W, G = ctx.saved_tensors
        gP = gW = gb = None
        g = g_loss.reshape(())
        if ctx.has_b and ctx.needs_input_grad[2]:
            if ctx.bslot is not None:  # on the side stream (_bias_on_side_stream)
                ctx.bslot.args = (G, g)
                gb = g.new_empty(()).expand(ctx.b_shape)
            else:
                gb = _colsum(G).mul_(g)
        if ctx.needs_input_grad[1]:
            # split-K MFMA, the upstream gradient applied on device; on the side stream when
            # W came through _weight_on_side_stream
            if ctx.slot is not None:
                ctx.slot.args = (P, G, g)
                gW = _placeholder_grad(W, g)
            else:
                gW = gemm_tn(P, G, scale=g)
        if ctx.needs_input_grad[0]:
            # dP = G . (g W)^T on the NT GEMM: Bt = g W, a scaled padded copy of W
            gP = gemm_nt(G, ctx.proj.bwd.get(W, False, scale=g))
        return gP, gW, gb, None, None, None, None, None, None


def _rows_call(logits, y, scale, scale_dev, out, loss_rows, correct, row_weight=None):
    M, N = logits.shape
    if N > ROWS_MAX_COLS:
        raise ValueError(f"softmax_xent supports up to {ROWS_MAX_COLS} classes")
    if M == 0:
        return
    with torch.cuda.device(logits.device):
        call("gcg_softmax_xent_weighted_f32", M, N, _ptr(logits), _ld(logits), _ptr(y),
             float(scale), _ptr(scale_dev), _ptr(out), _ld(out) if out is not None else 0,
             _ptr(loss_rows), _ptr(correct), _ptr(row_weight), _stream_handle(logits.device))


class _SoftmaxXent(torch.autograd.Function):
    """(loss, acc) of logits that exist (the reference order: logits = (H . Z2 + b)[idx]).
    Forward reads the logits once (loss and hits only); backward writes
    g (softmax - onehot)/M in one more pass, g read on the device (graph-capturable)."""

    @staticmethod
    def forward(ctx, logits, labels, denom: Optional[int] = None, row_weight=None):
        _require_cuda(logits, "logits")
        if logits.dtype != torch.float32 or logits.dim() != 2 or \
                (logits.shape[1] > 1 and logits.stride(1) != 1):
            raise TypeError("logits must be 2-D float32 with unit column stride")
        M, N = logits.shape
        y = _labels_i32(labels, M, N)
        loss_rows = torch.empty(M, dtype=torch.float32, device=logits.device)
        correct = torch.empty(M, dtype=torch.float32, device=logits.device)
        _rows_call(logits, y, 1.0, None, None, loss_rows, correct, row_weight)
        ctx.row_weight = row_weight
        ctx.save_for_backward(logits, y)
        ctx.D = float(max(M if denom is None else denom, 1))
        acc = correct.sum() / ctx.D
        ctx.mark_non_differentiable(acc)
        return loss_rows.sum() / ctx.D, acc

    @staticmethod
    def backward(ctx, g_loss, _g_acc):
        logits, y = ctx.saved_tensors
        M, N = logits.shape
        gl = empty_dense(M, N, logits.device)
        dummy = torch.empty(M, dtype=torch.float32, device=logits.device)
        g = device_scalar(g_loss)
        _rows_call(logits, y, 1.0 / ctx.D, g, gl, dummy, None, ctx.row_weight)
        return gl, None, None, None


def project_softmax_xent(P, W, b, labels, proj: Optional[Projection] = None,
                         denom: Optional[int] = None, row_weight: Optional[torch.Tensor] = None
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean CE loss, accuracy) of softmax(P . W + b) against labels, differentiable in P, W, b.
    denom: the row count the mean is taken over (default: these rows; the total over all
    ranks when each rank holds a share of the targets). row_weight: optional multiplicity of
    each row (every row's loss, hit and gradient scaled by it)."""
    if torch.compiler.is_compiling():  # gcg::project_softmax_xent (ops.py)
        return _ops.project_softmax_xent(P, W, b, labels, denom, _row_weight(row_weight, P.shape[0]))
    Wa, slot = _weight_on_side_stream(W)
    ba, bslot = _bias_on_side_stream(b)
    return _ProjectXent.apply(P, Wa, ba, labels, proj or Projection(), denom, slot,
                              _row_weight(row_weight, P.shape[0]), bslot)


def softmax_xent(logits: torch.Tensor, labels: torch.Tensor, denom: Optional[int] = None,
                 row_weight: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean CE loss, accuracy) of existing logits, differentiable in the logits;
    row_weight as in project_softmax_xent."""
    return _SoftmaxXent.apply(logits, labels, denom, _row_weight(row_weight, logits.shape[0]))


L1L2_WORKSPACE_BYTES = 2048  # GCG_L1L2_WORKSPACE_BYTES


class _L1L2Penalty(torch.autograd.Function):
    """acc + sum_i l1_i * sum|W_i| + l2_i * sum W_i^2, added up in the order of the weights: one
    launch pair per weight forward (gcg_l1l2_penalty_f32), one launch per weight backward
    (gcg_l1l2_grad_f32, the upstream gradient read on the device), instead of ~20 elementwise
    and reduction torch kernels for the penalty and its gradient per training step. `acc` (a
    device scalar or None) is the running sum of the previous weights' node."""

    @staticmethod
    def forward(ctx, coefs, acc, *weights):
        dev = weights[0].device
        out = torch.empty((), dtype=torch.float32, device=dev)
        ws = torch.empty(L1L2_WORKSPACE_BYTES // 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            for W, (l1, l2) in zip(weights, coefs):
                call("gcg_l1l2_penalty_f32", W.numel(), _ptr(W), float(l1), float(l2), _ptr(acc),
                     _ptr(out), _ptr(ws), L1L2_WORKSPACE_BYTES, _stream_handle(dev))
                acc = out
        ctx.coefs = coefs
        ctx.save_for_backward(*weights)
        return out

    @staticmethod
    def backward(ctx, g):
        g_acc = g if ctx.needs_input_grad[1] else None
        g = device_scalar(g)
        grads = []
        for i, (W, (l1, l2)) in enumerate(zip(ctx.saved_tensors, ctx.coefs)):
            if not ctx.needs_input_grad[2 + i]:
                grads.append(None)
                continue
            dW = torch.empty_like(W)
            with torch.cuda.device(W.device):
                call("gcg_l1l2_grad_f32", W.numel(), _ptr(W), float(l1), float(l2), _ptr(g),
                     _ptr(dW), _stream_handle(W.device))
            grads.append(dW)
        return (None, g_acc, *grads)


def l1l2_penalty(weights, coefs) -> torch.Tensor:
    """The MLPCONV weight penalty (mlpconv.py:235-243): sum over the weights, in the given
    order, of l1 * sum|W| + l2 * sum W^2 (l1 = regul_coef * l1_share, l2 = regul_coef *
    (1 - l1_share)), differentiable in every weight; deterministic. Device scalar.

    A weight whose product gradient is computed on the side stream (_weight_on_side_stream)
    gets its penalty node on that stream too, so every gradient reaching that weight is
    produced on the stream its AccumulateGrad node lives on (no cross-stream accumulation);
    consecutive weights on one stream share a node, and the running sum is chained from node
    to node in the given order (the same kernels and the same sum as one node)."""
    if not weights or len(weights) != len(coefs):
        raise ValueError("l1l2_penalty needs one (l1, l2) pair per weight, at least one weight")
    for W in weights:
        _require_cuda(W, "W")
        if W.dtype != torch.float32 or not W.is_contiguous():
            raise TypeError("l1l2_penalty needs contiguous float32 weights")
    coefs = [(float(a), float(b)) for a, b in coefs]
    dev = weights[0].device
    main = torch.cuda.current_stream(dev)
    groups = []  # [(on_side, [indices])]
    for i, W in enumerate(weights):
        side = bool(getattr(W, "_gcg_side_grad", False)) and torch.is_grad_enabled() \
            and W.requires_grad
        if groups and groups[-1][0] == side:
            groups[-1][1].append(i)
        else:
            groups.append((side, [i]))
    acc = None
    for side, idx in groups:
        ws = [weights[i] for i in idx]
        cs = tuple(coefs[i] for i in idx)
        if side:
            s = _side_stream(dev)
            s.wait_stream(main)
            with torch.cuda.stream(s):
                acc = _L1L2Penalty.apply(cs, acc, *ws)
            main.wait_stream(s)
        else:
            acc = _L1L2Penalty.apply(cs, acc, *ws)
    return acc


def softmax(logits: torch.Tensor) -> torch.Tensor:
    """Row softmax (predict_proba) through the row kernel."""
    _require_cuda(logits, "logits")
    M, N = logits.shape
    out = empty_dense(M, N, logits.device)
    _rows_call(logits, None, 1.0, None, out, None, None)
    return out
