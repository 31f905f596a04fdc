"""Dropout with counter-based masks: the reference's `drop_out=True` (mlpconv.py:37-58, 199-201,
210-211) without a stored mask.

The keep decision of an element is a pure function of its logical coordinates, the stream's
seed and id, and a step counter (include/gcg_spmm.h, restated in NumPy below):

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (uint32(i), uint32(j >> 2), uint32(step), stream_id)
    keep    = philox4x32_10(counter, key)[j & 3] >= floor(p * 2**32)

so the backward pass regenerates the mask instead of reading it, CSR(X) and CSR(X^T) drop the
same elements, any row partition draws the same mask, and a captured HIP graph draws a fresh
mask on every replay (the step is a device scalar the host advances before the replay).

  philox4x32_10, keep_mask_reference   NumPy: the executable statement of the rule (CPU)
  DropoutStream                        seed, stream id and the device step scalar
  DropoutSpec                          (stream, p, rescale): what a kernel call needs
  dropout_dense / dropout_relu_backward / csr_dropout    the three HIP entry points
  DropoutView                          a DeviceCSR's values behind a mask, structure shared
  SparseInputDropoutLayer, DropoutLayer (alias dropout)   Lasagne's names and arguments

Parity: the reference's masks come from Theano's MRG31k3p stream, which cannot be run here;
like the Glorot draw order this is distributional parity, unpinned.
"""
from __future__ import annotations

import math
from typing import Optional, Union

import numpy as np
import scipy.sparse as sps
import torch
import torch.nn as nn

from . import sparse as gs
from ._native import call
from .sparse import _ld, _ptr, _stream_handle

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------
# NumPy restatement (no GPU)
# ---------------------------------------------------------------------------------------
def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32-10 (Random123). counter: four words (scalars or arrays that broadcast
    together, or one array whose last axis is 4); key: two words. Returns uint32 [..., 4]."""
    if isinstance(counter, np.ndarray) and counter.ndim >= 1 and counter.shape[-1] == 4:
        counter = tuple(counter[..., i] for i in range(4))
    c = [np.asarray(x).astype(np.uint64) & _MASK32 for x in counter]
    c = [np.array(x) for x in np.broadcast_arrays(*c)]
    k0, k1 = (int(k) & _MASK32 for k in key)
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(_MASK32),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(_MASK32)]
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return np.stack(c, axis=-1).astype(np.uint32)


def dropout_threshold(p: float) -> int:
    """floor(p * 2**32) in double: an element is dropped iff its Philox word is below it."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("the dropout probability p must be in [0, 1)")
    return int(math.floor(p * 4294967296.0))


def dropout_scale(p: float, rescale: bool = True) -> float:
    """float32(1 / (1 - p)) when rescale (Lasagne's default), else 1."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("the dropout probability p must be in [0, 1)")
    return float(np.float32(1.0 / (1.0 - p))) if rescale else 1.0


def keep_mask_reference(rows, cols, p: float, seed: int, step: int, stream_id: int) -> np.ndarray:
    """Boolean keep mask of the elements (rows[...], cols[...]) (integer arrays that broadcast
    together; logical coordinates)."""
    rows, cols = np.broadcast_arrays(np.asarray(rows, dtype=np.int64),
                                     np.asarray(cols, dtype=np.int64))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10((rows, cols >> 2, int(step) & _MASK32, int(stream_id) & _MASK32),
                          (seed & _MASK32, seed >> 32))
    word = np.take_along_axis(words, (cols & 3)[..., None], axis=-1)[..., 0]
    return word >= np.uint32(dropout_threshold(p))


# ---------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------
def draw_seed(rng=None) -> int:
    """The seed of a dropout layer, drawn as Lasagne's DropoutLayer.__init__ draws it:
    get_rng().randint(1, 2147462579) from the stream the weights come from (numpy's global
    stream unless `rng` is given: an int seed, a RandomState or a Generator). [recalled
    Lasagne 0.2; Lasagne is not importable here, so this draw order is parity-unpinned.]"""
    if rng is None:
        rng = np.random.mtrand._rand
    elif isinstance(rng, (int, np.integer)):
        rng = np.random.RandomState(int(rng))
    if isinstance(rng, np.random.Generator):
        return int(rng.integers(1, 2147462579))
    return int(rng.randint(1, 2147462579))


class DropoutStream:
    """One independent mask stream: a 64-bit seed, a 32-bit stream id and the step counter.

    The step lives in a device int32 scalar the kernels read (as LasagneAdam's a_t), so a
    captured HIP graph replays with whatever `advance()` wrote before the replay. A forward
    and its backward must run under the same step; `advance()` once per training step."""

    def __init__(self, seed: int, stream_id: int = 0, device: Union[str, torch.device] = "cuda"):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.stream_id = int(stream_id) & _MASK32
        self.device = torch.device(device)
        self.step = -1  # the first advance() starts step 0 (the scalar's initial value)
        self.step_dev = torch.zeros((), dtype=torch.int32, device=self.device)

    def advance(self) -> int:
        """Host half of a step: write the next step value (like LasagneAdam.prepare)."""
        return self.set_step(self.step + 1)

    def set_step(self, step: int) -> int:
        self.step = int(step)
        self.step_dev.fill_(max(self.step, 0) & 0x7FFFFFFF)
        return self.step

    threshold = staticmethod(dropout_threshold)
    scale = staticmethod(dropout_scale)

    def keep_mask(self, rows, cols, p: float, step: Optional[int] = None) -> np.ndarray:
        """The NumPy restatement of this stream's mask at `step` (default: the current one)."""
        step = max(self.step, 0) if step is None else step
        return keep_mask_reference(rows, cols, p, self.seed, step & 0x7FFFFFFF, self.stream_id)


class DropoutSpec:
    """(stream, p, rescale) with the ABI values: what one masked kernel call needs."""

    __slots__ = ("stream", "p", "rescale", "threshold", "scale")

    def __init__(self, stream: DropoutStream, p: float, rescale: bool = True):
        self.stream, self.p, self.rescale = stream, float(p), bool(rescale)
        self.threshold = dropout_threshold(p)
        self.scale = dropout_scale(p, rescale)

    def abi(self):
        """threshold, scale, seed, step_dev, stream_id -- in the C-ABI's order."""
        s = self.stream
        return self.threshold, self.scale, s.seed, _ptr(s.step_dev), s.stream_id


def make_spec(stream: Optional[DropoutStream], p: float, rescale: bool = True,
              deterministic: bool = False) -> Optional[DropoutSpec]:
    """None when nothing is to be dropped (deterministic, or p == 0: mlpconv.py:43-44)."""
    if deterministic or float(p) == 0.0:
        return None
    if stream is None:
        raise ValueError("dropout needs a DropoutStream")
    return DropoutSpec(stream, p, rescale)


# ---------------------------------------------------------------------------------------
# the three entry points
# ---------------------------------------------------------------------------------------
def _check_2d(t: torch.Tensor, name: str):
    gs._require_cuda(t, name)
    if t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name} must be a 2-D float32 tensor with unit column stride")


def dropout_dense(X: torch.Tensor, spec: DropoutSpec, out: Optional[torch.Tensor] = None,
                  row0: int = 0, col_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = drop(X) (gcg_dropout_f32). out may be X (in place); logical rows row0 + r, logical
    columns col_ids[c] (int32 device tensor) or c."""
    _check_2d(X, "X")
    M, K = X.shape
    if out is None:
        out = gs.empty_dense(M, K, X.device)
    _check_2d(out, "out")
    if out.shape != X.shape:
        raise ValueError("out must have X's shape")
    if col_ids is not None and (col_ids.dtype != torch.int32 or col_ids.numel() != K
                                or not col_ids.is_contiguous()):
        raise ValueError(f"col_ids must be a contiguous int32[{K}] device tensor")
    with torch.cuda.device(X.device):
        call("gcg_dropout_f32", M, K, _ptr(X), _ld(X), _ptr(out), _ld(out), *spec.abi(),
             int(row0), _ptr(col_ids), _stream_handle(X.device))
    return out


def dropout_relu_backward(gY: torch.Tensor, spec: DropoutSpec,
                          gate: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None, bias_grad: bool = True,
                          row0: int = 0):
    """(g, db): the gradient of drop(rectify(.)) and its column sums in one pass
    (gcg_dropout_relu_backward_f32): the mask is regenerated, then Theano's gate rule as
    sparse.relu_backward(gate=...); gate None: g = keep ? gY * scale : 0. out may be gY.
    Beyond 1024 columns the same pass in slabs of 1024 (gcg_rectify_backward_wide_f32)."""
    gs._require_cuda(gY, "gY")
    M, K = gY.shape
    ldgate = 0
    if gate is not None:
        if gate.dtype != torch.uint8 or gate.shape != (M, K) or (K > 1 and gate.stride(1) != 1):
            raise ValueError("gate must be uint8 [M, K] with unit column stride")
        ldgate = gate.stride(0) if M > 1 else (K + 3) // 4 * 4
    rows16 = (M <= 1 or gY.stride(0) % 4 == 0) and gY.data_ptr() % 16 == 0
    if (K > 1 and gY.stride(1) != 1) or (K > 256 and not rows16):
        gY = gs.empty_dense(M, K, gY.device).copy_(gY)  # the wide path loads dwordx4
    if out is None:
        out = gs.empty_dense(M, K, gY.device)
    _check_2d(gY, "gY")
    _check_2d(out, "out")
    db = torch.empty(K, dtype=torch.float32, device=gY.device) if bias_grad else None
    ws = gs._colsum_workspace(M, K, gY.device)
    ld = gs._ld16 if K > 256 else _ld
    with torch.cuda.device(gY.device):
        call("gcg_dropout_relu_backward_f32" if K <= 1024 else "gcg_rectify_backward_wide_f32",
             M, K, _ptr(gY), ld(gY), _ptr(gate), ldgate, _ptr(out), ld(out), _ptr(db), _ptr(ws),
             ws.numel() * 4, *spec.abi(), int(row0), _stream_handle(gY.device))
    return out, db


def csr_dropout(A: gs.DeviceCSR, vals: torch.Tensor, out: torch.Tensor, spec: DropoutSpec,
                transposed: bool = False) -> torch.Tensor:
    """out[k] = drop(vals[k]) for every stored entry of A's structure (gcg_csr_dropout_f32);
    transposed: A is CSR(X^T), its entries are masked as the elements of X they are."""
    for t, n in ((vals, "vals"), (out, "out")):
        gs._require_cuda(t, n)
        if t.dtype != torch.float32 or t.numel() != A.nnz or not t.is_contiguous():
            raise ValueError(f"{n} must be a contiguous float32[nnz] device tensor")
    with torch.cuda.device(A.device):
        call("gcg_csr_dropout_f32", A.n_rows, A.n_cols, A.nnz, _ptr(A.indptr), _ptr(A.indices),
             _ptr(vals), _ptr(out), int(bool(transposed)), *spec.abi(), _stream_handle(A.device))
    return out


# ---------------------------------------------------------------------------------------
# a DeviceCSR's values behind a mask
# ---------------------------------------------------------------------------------------
class _DroppedValues(gs.DeviceCSR):
    """The structure of `struct` (indptr, indices, launch plans, gather hints, longest row:
    shared, not copied) with a persistent values buffer of its own, rewritten every step. The
    buffer's address never changes, so a captured HIP graph replays it."""

    def __init__(self, struct: gs.DeviceCSR, transposed: bool):
        self.struct = struct
        self.transposed = bool(transposed)
        self.indptr, self.indices = struct.indptr, struct.indices
        self.data = torch.empty_like(struct.data)
        self.shape, self.n_rows, self.n_cols = struct.shape, struct.n_rows, struct.n_cols
        self.nnz, self.device = struct.nnz, struct.device
        self.symmetric = False  # a mask is not symmetric: A^T always means the transposed twin
        self._plans = struct._plans
        self.__dict__["_gather_hints"] = struct.__dict__.setdefault("_gather_hints", {})
        self._max_row_nnz = struct.max_row_nnz()
        self._transpose = None
        self.op_id = gs._register_object(self)

    def fill(self, spec: DropoutSpec):
        csr_dropout(self.struct, self.struct.data, self.data, spec, self.transposed)

    def rows_transpose(self, rows):
        raise NotImplementedError("a dropout view has no cached row-subset transpose")


class DropoutView(_DroppedValues):
    """X behind a dropout mask (the reference's SparseInputDropoutLayer output): a DeviceCSR
    that shares everything but the values with its base. `refresh(spec)` rewrites the values of
    X and of every twin the backward has asked for so far -- CSR(X^T), or the dense head block
    and the tail's transpose of DeviceCSR._dense_column_split -- on the current stream; a twin
    asked for later in the same step is filled when it is created. All of them mask element
    (i, j) alike, by construction."""

    def __init__(self, base: gs.DeviceCSR, stream: DropoutStream):
        super().__init__(base, transposed=False)
        self.base, self.stream = base, stream
        self._spec: Optional[DropoutSpec] = None
        self._t: Optional[_DroppedValues] = None
        self._head_src = self._cols32 = None

    def refresh(self, spec: DropoutSpec) -> "DropoutView":
        if spec.stream is not self.stream:
            raise ValueError("this view belongs to another DropoutStream")
        self._spec = spec
        self.fill(spec)
        if self._t is not None:
            self._t.fill(spec)
        split = self.__dict__.get("_dense_split")
        if split is not None:
            self._fill_split(split, spec)
        return self

    def _fill_split(self, split, spec: DropoutSpec):
        _cols, head, tail_t = split
        tail_t.fill(spec)
        # on the caller's (main) stream: tmatmul's side stream waits on it before the GEMM
        dropout_dense(self._head_src, spec, out=head, col_ids=self._cols32)

    def _base_transpose(self) -> gs.DeviceCSR:
        t = self.base.transpose()
        if t is self.base:  # a symmetric base stands in for its own transpose; a mask cannot
            b = self.base
            t = gs.DeviceCSR(b.indptr, b.indices, b.data, b.shape, symmetric=False,
                             validate=False).transpose()
        return t

    def transpose(self) -> gs.DeviceCSR:
        if self._t is None:
            t = _DroppedValues(self._base_transpose(), transposed=True)
            t._transpose = self
            if self._spec is not None:
                t.fill(self._spec)
            self._t = t
        return self._t

    def _dense_column_split(self):
        if "_dense_split" not in self.__dict__:
            split = None
            bs = self.base._dense_column_split()
            if bs is not None:
                cols, Xh, tail_t = bs
                self._head_src, self._cols32 = Xh, cols.to(torch.int32).contiguous()
                split = (cols, gs.empty_dense(Xh.shape[0], Xh.shape[1], self.device),
                         _DroppedValues(tail_t, transposed=True))
                if self._spec is not None:
                    self._fill_split(split, self._spec)
            self._dense_split = split
        return self._dense_split


def dropout_view(base: gs.DeviceCSR, stream: DropoutStream) -> DropoutView:
    """The view of `base` for `stream`, created once per (matrix, stream)."""
    cache = base.__dict__.setdefault("_dropout_views", {})
    v = cache.get(id(stream))
    if v is None or v.stream is not stream:
        v = DropoutView(base, stream)
        cache[id(stream)] = v
    return v


# ---------------------------------------------------------------------------------------
# layers (Lasagne's names and arguments)
# ---------------------------------------------------------------------------------------
def _not_under_compile():
    if torch.compiler.is_compiling():
        raise NotImplementedError(
            "dropout is not available under torch.compile: the mask kernels are not registered "
            "torch ops; run the layer eagerly or pass deterministic=True")


class SparseInputDropoutLayer(nn.Module):
    """mlpconv.py:37-58: dropout on a sparse input, structure kept, values masked.

    forward(X, deterministic=False) returns X itself when deterministic or p == 0, else the
    DropoutView of X with this step's mask. The stream's seed is drawn at construction as
    Lasagne draws it (draw_seed) unless a DropoutStream is given; the owner of the stream
    advances it once per training step."""

    def __init__(self, incoming=None, p: float = 0.5, rescale: bool = True,
                 stream: Optional[DropoutStream] = None,
                 device: Union[str, torch.device] = "cuda", rng=None, stream_id: int = 0):
        super().__init__()
        dropout_threshold(p)
        self.p, self.rescale = float(p), bool(rescale)
        self.device = torch.device(device)
        self.stream = stream if stream is not None else \
            DropoutStream(draw_seed(rng), stream_id, self.device)
        self._cache = {}

    def forward(self, input, deterministic: bool = False, **kwargs):
        if not (isinstance(input, gs.DeviceCSR) or sps.issparse(input)):
            raise ValueError("Input for this layer must be sparse")  # mlpconv.py:40-42
        spec = make_spec(self.stream, self.p, self.rescale, deterministic)
        if spec is None:
            return input
        _not_under_compile()
        if not isinstance(input, gs.DeviceCSR):
            from .layers import _upload_cached
            input = _upload_cached(self._cache, input, self.device)
        return dropout_view(input, self.stream).refresh(spec)

    def get_output_for(self, input, **kwargs):
        return self.forward(input, **kwargs)


class _DenseDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, spec):
        ctx.spec = spec
        return dropout_dense(X if X.stride(-1) == 1 else X.contiguous(), spec)

    @staticmethod
    def backward(ctx, gY):
        g, _ = dropout_relu_backward(gY, ctx.spec, gate=None, bias_grad=False)
        return g, None


class DropoutLayer(nn.Module):
    """lasagne.layers.DropoutLayer on a dense [M, K] float32 tensor: forward gcg_dropout_f32,
    backward the mask regenerated by dropout_relu_backward."""

    def __init__(self, incoming=None, p: float = 0.5, rescale: bool = True,
                 stream: Optional[DropoutStream] = None,
                 device: Union[str, torch.device] = "cuda", rng=None, stream_id: int = 0):
        super().__init__()
        dropout_threshold(p)
        self.p, self.rescale = float(p), bool(rescale)
        self.stream = stream if stream is not None else \
            DropoutStream(draw_seed(rng), stream_id, torch.device(device))

    def forward(self, input, deterministic: bool = False, **kwargs):
        spec = make_spec(self.stream, self.p, self.rescale, deterministic)
        if spec is None:
            return input
        _not_under_compile()
        if input.dim() != 2:
            raise NotImplementedError("DropoutLayer takes a 2-D input")
        return _DenseDropout.apply(input, spec)

    def get_output_for(self, input, **kwargs):
        return self.forward(input, **kwargs)


dropout = DropoutLayer  # shortcut, as lasagne.layers.dropout
