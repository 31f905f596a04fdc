"""The location-to-language model -- the reference's loc2lang.py (lat/lon to a word distribution).

A coordinate goes through a layer of C trainable bivariate Gaussians (lasagne_layers.py:156-214),
a rectified hidden layer and a softmax over the vocabulary, and is trained against each user's
l1-normalised bag of words by categorical cross-entropy with Adamax (loc2lang.py:118-292).

  bigaus_layer             G [B, C], the density of every component     gcg_bigaus_layer_f32,
                           at every coordinate, differentiable in the   gcg_bigaus_layer_backward_f32
                           three parameter tensors
  BivariateGaussianLayer   the reference's layer: its defaults and draw order
  softmax_xent_csr         mean cross-entropy of logits [M, V] against  gcg_softmax_xent_csr_f32
                           rows of a CSR target, differentiable in the  (loss and gradient, one
                           logits; the target is never densified        launch)
  softmax_wide             softmax of rows of any width                 the same kernel
  LasagneAdamax            lasagne.updates.adamax, one launch per       gcg_adamax_step_f32
                           parameter
  NNModel_loc2lang         the reference's class: constructor arguments, fit, predict
  NNModel_loc2lang_nomdn   its nomdn=True build, the baseline: a rectified dense  gcg_minibatch_w1_adamax_step_f32
                           layer in place of the Gaussians, over the grid
                           representation (grid.py, sparse) or raw coordinates
  local_words              get_local_words (loc2lang.py:755-766) without the named-entity filter
  row_lse                  the float64 log-sum-exp of every logits row  gcg_row_lse_f64
  softmax_column_stats     per word, sum_n p and sum_n p log p of       gcg_softmax_column_stats_f64
                           p = softmax(z), accumulated over row chunks
  region_recall            the recall lines of state_dialect_words (loc2lang.py:587-614) from a
                           [G, V] score matrix and the regions' gold words

The model's analyses (word_entropies, local_words, word_probabilities, top_words,
region_word_scores) run on these two kernels in one chunked scan; the n x V probabilities never
leave the device and are never held whole.

The transforms of the Gaussians' parameters and the order of every sum are stated in
include/gcg_spmm.h.
"""
from __future__ import annotations

import logging
from collections import namedtuple
from typing import Optional

import numpy as np
import scipy.sparse as sps
import torch

from . import dense
from . import sparse as gs
from ._native import call, device_scalar, workspace, workspace_bytes
from .layers import _as_tensor, _glorot_uniform
from .mdn import MAX_COMPONENTS, _check_components, split_dparams
from .mlp import BatchSegments, plan_segmented_epoch, w1_adamax_step
from .sparse import _ld, _ptr, _stream_handle
from .training import (LasagneOptimizer, MiniBatchTrainer, lower_loss_by_margin, n_batches,
                       run_epochs)

log = logging.getLogger(__name__)

MAX_COLS = 1 << 24          # gcg_softmax_xent_csr_f32's widest row
MAX_HIDDEN = 1024           # the rectify backward's one-pass kernel (sparse.relu_backward)
EVAL_CHUNK_BYTES = 1 << 30  # a chunk's logits stay under this in evaluation and predict

RegionRecall = namedtuple("RegionRecall", "ks recall oracle per_group ranks")


def _row_chunk(x, a: int, b: int):
    """Rows [a, b) of a model input: a slice of a dense tensor, DeviceCSR.row_slice of a sparse one."""
    return x.row_slice(a, b) if isinstance(x, gs.DeviceCSR) else x[a:b]


# -- the Gaussian layer ---------------------------------------------------------------------
def _coords(X: torch.Tensor, dev) -> torch.Tensor:
    gs._require_cuda(X, "X")
    if X.dtype != torch.float32 or X.dim() != 2 or X.shape[1] != 2 or X.device != dev:
        raise ValueError("X must be a float32 [B, 2] tensor (lat, lon) on the parameters' device")
    return X.contiguous()


def bigaus_forward(X: torch.Tensor, mus: torch.Tensor, sigmas_raw: torch.Tensor,
                   corxy_raw: torch.Tensor) -> torch.Tensor:
    """G [B, C] float32: the density of component c at the coordinate X[r] (one
    gcg_bigaus_layer_f32 call; no autograd)."""
    mus, sigmas_raw, corxy_raw = _check_components(mus, sigmas_raw, corxy_raw)
    X = _coords(X, mus.device)
    B, C, dev = X.shape[0], mus.shape[0], mus.device
    G = gs.empty_dense(B, C, dev)
    with torch.cuda.device(dev):
        call("gcg_bigaus_layer_f32", B, C, _ptr(X), _ptr(mus), _ptr(sigmas_raw), _ptr(corxy_raw),
             _ptr(G), _ld(G), _stream_handle(dev))
    return G


def bigaus_backward_workspace_bytes(B: int, C: int) -> int:
    return workspace_bytes("gcg_bigaus_layer_backward_f32_workspace_bytes", B, C)


def bigaus_backward(X: torch.Tensor, mus: torch.Tensor, sigmas_raw: torch.Tensor,
                    corxy_raw: torch.Tensor, dG: torch.Tensor,
                    scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dparams [5, C] (mdn.split_dparams' planes): the gradient of the three parameter tensors
    from the upstream dG [B, C], times the device scalar `scale` when given (one
    gcg_bigaus_layer_backward_f32 call)."""
    mus, sigmas_raw, corxy_raw = _check_components(mus, sigmas_raw, corxy_raw)
    X = _coords(X, mus.device)
    B, C, dev = X.shape[0], mus.shape[0], mus.device
    gs._require_cuda(dG, "dG")
    if dG.dtype != torch.float32 or tuple(dG.shape) != (B, C) or dG.device != dev:
        raise ValueError(f"dG must be a float32 [{B}, {C}] tensor on {dev}")
    if C > 1 and dG.stride(1) != 1:
        dG = dG.contiguous()
    dparams = torch.empty((5, C), dtype=torch.float32, device=dev)
    if B == 0:
        return dparams.zero_()
    ws, nbytes = workspace("gcg_bigaus_layer_backward_f32_workspace_bytes", dev, B, C)
    scale = device_scalar(scale)
    with torch.cuda.device(dev):
        call("gcg_bigaus_layer_backward_f32", B, C, _ptr(X), _ptr(mus), _ptr(sigmas_raw),
             _ptr(corxy_raw), _ptr(dG), _ld(dG), _ptr(scale), _ptr(dparams), _ptr(ws), nbytes,
             _stream_handle(dev))
    return dparams


class _BigausLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, mus, sigmas_raw, corxy_raw):
        ctx.save_for_backward(X, mus, sigmas_raw, corxy_raw)
        return bigaus_forward(X, mus, sigmas_raw, corxy_raw)

    @staticmethod
    def backward(ctx, dG):
        dmus, dsig, dcor = split_dparams(bigaus_backward(*ctx.saved_tensors, dG))
        return None, dmus, dsig, dcor


def bigaus_layer(X: torch.Tensor, mus: torch.Tensor, sigmas_raw: torch.Tensor,
                 corxy_raw: torch.Tensor) -> torch.Tensor:
    """BivariateGaussianLayer.get_output_for (lasagne_layers.py:187-214): G [B, C], the density
    of N(mus[c], softplus(sigmas_raw[c]), softsign(corxy_raw[c])) at X[r] (lat, lon),
    differentiable in the three parameter tensors; X has no gradient (it is the network's
    input)."""
    return _BigausLayer.apply(X, mus, sigmas_raw, corxy_raw)


class BivariateGaussianLayer(torch.nn.Module):
    """lasagne_layers.BivariateGaussianLayer: num_units Gaussians over (lat, lon). Parameters not
    given are drawn as the reference draws them, in its order, from NumPy's global stream:
    mus = randn(C, 2), sigmas = 10 * ones(C, 2) (raw: sigma = softplus(.)), corxy = randn(C)
    (raw: rho = softsign(.)) (lasagne_layers.py:164-178)."""

    def __init__(self, num_units: int, mus=None, sigmas=None, corxy=None, device="cuda"):
        super().__init__()
        C = int(num_units)
        if not 1 <= C <= MAX_COMPONENTS:
            raise ValueError(f"num_units must be in [1, {MAX_COMPONENTS}], got {C}")
        mus, sigmas, corxy = draw_components(C, mus, sigmas, corxy)
        self.num_units = C
        self.mus = torch.nn.Parameter(_as_tensor(mus, (C, 2), device))
        self.sigmas = torch.nn.Parameter(_as_tensor(sigmas, (C, 2), device))
        self.corxy = torch.nn.Parameter(_as_tensor(corxy, (C,), device))

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        return bigaus_layer(X, self.mus, self.sigmas, self.corxy)


def draw_components(C: int, mus=None, sigmas=None, corxy=None):
    """The layer's three initial arrays: those given, the others by lasagne_layers.py:164-178
    (mus' draw before corxy's; sigmas takes none)."""
    if mus is None:
        mus = np.random.randn(C, 2).astype(np.float32)
    if sigmas is None:
        sigmas = np.array([10, 10], np.float32) * np.ones((C, 2), np.float32)
    if corxy is None:
        corxy = np.random.randn(C).reshape((C,)).astype(np.float32)
    return mus, sigmas, corxy


# -- softmax cross-entropy against sparse soft targets ------------------------------------------
def check_targets(Y) -> sps.csr_matrix:
    """A scipy sparse (or dense) target as the canonical-column CSR the kernel needs, float32,
    checked on the host: every column in [0, n_cols) and no column twice in a row (the kernel
    subtracts a row's entries in place; of two on one column one would be lost). ValueError
    otherwise -- nothing is summed or dropped silently."""
    if not sps.issparse(Y):
        Y = sps.csr_matrix(np.asarray(Y, dtype=np.float32))
    Y = Y.tocsr() if Y.format != "csr" else Y
    indptr, indices = np.asarray(Y.indptr), np.asarray(Y.indices)
    if indptr.size != Y.shape[0] + 1 or indptr[0] != 0 or indptr[-1] != indices.size or \
            (np.diff(indptr) < 0).any():
        raise ValueError("target CSR: indptr must be monotone from 0 to nnz")
    if indices.size and (indices.min() < 0 or indices.max() >= Y.shape[1]):
        raise ValueError(f"target CSR: a column index is outside [0, {Y.shape[1]})")
    row_of = np.repeat(np.arange(Y.shape[0]), np.diff(indptr))
    key = row_of.astype(np.int64) * Y.shape[1] + indices
    if np.unique(key).size != key.size:
        raise ValueError("target CSR: a row holds the same column twice (sum_duplicates() first)")
    return sps.csr_matrix((np.asarray(Y.data, dtype=np.float32), indices.astype(np.int32),
                           indptr.astype(np.int32)), shape=Y.shape)


def target_csr(Y, device="cuda") -> gs.DeviceCSR:
    """Upload a target matrix once: check_targets on the host, then DeviceCSR (validated on the
    device as every DeviceCSR is), marked as free of duplicate columns."""
    if isinstance(Y, gs.DeviceCSR):
        return _checked(Y)
    Yd = gs.DeviceCSR.from_scipy(check_targets(Y), device)
    Yd._rows_unique = True
    return Yd


def _checked(Y: gs.DeviceCSR) -> gs.DeviceCSR:
    """A DeviceCSR built elsewhere: its rows checked for duplicate columns once, on the device
    (one synchronisation, remembered on the object)."""
    if getattr(Y, "_rows_unique", None) is None:
        unique = True
        if Y.nnz > 1:
            counts = (Y.indptr[1:] - Y.indptr[:-1]).to(torch.int64)
            row_of = torch.repeat_interleave(torch.arange(Y.n_rows, device=Y.device), counts)
            key = row_of * Y.n_cols + Y.indices.to(torch.int64)
            unique = int(torch.unique(key).numel()) == Y.nnz
        Y._rows_unique = unique
    if not Y._rows_unique:
        raise ValueError("target CSR: a row holds the same column twice")
    return Y


def check_rows(rows, y_rows: int, M: int) -> np.ndarray:
    """Host-side row ids of the target, one per logits row, as int32: ValueError unless there
    are M of them, all in [0, y_rows)."""
    rows = np.asarray(rows)
    if rows.ndim != 1 or rows.size != M or rows.dtype.kind not in "iu":
        raise ValueError(f"rows must be {M} integer row ids of the target")
    if rows.size and (rows.min() < 0 or rows.max() >= y_rows):
        raise ValueError(f"rows: a row id is outside [0, {y_rows})")
    return np.ascontiguousarray(rows, dtype=np.int32)


def _device_rows(rows, Y: gs.DeviceCSR, M: int) -> Optional[torch.Tensor]:
    """rows as the kernel takes them. A host array is validated here; a device tensor is taken
    as it is (the kernel gives a row id out of range a NaN loss, never an index)."""
    if rows is None:
        if Y.n_rows < M:
            raise ValueError(f"the target has {Y.n_rows} rows, the logits {M}")
        return None
    if isinstance(rows, torch.Tensor) and rows.is_cuda:
        if rows.dtype != torch.int32 or rows.dim() != 1 or rows.numel() != M or \
                rows.device != Y.device:
            raise ValueError(f"device rows must be {M} int32 row ids on the target's device")
        return rows.contiguous()
    if isinstance(rows, torch.Tensor):
        rows = rows.numpy()
    return torch.from_numpy(check_rows(rows, Y.n_rows, M)).to(Y.device)


def _check_logits(logits: torch.Tensor) -> torch.Tensor:
    gs._require_cuda(logits, "logits")
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError("logits must be a float32 [M, N] tensor")
    if not 1 <= logits.shape[1] <= MAX_COLS:
        raise ValueError(f"logits must have 1 .. {MAX_COLS} columns")
    return logits if logits.shape[1] == 1 or logits.stride(1) == 1 else logits.contiguous()


def xent_csr_forward_backward(logits: torch.Tensor, Y: gs.DeviceCSR,
                              rows: Optional[torch.Tensor] = None, scale: float = 1.0,
                              scale_dev: Optional[torch.Tensor] = None, want_grad: bool = True,
                              in_place: bool = False):
    """(loss_rows [M], dlogits or None) from one gcg_softmax_xent_csr_f32 call.
    loss_rows[i] = -sum_j Y[rows[i]][j] log softmax(logits[i])_j; dlogits = scale * *scale_dev *
    d loss_rows[i] / d logits[i] (None unless want_grad; in_place: written over the logits).
    rows: int32 device row ids of Y (None: row i), Y: a target_csr(...)."""
    logits = _check_logits(logits)
    M, N = logits.shape
    if Y.n_cols != N or Y.device != logits.device:
        raise ValueError(f"the target must be [*, {N}] on {logits.device}")
    dev = logits.device
    loss_rows = torch.empty(M, dtype=torch.float32, device=dev)
    out = None
    if want_grad:
        out = logits if in_place else gs.empty_dense(M, N, dev)
    scale_dev = device_scalar(scale_dev)
    with torch.cuda.device(dev):
        call("gcg_softmax_xent_csr_f32", M, N, _ptr(logits), _ld(logits), Y.n_rows,
             _ptr(Y.indptr), _ptr(Y.indices), _ptr(Y.data), _ptr(rows), float(scale),
             _ptr(scale_dev), _ptr(out), _ld(out) if out is not None else 0, _ptr(loss_rows),
             _stream_handle(dev))
    return loss_rows, out


class _SoftmaxXentCSR(torch.autograd.Function):
    """The forward launch already writes the gradient of the mean (upstream 1); backward scales
    it by the upstream gradient."""

    @staticmethod
    def forward(ctx, logits, Y, rows, denom):
        want = ctx.needs_input_grad[0]
        loss_rows, dZ = xent_csr_forward_backward(logits, Y, rows, scale=1.0 / denom,
                                                  want_grad=want)
        ctx.dZ = dZ
        return loss_rows.sum() / denom

    @staticmethod
    def backward(ctx, g):
        return ctx.dZ * g, None, None, None


def softmax_xent_csr(logits: torch.Tensor, Y: gs.DeviceCSR, rows=None,
                     denom: Optional[int] = None) -> torch.Tensor:
    """lasagne.objectives.categorical_crossentropy(softmax(logits), Y[rows]).sum() / denom
    (loc2lang.py:193-194; denom defaults to the M rows: the mean) as a device scalar,
    differentiable in the logits. Y: the soft targets as a DeviceCSR (target_csr: columns in
    range, none twice in a row), never densified; rows: one row id of Y per logits row -- a host
    array (validated: ValueError before any launch) or int32 device tensor; None pairs row i
    with row i. Written as sum_k y_k (logsumexp(z) - z_k): the reference's -sum y log p wherever
    that is finite."""
    Y = target_csr(Y)
    logits = _check_logits(logits)
    M = logits.shape[0]
    rows = _device_rows(rows, Y, M)
    return _SoftmaxXentCSR.apply(logits, Y, rows, float(max(M if denom is None else denom, 1)))


def softmax_wide(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row softmax of logits [M, N] of any width up to 2^24 (dense.softmax stops at 4096
    columns): gcg_softmax_xent_csr_f32 without a target. out may be the logits."""
    logits = _check_logits(logits)
    M, N = logits.shape
    if out is None:
        out = gs.empty_dense(M, N, logits.device)
    with torch.cuda.device(logits.device):
        call("gcg_softmax_xent_csr_f32", M, N, _ptr(logits), _ld(logits), 0, None, None, None,
             None, 1.0, None, _ptr(out), _ld(out), None, _stream_handle(logits.device))
    return out


# -- the analyses' two passes over a chunk of logits ------------------------------------------------
def row_lse(logits: torch.Tensor) -> torch.Tensor:
    """lse [M] float64: max_j z_ij + log sum_j exp(z_ij - max) of every row of logits [M, N]
    (gcg_row_lse_f64: softmax_xent_csr's float32 fold, the log and the add in double)."""
    if not isinstance(logits, torch.Tensor):
        raise TypeError("logits must be a torch tensor")
    logits = _check_logits(logits)
    M, N = logits.shape
    lse = torch.empty(M, dtype=torch.float64, device=logits.device)
    with torch.cuda.device(logits.device):
        call("gcg_row_lse_f64", M, N, _ptr(logits), _ld(logits), _ptr(lse),
             _stream_handle(logits.device))
    return lse


def _check_f64(t, n: int, dev, name: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor")
    gs._require_cuda(t, name)
    if t.dtype != torch.float64 or t.dim() != 1 or t.numel() != n or t.device != dev or \
            not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float64 [{n}] tensor on {dev}")


def softmax_column_stats(logits: torch.Tensor, lse: torch.Tensor, S: torch.Tensor,
                         T: torch.Tensor) -> None:
    """Adds the rows of logits [M, N] to the per-column sums S, T (float64 [N], zeroed by the
    caller before the first chunk): with p = exp(z - lse[i]), S[j] += p and T[j] += p (z - lse[i])
    (0 where p == 0), the rows in ascending order (gcg_softmax_column_stats_f64). Chunks of rows
    given in order leave the bits of one call over all rows. lse: row_lse(logits)."""
    if not isinstance(logits, torch.Tensor):
        raise TypeError("logits must be a torch tensor")
    logits = _check_logits(logits)
    M, N = logits.shape
    _check_f64(lse, M, logits.device, "lse")
    _check_f64(S, N, logits.device, "S")
    _check_f64(T, N, logits.device, "T")
    if S.data_ptr() == T.data_ptr():
        raise ValueError("S and T must be two tensors")
    with torch.cuda.device(logits.device):
        call("gcg_softmax_column_stats_f64", M, N, _ptr(logits), _ld(logits), _ptr(lse), _ptr(S),
             _ptr(T), _stream_handle(logits.device))


def check_words(words, V: int) -> np.ndarray:
    """Word ids as int64, checked on the host: a 1-D integer array with every id in [0, V);
    repeats and any order are fine."""
    words = np.asarray(words)
    if words.ndim != 1 or (words.size and words.dtype.kind not in "iu"):
        raise ValueError("words must be a 1-D array of integer word ids")
    if words.size and (words.min() < 0 or words.max() >= V):
        raise ValueError(f"words: a word id is outside [0, {V})")
    return np.ascontiguousarray(words, dtype=np.int64)


def check_groups(group_ptr, group_rows, n: int):
    """(group_ptr, group_rows) as int64, checked on the host: group g holds the rows
    group_rows[group_ptr[g] : group_ptr[g + 1]]. group_ptr must run monotonically from 0 to
    len(group_rows), every row id must lie in [0, n), and no group may be empty (its mean does not
    exist). Groups may overlap."""
    ptr, rows = np.asarray(group_ptr), np.asarray(group_rows)
    if ptr.ndim != 1 or ptr.size < 1 or ptr.dtype.kind not in "iu" or rows.ndim != 1 or \
            (rows.size and rows.dtype.kind not in "iu"):
        raise ValueError("group_ptr and group_rows must be 1-D integer arrays")
    if ptr[0] != 0 or ptr[-1] != rows.size or (np.diff(ptr) < 0).any():
        raise ValueError("group_ptr must be monotone from 0 to len(group_rows)")
    if (np.diff(ptr) == 0).any():
        raise ValueError("a group is empty")
    if rows.size and (rows.min() < 0 or rows.max() >= n):
        raise ValueError(f"group_rows: a row id is outside [0, {n})")
    return ptr.astype(np.int64), rows.astype(np.int64)


# -- Adamax -------------------------------------------------------------------------------------
class LasagneAdamax(LasagneOptimizer):
    """lasagne.updates.adamax: t += 1; a_t = lr/(1-b1^t); m = b1*m + (1-b1)*g;
    u = max(b2*u, |g|); p -= a_t*m/(u+eps). mlpconv.LasagneAdam's interface."""

    entry, second, lr = "gcg_adamax_step_f32", "u", 2e-3

    def step_size(self, t):
        return self.lr / (1 - self.beta1 ** t)


# -- the model ------------------------------------------------------------------------------
class NNModel_loc2lang(MiniBatchTrainer):
    """loc2lang.NNModel (loc2lang.py:118-292) with every product, the Gaussian layer, the loss
    and the update on the GPU.

    Network: G = bigaus_layer(X) with n_gaus_comp components; relu(G.Wh + bh) with hid_size
    units when hid_size is non-zero; the linear projection to output_size logits whose softmax
    is folded into the loss. GlorotUniform weights and zero biases, drawn in Lasagne's
    construction order on NumPy's global stream: the layer's mus and corxy (each only when the
    constructor was not given it), Wh, Wo. The parameter list has get_all_param_values' order
    [mus, sigmas, corxy, (Wh, bh,) Wo, bo] (get_params, set_params, init_parameters).
    Loss: softmax_xent_csr against the rows' l1-normalised bags of words, held on the device as
    one CSR per split and never densified. Adamax, lr 2e-3, on every parameter.

    One epoch (loc2lang.py:246-273): shuffled batches with the tail dropped; a batch's target
    rows are reached through their row ids (no slice of Y per batch); the reported train loss
    is the mean of the batch losses (each before its update), accumulated on the device; no host
    synchronisation between an epoch's first and last batch. The dev loss is the mean over all
    dev rows (loc2lang.py:257: no tail drop). A dev loss is kept when
    l_val < best and best - l_val > 1e-4 l_val; otherwise a counter runs and training stops when
    it exceeds early_stopping_max_down; the best parameters are restored. fit returns
    (perplexity_test, perplexity_dev) = 2 ** loss with the natural-log loss, as the reference
    computes it.

    Step: the Gaussian layer, the two NT GEMMs (rectify in the first one's epilogue),
    gcg_softmax_xent_csr_f32 (losses, and the gradient written over the logits), the weight
    gradients (TN GEMMs) and input gradients (NT GEMMs), the rectify backward with its column
    sums, gcg_bigaus_layer_backward_f32, one Adamax launch per parameter.

    Deviations. The loss is evaluated as sum y (logsumexp - z), finite where the reference's
    log(softmax) underflows to -inf; region_word_scores is likewise finite where the reference's
    np.log(softmax) is -inf (it never forms a probability). top_words ranks the logits, ties to the
    lower index (the reference argsorts float32 probabilities, to which distinct logits can
    round, and reverses an unstable sort). Evaluation and predict run in row chunks whose logits stay
    under 1 GiB, the row losses added in row order in float64 (the reference evaluates a split
    in one call). When no epoch satisfies the selection rule (n_epochs = 0, or a NaN loss) the
    last parameters are kept, where the reference would pass None to set_all_param_values and
    crash. The rectify passes no gradient at a pre-activation of exactly 0 (Theano: half).
    nomdn=True, a truthy reload, sparse (grid) inputs and a dtype other than float32 are
    refused; regul_coef, drop_out, dropout_coef and autoencoder are accepted and unused, as the
    reference's build uses none of them (no penalty and no dropout exist in what it executes).
    """

    def __init__(self, n_epochs=10, batch_size=1000, regul_coef=1e-6, input_size=None,
                 output_size=None, hid_size=500, drop_out=False, dropout_coef=0.5,
                 early_stopping_max_down=10, dtype="float32", autoencoder=100, reload=False,
                 n_gaus_comp=500, mus=None, sigmas=None, corxy=None, nomdn=False,
                 dataset_name="", init_parameters=None, device="cuda"):
        input_size = self._check_mode(nomdn, input_size)
        if reload:
            raise NotImplementedError("reload (a pickled model file) is not built")
        if dtype != "float32":
            raise ValueError("the GPU path computes in float32 (loc2lang.py dtype='float32')")
        if not 1 <= int(n_gaus_comp) <= self.max_units:
            raise ValueError(f"n_gaus_comp must be in [1, {self.max_units}]")
        if not 0 <= int(hid_size) <= MAX_HIDDEN:
            raise ValueError(f"hid_size must be in [0, {MAX_HIDDEN}]")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be positive")
        C = int(n_gaus_comp)
        self._check_component_args(C, mus, sigmas, corxy)
        self.n_epochs = n_epochs
        self.batch_size = int(batch_size)
        self.regul_coef = regul_coef
        self.hid_size = int(hid_size)
        self.drop_out = drop_out
        self.dropout_coef = dropout_coef
        self.early_stopping_max_down = early_stopping_max_down
        self.dtype = dtype
        self.input_size = input_size
        self.output_size = None if output_size is None else int(output_size)
        self.autoencoder = autoencoder
        self.reload = False
        self.n_gaus_comp = C
        self.mus_init, self.sigmas_init, self.corxy_init = mus, sigmas, corxy
        self.nomdn = type(self).nomdn
        self.dataset_name = dataset_name
        self.init_parameters = init_parameters
        self.device = torch.device(device)
        self.history = []
        self.params = None
        if self.output_size is not None and self.input_size is not None:
            self._build(self.output_size)  # the reference builds in its constructor

    # -- what the no-MDN baseline (NNModel_loc2lang_nomdn) states differently ---------------
    nomdn = False
    max_units = MAX_COMPONENTS  # the first layer's widest

    def _check_mode(self, nomdn, input_size) -> Optional[int]:
        """The constructor's refusals that depend on the input mode; returns input_size."""
        if nomdn:
            raise NotImplementedError("nomdn (a rectified dense layer in place of the Gaussians) "
                                      "is a class of its own: NNModel_loc2lang_nomdn")
        if input_size is not None and int(input_size) != 2:
            raise NotImplementedError("the input is a coordinate [lat, lon] (input_size 2); the "
                                      "grid representation is NNModel_loc2lang_nomdn's input")
        return 2

    @staticmethod
    def _check_component_args(C, mus, sigmas, corxy) -> None:
        for x, shape, name in ((mus, (C, 2), "mus"), (sigmas, (C, 2), "sigmas"),
                               (corxy, (C,), "corxy")):
            if x is not None and np.shape(x) != shape:
                raise ValueError(f"{name} must have shape {shape}, got {np.shape(x)}")

    def _first_layer(self, x) -> torch.Tensor:
        """The first layer's output [n, n_gaus_comp] (the reference's f_gaus)."""
        return bigaus_forward(x, self.mus, self.sigmas, self.corxy)

    def _set_train(self, x) -> None:
        """fit's training input, as _prepare_epoch gathers it per epoch."""
        self._train_data = x

    # -- model --------------------------------------------------------------------------
    @property
    def names(self):
        return ["mus", "sigmas", "corxy"] + (["Wh", "bh"] if self.hid_size else []) + ["Wo", "bo"]

    def _build(self, V: int):
        if not 1 <= V <= MAX_COLS:
            raise ValueError(f"output_size must be in [1, {MAX_COLS}]")
        C, K = self.n_gaus_comp, self.hid_size
        init = self.init_parameters
        if init is not None:
            if len(init) != len(self.names):
                raise ValueError(f"init_parameters must be [{', '.join(self.names)}], as "
                                 "lasagne.layers.get_all_param_values gives them")
            init = list(init)
        else:  # Lasagne's construction order: the Gaussian layer, the hidden layer, the output
            init = list(draw_components(C, self.mus_init, self.sigmas_init, self.corxy_init))
            if K:
                init += [_glorot_uniform(C, K), np.zeros(K, np.float32)]
            init += [_glorot_uniform(K or C, V), np.zeros(V, np.float32)]
        shapes = [(C, 2), (C, 2), (C,)] + ([(C, K), (K,)] if K else []) + [(K or C, V), (V,)]
        self.params = [self._param(x, s) for x, s in zip(init, shapes)]
        self.mus, self.sigmas, self.corxy = self.params[:3]
        self.Wh, self.bh = (self.params[3], self.params[4]) if K else (None, None)
        self.Wo, self.bo = self.params[-2], self.params[-1]
        self._proj_h, self._proj_o = dense.Projection(), dense.Projection()
        self.output_size = V
        self.optimizer = LasagneAdamax(self.params, lr=2e-3, beta1=0.9, beta2=0.999,
                                       epsilon=1e-8)

    def _features(self, x: torch.Tensor):
        """(G, H): the first layer's output and the last layer before the projection."""
        G = self._first_layer(x)
        if not self.hid_size:
            return G, G
        return G, dense.gemm_nt(G, self._proj_h.fwd.get(self.Wh, True), bias=self.bh, act="relu")

    def _logits(self, x: torch.Tensor) -> torch.Tensor:
        H = self._features(x)[1]
        return dense.gemm_nt(H, self._proj_o.fwd.get(self.Wo, True), bias=self.bo)

    def _chunk_rows(self) -> int:
        return max(1, EVAL_CHUNK_BYTES // (4 * gs.row_stride(self.output_size)) - 1)

    def _to_coords(self, X, name: str = "X") -> torch.Tensor:
        if sps.issparse(X) or isinstance(X, gs.DeviceCSR):
            raise NotImplementedError("the input is a dense [n, 2] coordinate array; the sparse "
                                      "grid representation is NNModel_loc2lang_nomdn's input")
        if isinstance(X, torch.Tensor):
            X = X.detach().cpu().numpy()
        X = np.asarray(X)
        if X.ndim != 2 or X.shape[1] != 2:
            raise ValueError(f"{name} must have shape (n, 2) [lat, lon], got {X.shape}")
        return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(self.device)

    @torch.no_grad()
    def _evaluate(self, x: torch.Tensor, Y: gs.DeviceCSR) -> float:
        """f_val (loc2lang.py:210, 257): the mean loss over every row of a split, in row chunks;
        the row losses are added in row order, in float64, on the host (one synchronisation)."""
        n, step = x.shape[0], self._chunk_rows()
        rows_all = torch.arange(n, dtype=torch.int32, device=self.device)
        losses = torch.empty(n, dtype=torch.float32, device=self.device)
        for a in range(0, n, step):
            b = min(a + step, n)
            Z = self._logits(_row_chunk(x, a, b))
            losses[a:b] = xent_csr_forward_backward(Z, Y, rows_all[a:b], want_grad=False)[0]
        return float(np.cumsum(losses.cpu().numpy().astype(np.float64))[-1] / n)

    # -- training -----------------------------------------------------------------------
    @torch.no_grad()
    def _step(self, x: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
        """One batch: the loss (device scalar) and the gradients of every parameter, then the
        Adamax update."""
        B, opt = x.shape[0], self.optimizer
        G, H = self._features(x)
        Z = dense.gemm_nt(H, self._proj_o.fwd.get(self.Wo, True), bias=self.bo)
        loss_rows, dZ = xent_csr_forward_backward(Z, self._y_train, rows, scale=1.0 / B,
                                                  in_place=True)
        loss = loss_rows.sum() / B
        self.Wo.grad = dense.gemm_tn(H, dZ)
        self.bo.grad = dZ.sum(dim=0) if dZ.shape[1] > 1024 else gs.colsum(dZ)
        dH = dense.gemm_nt(dZ, self._proj_o.bwd.get(self.Wo, False))
        if self.hid_size:
            g, self.bh.grad = gs.relu_backward(dH, Y=H, out=dH)
            self.Wh.grad = dense.gemm_tn(G, g)
            dG = dense.gemm_nt(g, self._proj_h.bwd.get(self.Wh, False))
        else:
            dG = dH
        dparams = bigaus_backward(x, self.mus, self.sigmas, self.corxy, dG)
        self.mus.grad, self.sigmas.grad, self.corxy.grad = split_dparams(dparams)
        opt.step()
        return loss

    @torch.no_grad()
    def _run_batches(self) -> torch.Tensor:
        """Device half of an epoch (the host half: MiniBatchTrainer._prepare_epoch, which
        gathers the epoch's coordinates): every batch's step, no host synchronisation. Returns
        the mean of the batch losses as a device scalar."""
        B = self.batch_size
        total = torch.zeros((), dtype=torch.float32, device=self.device)
        self.batch_losses = []
        for b in range(self._n_batches):
            loss = self._step(self._epoch_data[b * B:(b + 1) * B],
                              self._perm[b * B:(b + 1) * B])
            self.batch_losses.append(loss)
            total += loss
        return total / self._n_batches

    def _split(self, X, Y, name: str):
        x = self._to_coords(X, name)
        Yd = target_csr(Y, self.device)
        if Yd.n_rows != x.shape[0]:
            raise ValueError(f"X_{name} has {x.shape[0]} rows, Y_{name} {Yd.n_rows}")
        return x, Yd

    @torch.no_grad()
    def fit(self, X_train, Y_train, X_dev, Y_dev, X_test, Y_test, epoch_orders=None):
        """loc2lang.py:229-288. X_*: [n, 2] coordinate arrays (lat, lon); Y_*: the rows' bags of
        words, scipy sparse or dense [n, V], uploaded once as CSR. Returns
        (perplexity_test, perplexity_dev). epoch_orders (tests, measurement): one permutation of
        the training rows per epoch instead of the np.random.shuffle draws."""
        x_train, self._y_train = self._split(X_train, Y_train, "train")
        self._set_train(x_train)
        self._n_train = x_train.shape[0]
        x_dev, y_dev = self._split(X_dev, Y_dev, "dev")
        x_test, y_test = self._split(X_test, Y_test, "test")
        V = self._y_train.n_cols
        if y_dev.n_cols != V or y_test.n_cols != V:
            raise ValueError("Y_train, Y_dev and Y_test differ in width")
        if self.params is None:
            self._build(V)
        elif self.output_size != V:
            raise ValueError(f"Y_train has {V} columns, output_size says {self.output_size}")
        n_batches(self._n_train, self.batch_size)  # n < B raises
        if x_dev.shape[0] == 0 or x_test.shape[0] == 0:
            raise ValueError("the dev and test splits need at least one row")
        log.info("training with %d n_epochs and %d batch_size", self.n_epochs, self.batch_size)
        self.history, self.epoch_batch_losses = [], []
        best, best_params = run_epochs(
            lambda n: (self._train_epoch(None if epoch_orders is None else epoch_orders[n]),),
            lambda: (self._evaluate(x_dev, y_dev),), self.params, self.history, self.n_epochs,
            lower_loss_by_margin, self.early_stopping_max_down,
            after_epoch=lambda n: self.epoch_batch_losses.append(
                torch.stack(self.batch_losses).cpu().numpy()))
        self.best_val_loss = best[0]
        self.last_params = [p.detach().cpu().numpy() for p in self.params]
        if best_params is not None:  # None: no epoch qualified; keep the last parameters
            self.set_params(best_params)
        l_test = self._evaluate(x_test, y_test)
        l_dev = self._evaluate(x_dev, y_dev)
        self.test_loss, self.dev_loss = l_test, l_dev
        log.info("test loss is %f and perplexity is %f", l_test, np.power(2, l_test))
        log.info("dev loss is %f and perplexity is %f", l_dev, np.power(2, l_dev))
        return np.power(2, l_test), np.power(2, l_dev)

    # -- reference API ------------------------------------------------------------------
    def _built(self):
        if self.params is None:
            raise RuntimeError("the model has no parameters yet: give output_size or call fit")

    @torch.no_grad()
    def predict(self, X) -> np.ndarray:
        """f_predict_proba (loc2lang.py:290-292): [n, V] word probabilities for every row of X,
        as a NumPy array, computed in row chunks."""
        self._built()
        x = self._to_coords(X)
        n, step = x.shape[0], self._chunk_rows()
        out = np.empty((n, self.output_size), np.float32)
        for a in range(0, n, step):
            Z = self._logits(_row_chunk(x, a, min(a + step, n)))
            out[a:a + step] = softmax_wide(Z, out=Z).cpu().numpy()
        return out

    @torch.no_grad()
    def gaus_output(self, X) -> np.ndarray:
        """f_gaus (loc2lang.py:208): the Gaussian layer's output [n, n_gaus_comp]."""
        self._built()
        return self._first_layer(self._to_coords(X)).cpu().numpy()

    # -- the analyses (loc2lang.py:516-614, 693-766) ------------------------------------------------
    def _scan(self, x: torch.Tensor, per_chunk) -> None:
        """The one pass over the rows of x that every analysis shares: per chunk of _chunk_rows()
        rows the logits once, their row_lse, then per_chunk(a, b, Z, lse) for the rows [a, b). No
        host synchronisation; the chunk's logits are dropped before the next chunk's exist."""
        n, step = x.shape[0], self._chunk_rows()
        for a in range(0, n, step):
            b = min(a + step, n)
            Z = self._logits(_row_chunk(x, a, b))
            per_chunk(a, b, Z, row_lse(Z))

    @torch.no_grad()
    def word_entropies(self, X) -> torch.Tensor:
        """float64 [V] on the device: the entropy (natural log, 0 log 0 = 0) of every word's
        predicted probability over the rows of X after l1-normalising it over those rows -- what
        get_local_words sorts (loc2lang.py:757-758) -- as log S - T / S from the column sums
        S = sum_n p, T = sum_n p log p; NaN where S == 0."""
        self._built()
        x = self._to_coords(X)
        S = torch.zeros(self.output_size, dtype=torch.float64, device=self.device)
        T = torch.zeros_like(S)
        self._scan(x, lambda a, b, Z, lse: softmax_column_stats(Z, lse, S, T))
        return torch.where(S == 0, torch.full_like(S, float("nan")), torch.log(S) - T / S)

    def local_words(self, X, k: int = 50) -> np.ndarray:
        """local_words(self.predict(X), k) without the [n, V] array: the indices of the k lowest
        word_entropies, ascending, stable."""
        return torch.argsort(self.word_entropies(X), stable=True)[:int(k)].cpu().numpy()

    @torch.no_grad()
    def word_probabilities(self, X, words, as_tensor: bool = False):
        """predict(X)[:, words] as float32 [n, len(words)] (the input of contour_me for the plotted
        words, loc2lang.py:747-753): the columns gathered from each chunk's own logits,
        exp(z - lse). words: host word ids in [0, V), any order, repeats allowed. A NumPy array,
        or the device tensor with as_tensor."""
        self._built()
        x = self._to_coords(X)
        w = torch.from_numpy(check_words(words, self.output_size)).to(self.device)
        out = torch.empty((x.shape[0], w.numel()), dtype=torch.float32, device=self.device)

        def gather(a, b, Z, lse):
            out[a:b] = torch.exp(Z[:, w].to(torch.float64) - lse[:, None])

        self._scan(x, gather)
        return out if as_tensor else out.cpu().numpy()

    @torch.no_grad()
    def top_words(self, X, k: int) -> np.ndarray:
        """[n, k] int64: per row of X its k most probable words, the most probable first
        (np.argsort(preds)[0][::-1][:k], loc2lang.py:701). Ranked on the logits (softmax is
        monotone), ties to the lower index: a stable descending sort of each chunk in torch."""
        self._built()
        k = int(k)
        if not 1 <= k <= self.output_size:
            raise ValueError(f"k must be in [1, {self.output_size}]")
        x = self._to_coords(X)
        out = torch.empty((x.shape[0], k), dtype=torch.int64, device=self.device)

        def top(a, b, Z, lse):
            out[a:b] = torch.sort(Z, dim=1, descending=True, stable=True)[1][:, :k]

        self._scan(x, top)
        return out.cpu().numpy()

    @torch.no_grad()
    def region_word_scores(self, X, group_ptr, group_rows) -> torch.Tensor:
        """float32 [G, V] on the device: dialect_normalized_logprobs (loc2lang.py:569-579) of
        every group of rows of X, mean_{n in g} log p_nv - mean_n log p_nv. The logits are linear
        in the last hidden layer h, so this is ((mean_g h - mean h) . Wo)_v - (mean_g lse - mean
        lse): the scan gives lse, _features gives h (the Gaussian layer's output when hid_size is
        0), the means are taken in float64 and one [G, hid] x [hid, V] GEMM does the rest. Group g
        holds the rows group_rows[group_ptr[g] : group_ptr[g + 1]] (check_groups); groups may
        overlap. Finite where the reference's np.log(softmax) underflows to -inf."""
        self._built()
        x = self._to_coords(X)
        n = x.shape[0]
        if n == 0:
            raise ValueError("X has no rows")
        ptr, rows = check_groups(group_ptr, group_rows, n)
        G = ptr.size - 1
        # [G + 1, n] float64 weights: row g holds 1 / |g| per member (a row twice counts twice, as
        # np.mean over the reference's index list would), the last row 1 / n: the global mean
        A = np.zeros((G + 1, n), np.float64)
        np.add.at(A, (np.repeat(np.arange(G), np.diff(ptr)), rows), 1.0)
        A[:G] /= np.diff(ptr)[:, None]
        A[G] = 1.0 / n
        A = torch.from_numpy(A).to(self.device)
        lse = torch.empty(n, dtype=torch.float64, device=self.device)

        def keep(a, b, Z, l):
            lse[a:b] = l

        self._scan(x, keep)
        H = self._features(x)[1]
        means = A @ torch.cat([H.to(torch.float64), lse[:, None]], dim=1)
        d = means[:G] - means[G]
        dh = gs.empty_dense(G, H.shape[1], self.device)
        dh.copy_(d[:, :-1])
        scores = dense.gemm_nt(dh, self._proj_o.fwd.get(self.Wo, True))
        return scores.sub_(d[:, -1:].to(torch.float32))

    def get_params(self):
        self._built()
        return [p.detach().cpu().numpy() for p in self.params]

    def set_params(self, params):
        """loc2lang.py:214-215."""
        self._built()
        if len(params) != len(self.params):
            raise ValueError(f"expected [{', '.join(self.names)}]")
        with torch.no_grad():
            for p, v in zip(self.params, params):
                p.copy_(_as_tensor(v, tuple(p.shape), self.device))


class NNModel_loc2lang_nomdn(NNModel_loc2lang):
    """The baseline the Gaussian layer is compared against: loc2lang.NNModel with nomdn=True
    (loc2lang.py:167-171), a rectified dense layer of n_gaus_comp units (the reference keeps that
    name) where the Gaussians were. Everything else is NNModel_loc2lang's: the epoch loop, the
    selection rule, the loss, the chunked evaluation, predict and the analyses.

    Network: G = rectify(X.Wg + bg); relu(G.Wh + bh) when hid_size is non-zero; the projection to
    output_size logits. The parameter list is [Wg, bg, (Wh, bh,) Wo, bo] (get_params, set_params,
    init_parameters, names); GlorotUniform weights drawn in Lasagne's construction order Wg, Wh, Wo
    on NumPy's global stream, zero biases. Adamax, lr 2e-3, on every parameter.

    Input. Sparse -- a scipy CSR or a DeviceCSR, input_size = its width: the grid representation
    (grid.grid_representation), the reference's `-nomdn` with a grid. Or a dense [n, input_size]
    array: the reference's `-nomdn` on raw coordinates, input_size 2. input_size=None takes the
    width at fit. fit, predict, gaus_output and every analysis take either kind (a sparse input
    goes through in row chunks, DeviceCSR.row_slice); a width other than the model's is a
    ValueError.

    The sparse epoch is mlp.MLP's: the epoch's batches are segmented by column on the device
    (mlp.BatchSegments, one per run of plan_segmented_epoch), the forward of a batch is
    spmm_rows(X, Wg, bg, rows, act="relu"), and the step runs the rectify backward with its
    column sums for bg, then Wg's whole update in one pass over Wg, m, u
    (gcg_minibatch_w1_adamax_step_f32: no input_size x n_gaus_comp gradient exists; a row of Wg
    that no training row touches keeps its bits), then one Adamax launch for each other
    parameter, on the same step count. No host synchronisation between an epoch's first and
    last batch.

    With a dense input the first layer and its gradients are plain torch ops (addmm, relu, the
    transposed product): the inner dimension is the input's width, 2, and nothing there is hot.

    mus, sigmas and corxy are accepted and unused, as the reference's nomdn build ignores them;
    reload and a dtype other than float32 are refused as in NNModel_loc2lang. Left out: another
    first-layer activation (the reference's log line says tanh, its code rectifies)."""

    nomdn = True
    max_units = MAX_HIDDEN  # the first layer is rectified: the rectify backward's one-pass kernel

    def __init__(self, *args, **kw):
        self._inputs = {}   # MiniBatchTrainer._input's upload cache
        self._sparse = False
        super().__init__(*args, **kw)

    def _check_mode(self, nomdn, input_size) -> Optional[int]:
        if input_size is None:
            return None
        if int(input_size) < 1:
            raise ValueError("input_size must be positive")
        self.in_size = int(input_size)  # what MiniBatchTrainer._input checks a sparse X against
        return self.in_size

    @staticmethod
    def _check_component_args(C, mus, sigmas, corxy) -> None:
        pass

    @property
    def names(self):
        return ["Wg", "bg"] + (["Wh", "bh"] if self.hid_size else []) + ["Wo", "bo"]

    def _build(self, V: int):
        if not 1 <= V <= MAX_COLS:
            raise ValueError(f"output_size must be in [1, {MAX_COLS}]")
        F, C, K = self.input_size, self.n_gaus_comp, self.hid_size
        init = self.init_parameters
        if init is not None:
            if len(init) != len(self.names):
                raise ValueError(f"init_parameters must be [{', '.join(self.names)}], as "
                                 "lasagne.layers.get_all_param_values gives them")
            init = list(init)
        else:  # Lasagne's construction order: the first layer, the hidden layer, the output
            init = [_glorot_uniform(F, C), np.zeros(C, np.float32)]
            if K:
                init += [_glorot_uniform(C, K), np.zeros(K, np.float32)]
            init += [_glorot_uniform(K or C, V), np.zeros(V, np.float32)]
        shapes = [(F, C), (C,)] + ([(C, K), (K,)] if K else []) + [(K or C, V), (V,)]
        self.params = [self._param(x, s) for x, s in zip(init, shapes)]
        self.Wg, self.bg = self.params[:2]
        self.Wh, self.bh = (self.params[2], self.params[3]) if K else (None, None)
        self.Wo, self.bo = self.params[-2], self.params[-1]
        self._proj_h, self._proj_o = dense.Projection(), dense.Projection()
        self.output_size = V
        # one optimiser for every parameter: on a sparse input Wg's m and u are updated inside
        # the one-pass step and the launches cover the others, on the same step count
        self.optimizer = LasagneAdamax(self.params, lr=2e-3, beta1=0.9, beta2=0.999,
                                       epsilon=1e-8)

    def _first_layer(self, x, rows=None) -> torch.Tensor:
        """rectify(X.Wg + bg) of the rows of x (every row, or the int32 device row ids `rows` of
        a sparse x), in the padded layout the GEMMs take."""
        if isinstance(x, gs.DeviceCSR):
            return gs.spmm_rows(x, self.Wg, self.bg, rows, act="relu")
        G = gs.empty_dense(x.shape[0], self.n_gaus_comp, self.device)
        return G.copy_(torch.relu(torch.addmm(self.bg, x, self.Wg)))

    def _to_coords(self, X, name: str = "X"):
        """A model input on the device: a DeviceCSR for a sparse X, a float32 [n, input_size]
        tensor for a dense one; the first input fixes an input_size left open."""
        if sps.issparse(X) or isinstance(X, gs.DeviceCSR):
            if self.input_size is None:
                self.input_size = self.in_size = int(X.shape[1])
            return self._input(X)
        if isinstance(X, torch.Tensor):
            X = X.detach().cpu().numpy()
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError(f"{name} must have shape (n, input_size), got {X.shape}")
        if self.input_size is None:
            self.input_size = self.in_size = int(X.shape[1])
        if X.shape[1] != self.input_size:
            raise ValueError(f"X has {X.shape[1]} columns, the model {self.input_size}")
        return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(self.device)

    def _set_train(self, x) -> None:
        self._sparse = isinstance(x, gs.DeviceCSR)
        self._x_train = x
        if not self._sparse:
            self._train_data = x
            return
        # the rows are reached through their ids; every segmentation call is sized from the
        # host's copy of indptr (copied once)
        self._indptr_host = x.indptr.cpu().numpy().astype(np.int64)
        self._train_data = torch.arange(x.n_rows, dtype=torch.int32, device=self.device)

    def _plan_epoch(self, order: np.ndarray) -> np.ndarray:
        if self._sparse:
            return plan_segmented_epoch(self, order)
        return super()._plan_epoch(order)

    # -- training -----------------------------------------------------------------------
    @torch.no_grad()
    def _step(self, x, rows: torch.Tensor, seg=None, b: int = 0) -> torch.Tensor:
        """One batch: x is the batch's [B, input_size] rows, or with `seg` (the run's
        BatchSegments, b the batch's index in it) the sparse training input, `rows` its row ids.
        The loss (device scalar), every gradient, then the Adamax update."""
        B, opt = rows.numel(), self.optimizer
        G = self._first_layer(x, rows if seg is not None else None)
        H = G
        if self.hid_size:
            H = dense.gemm_nt(G, self._proj_h.fwd.get(self.Wh, True), bias=self.bh, act="relu")
        Z = dense.gemm_nt(H, self._proj_o.fwd.get(self.Wo, True), bias=self.bo)
        loss_rows, dZ = xent_csr_forward_backward(Z, self._y_train, rows, scale=1.0 / B,
                                                  in_place=True)
        loss = loss_rows.sum() / B
        self.Wo.grad = dense.gemm_tn(H, dZ)
        self.bo.grad = dZ.sum(dim=0) if dZ.shape[1] > 1024 else gs.colsum(dZ)
        dH = dense.gemm_nt(dZ, self._proj_o.bwd.get(self.Wo, False))
        if self.hid_size:
            g, self.bh.grad = gs.relu_backward(dH, Y=H, out=dH)
            self.Wh.grad = dense.gemm_tn(G, g)
            dG = dense.gemm_nt(g, self._proj_h.bwd.get(self.Wh, False))
        else:
            dG = dH
        gG, self.bg.grad = gs.relu_backward(dG, Y=G, out=dG)
        if seg is None:
            self.Wg.grad = x.t() @ gG
            opt.step()
            return loss
        opt.prepare()
        w1_adamax_step(self.Wg, opt.m[0], opt.u[0], gG, seg, b, opt.a_t, opt.beta1, opt.beta2,
                       opt.eps)
        opt.apply(first=1)
        return loss

    @torch.no_grad()
    def _run_batches(self) -> torch.Tensor:
        if not self._sparse:
            return super()._run_batches()
        B, X = self.batch_size, self._x_train
        total = torch.zeros((), dtype=torch.float32, device=self.device)
        self.batch_losses = []
        for first, stop, nnz_sel in self._runs:
            seg = BatchSegments(X, self._perm[first * B:stop * B], B, nnz_sel)
            for b in range(first, stop):
                # the order was checked on the host (a permutation of the training rows)
                loss = self._step(X, self._perm[b * B:(b + 1) * B], seg, b - first)
                self.batch_losses.append(loss)
                total += loss
        return total / self._n_batches

    @torch.no_grad()
    def gaus_output(self, X) -> np.ndarray:
        """f_gaus (loc2lang.py:208): the first layer's output [n, n_gaus_comp], in row chunks."""
        self._built()
        x = self._to_coords(X)
        n, step = x.shape[0], self._chunk_rows()
        out = np.empty((n, self.n_gaus_comp), np.float32)
        for a in range(0, n, step):
            out[a:a + step] = self._first_layer(_row_chunk(x, a, min(a + step, n))).cpu().numpy()
        return out


NNModel = NNModel_loc2lang  # the reference's name for it


def local_words(preds, k: int = 50) -> np.ndarray:
    """get_local_words (loc2lang.py:755-766) without the vocabulary and the named-entity filter:
    the columns of preds [n, V] (a word's probability at n places) are l1-normalised over the
    rows, each column's entropy is taken (scipy.stats.entropy: natural log, 0 log 0 = 0), and
    the indices of the k lowest entropies are returned in ascending order of entropy (stable).
    Plain torch, float64: not a hot path."""
    p = torch.as_tensor(np.asarray(preds) if not isinstance(preds, torch.Tensor) else preds)
    if p.dim() != 2:
        raise ValueError("preds must be [n, V]")
    p = p.to(torch.float64)
    norm = p.abs().sum(dim=0, keepdim=True)
    p = p / torch.where(norm == 0, torch.ones_like(norm), norm)  # sklearn leaves a zero column
    ent = -torch.special.xlogy(p, p).sum(dim=0)
    ent = torch.where(norm[0] == 0, torch.full_like(ent, float("nan")), ent)  # entropy of 0 / 0
    return torch.argsort(ent, stable=True)[:int(k)].cpu().numpy()


def region_recall(scores, gold_ptr, gold_word,
                  fractions=(0.01, 0.05, 0.1, 0.15, 0.2)) -> RegionRecall:
    """The recall lines of state_dialect_words (loc2lang.py:587-614) from scores [G, V] (the
    model's region_word_scores; any torch tensor or array, on any device) and the regions' gold
    words: group g's are gold_word[gold_ptr[g] : gold_ptr[g + 1]] (host arrays: ids in [0, V),
    none twice in a group).

    ks[i] = int(fractions[i] * V), as the reference truncates it (0 for a small V: no word is
    retrieved). rank(g, w) = #{v : s_gv > s_gw} + #{v > w : s_gv == s_gw}: w's position in
    reversed(argsort(s_g)) under a stable sort (the reference's argsort is unstable; a NaN score
    sorts as the largest, as in NumPy). A group's recall at k is the share of its gold words with
    rank < k; groups without gold words are skipped (covered_dialects) and hold NaN.

    RegionRecall(ks, recall, oracle, per_group, ranks): recall[i] the mean over the remaining
    groups at ks[i] and oracle[i] the reference's "oracle" line, mean min(k, |gold_g|) / |gold_g|
    (both NaN when no group has gold words); per_group float64 [len(ks), G]; ranks int64
    [len(gold_word)]. Plain torch: a sort per covered group, not a hot path."""
    s = scores if isinstance(scores, torch.Tensor) else torch.as_tensor(np.asarray(scores))
    if s.dim() != 2:
        raise ValueError("scores must be [G, V]")
    G, V = s.shape
    ptr, words = np.asarray(gold_ptr), np.asarray(gold_word)
    if ptr.ndim != 1 or ptr.size != G + 1 or ptr.dtype.kind not in "iu" or words.ndim != 1 or \
            (words.size and words.dtype.kind not in "iu"):
        raise ValueError(f"gold_ptr must be {G + 1} integers and gold_word a 1-D integer array")
    if ptr[0] != 0 or ptr[-1] != words.size or (np.diff(ptr) < 0).any():
        raise ValueError("gold_ptr must be monotone from 0 to len(gold_word)")
    if words.size and (words.min() < 0 or words.max() >= V):
        raise ValueError(f"gold_word: a word id is outside [0, {V})")
    fractions = [float(f) for f in fractions]
    if any(not 0 <= f <= 1 for f in fractions):
        raise ValueError("fractions must lie in [0, 1]")
    ptr, words = ptr.astype(np.int64), words.astype(np.int64)
    ks = [int(f * V) for f in fractions]
    ranks = np.zeros(words.size, np.int64)
    per_group = np.full((len(ks), G), np.nan)
    oracle = np.full((len(ks), G), np.nan)
    for g in range(G):
        w = words[ptr[g]:ptr[g + 1]]
        if w.size == 0:
            continue
        if np.unique(w).size != w.size:
            raise ValueError(f"gold_word: group {g} holds a word twice")
        order = torch.argsort(s[g], stable=True)  # ascending; reversed: ties to the higher index
        place = torch.empty_like(order)
        place[order] = torch.arange(V, device=s.device)
        r = (V - 1 - place[torch.as_tensor(w, device=s.device)]).cpu().numpy()
        ranks[ptr[g]:ptr[g + 1]] = r
        for i, k in enumerate(ks):
            per_group[i, g] = float((r < k).sum()) / w.size
            oracle[i, g] = float(min(k, w.size)) / w.size
    covered = np.diff(ptr) > 0
    if covered.any():
        recall = [float(per_group[i, covered].mean()) for i in range(len(ks))]
        best = [float(oracle[i, covered].mean()) for i in range(len(ks))]
    else:
        recall = best = [float("nan")] * len(ks)
    return RegionRecall(ks, recall, best, per_group, ranks)
