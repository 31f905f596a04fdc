"""MLP -- the reference's mini-batch trainer (mlp.py:96-311) with every product on the GPU.

The model tensormain.main_justinputconv trains (tensormain.py:79-150): the features are
pre-multiplied once, X_conv = H * X (`input_convolution`, the HIP SpGEMM), then a sparse-input
MLP -- rectify(X.W1 + b1) (SparseInputDenseLayer), softmax(h.W2 + b2) -- is trained on
shuffled mini-batches (mlp.py:77-92, 268-270) with lasagne.updates.adam(lr=0.002) (mlp.py:244).

One epoch:
  order     np.random.shuffle(np.arange(n)) from numpy's global stream; batches are
            order[s:s+B] for s in range(0, n-B+1, B), the tail is dropped (mlp.py:81-91)
  segment   the column grouping of all the epoch's batches at once, on the device
            (gcg_minibatch_segment): per batch the touched columns of X[batch] and, per column,
            the (row position, value) entries -- (X[batch])^T without building it per step
  step      h = rectify(X[batch].W1 + b1) with gate bytes (plan-less HIP SpMM over the batch's
            rows), the fused MFMA output layer + loss and its gradients (dense), the rectify
            backward + db1 (one pass), then ONE pass over W1 (gcg_minibatch_w1_step_f32): the
            data gradient of the rows the batch touches, the L1/L2 penalty gradient and Adam,
            with no F x K gradient in memory; b1, W2, b2 through gcg_adam_step_f32.
No host synchronisation happens between the first and the last batch of an epoch.

Validation: the reference runs f_val on dev after every batch and uses the last one of the
epoch (mlp.py:271-280); here it runs once per epoch, after the last batch. Model selection is
mlp.py:272-285: strict acc_val > best_val_acc keeps the parameters, otherwise a counter runs up
to early_stopping_max_down; the best parameters are restored (the last ones when no epoch ever
improved -- the reference would crash on None there).

DropoutMLP is the same trainer with the reference's drop_out=True: Philox masks on the input
(applied where the epoch is segmented) and, as an option, on the hidden output.

Left out, as MLPCONV leaves them: complete_prob (soft labels), dense inputs; with dropout also
add_hidden=False.
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np
import scipy.sparse as sps
import torch
from torch.autograd.graph import increment_version

from . import dense
from . import dropout as _drop
from . import sparse as gs
from ._native import call
from .layers import _as_device_csr, _glorot_uniform
from .mlpconv import LasagneAdam
from .sparse import _ld, _ptr, _stream_handle
from .training import MiniBatchTrainer, higher_accuracy, n_batches, restore, run_epochs

log = logging.getLogger(__name__)

# Entries (selected nonzeros) segmented per gcg_minibatch_segment call: an epoch with more is cut
# into runs of whole batches (the sizes come from the host's copy of indptr, so a run boundary
# costs no synchronisation). 2^26 entries need ~2.2 GB of keys, payloads and outputs.
SEGMENT_CHUNK_ENTRIES = 1 << 26


def iterate_minibatch_indices(n: int, batchsize: int, shuffle: bool = True):
    """The index lists of mlp.py:81-91 (iterate_minibatches): one np.random.shuffle of
    arange(n) from numpy's global stream, then order[s:s+B] for s in range(0, n-B+1, B); the
    tail is dropped. Returns the list of batches."""
    order = np.arange(n)
    if shuffle:
        np.random.shuffle(order)
    return [order[s:s + batchsize] for s in range(0, n - batchsize + 1, batchsize)]


def output_size(Y_train) -> int:
    """out_size = len(set(Y_train)) (mlp.py:132) -- the number of distinct labels, not max+1."""
    return len(set(np.asarray(Y_train).tolist()))


def default_hidden_size(out_size: int, in_size: int) -> int:
    """mlp.py:138."""
    return min(5 * out_size, int(in_size / 20))


def input_convolution(H, X, device="cuda") -> gs.DeviceCSR:
    """X_conv = H * X, then .tocsr().astype('float32') (tensormain.py:114-115), on the GPU
    (sparse.spgemm: every entry summed in scipy's order, canonical output). A float64 scipy H --
    the reference's D^-1/2 A D^-1/2 is float64 there -- accumulates in float64 as scipy's
    upcast does; a float32 H or a DeviceCSR in float32."""
    Xd = _as_device_csr(X, device)
    if isinstance(H, gs.DeviceCSR):
        return gs.spgemm(H, Xd)
    if not sps.issparse(H):
        raise ValueError("Input for this layer must be sparse")
    Hc = H.tocsr()
    if Hc.dtype == np.float64:
        Hd = gs.DeviceCSR.from_scipy(Hc.astype(np.float32), Xd.device)
        return gs.spgemm(Hd, Xd, a_data64=torch.from_numpy(np.ascontiguousarray(Hc.data))
                         .to(Xd.device))
    return gs.spgemm(gs.DeviceCSR.from_scipy(Hc, Xd.device), Xd)


def plan_epoch(order, indptr_host: np.ndarray, batch: int):
    """Host half of an epoch's segmentation: (perm, runs, n_batches). perm is the order cut to
    whole batches (int64, range-checked); runs are (first batch, stop batch, selected entries)
    triples, greedy runs of whole batches under SEGMENT_CHUNK_ENTRIES, one segmentation call
    each. The sizes come from the host's copy of indptr: no synchronisation."""
    n = indptr_host.size - 1
    order = np.asarray(order)
    if order.ndim != 1 or order.size != n:
        raise ValueError(f"an epoch's order must list the {n} training rows")
    nb = n_batches(n, batch)
    perm = np.ascontiguousarray(order[:nb * batch], dtype=np.int64)
    if perm.min() < 0 or perm.max() >= n:
        raise IndexError("epoch order out of range")
    lens = indptr_host[perm + 1] - indptr_host[perm]
    per_batch = lens.reshape(nb, batch).sum(axis=1)
    runs, start, acc = [], 0, 0
    for b in range(nb):
        if b > start and acc + int(per_batch[b]) > SEGMENT_CHUNK_ENTRIES:
            runs.append((start, b, acc))
            start, acc = b, 0
        acc += int(per_batch[b])
    runs.append((start, nb, acc))
    return perm, runs, nb


def plan_segmented_epoch(self, order) -> np.ndarray:
    """MiniBatchTrainer._plan_epoch of the sparse-input trainers: plan_epoch's cut, kept on the
    host too (`_perm_host`, which tools/bench_mlp.py reads), and its runs (`_runs`)."""
    self._perm_host, self._runs, _ = plan_epoch(order, self._indptr_host, self.batch_size)
    return self._perm_host


class BatchSegments:
    """The column grouping of a run of consecutive batches (gcg_minibatch_segment): batch b of
    the run owns segments batch_seg_ptr[b] .. batch_seg_ptr[b+1]; segment s has column
    seg_col[s] and entries seg_ptr[s] .. seg_ptr[s+1] of (ent_pos, ent_val).

    drop (a dropout.DropoutSpec) with vals_drop (float32[X.nnz]): input dropout on X at
    segmentation (gcg_minibatch_segment_dropout). Batch b of the run is masked under step
    s0 + b, s0 the stream's current step (`first_step`); ent_val holds the masked values and
    vals_drop receives them at the selected rows' CSR slots, for the forward. The stream is
    advanced by the run's number of batches afterwards."""

    def __init__(self, X: gs.DeviceCSR, perm: torch.Tensor, batch: int, nnz_sel: int,
                 drop=None, vals_drop: torch.Tensor = None):
        gs._require_cuda(perm, "perm")
        if perm.dtype != torch.int32 or perm.dim() != 1 or not perm.is_contiguous():
            raise TypeError("perm must be a contiguous 1-D int32 tensor")
        n_sel = perm.numel()
        dev = X.device
        cap, nb = C.c_int64(), C.c_size_t()
        with torch.cuda.device(dev):
            call("gcg_minibatch_segment_sizes", n_sel, batch, X.n_cols, nnz_sel, C.byref(cap),
                 C.byref(nb))
            self.n_batches = n_sel // batch
            self.batch = batch
            self.nnz_sel = nnz_sel
            self.batch_seg_ptr = torch.empty(self.n_batches + 1, dtype=torch.int32, device=dev)
            self.seg_col = torch.empty(cap.value, dtype=torch.int32, device=dev)
            self.seg_ptr = torch.empty(cap.value + 1, dtype=torch.int32, device=dev)
            self.ent_pos = torch.empty(max(nnz_sel, 1), dtype=torch.int32, device=dev)
            self.ent_val = torch.empty(max(nnz_sel, 1), dtype=torch.float32, device=dev)
            ws = torch.empty((nb.value + 7) // 8, dtype=torch.int64, device=dev)
            if drop is None:
                call("gcg_minibatch_segment", X.n_rows, X.n_cols, _ptr(X.indptr),
                     _ptr(X.indices), _ptr(X.data), _ptr(perm), n_sel, batch, nnz_sel,
                     _ptr(self.batch_seg_ptr), _ptr(self.seg_col), _ptr(self.seg_ptr),
                     _ptr(self.ent_pos), _ptr(self.ent_val), _ptr(ws), ws.numel() * 8,
                     _stream_handle(dev))
                return
            gs._require_cuda(vals_drop, "vals_drop")
            if vals_drop.dtype != torch.float32 or vals_drop.numel() != X.nnz or \
                    not vals_drop.is_contiguous():
                raise ValueError("vals_drop must be a contiguous float32[nnz] device tensor")
            stream = drop.stream
            if stream.step < 0:  # a fresh stream: step 0 is what its device scalar holds
                stream.set_step(0)
            self.first_step = stream.step
            call("gcg_minibatch_segment_dropout", X.n_rows, X.n_cols, _ptr(X.indptr),
                 _ptr(X.indices), _ptr(X.data), _ptr(perm), n_sel, batch, nnz_sel,
                 _ptr(self.batch_seg_ptr), _ptr(self.seg_col), _ptr(self.seg_ptr),
                 _ptr(self.ent_pos), _ptr(self.ent_val), _ptr(vals_drop), _ptr(ws),
                 ws.numel() * 8, *drop.abi(), _stream_handle(dev))
            stream.set_step(self.first_step + self.n_batches)


def w1_step(W: torch.Tensor, m: torch.Tensor, v: torch.Tensor, G: torch.Tensor,
            seg: BatchSegments, b: int, l1: float, l2: float, a_t: torch.Tensor,
            beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8) -> None:
    """The W1 update of batch b of `seg` in one pass over W, m, v (gcg_minibatch_w1_step_f32):
    g = (X[batch])^T . G + l1 sgn(W) + 2 l2 W, then Lasagne Adam with the step size a_t (device
    scalar). G: [batch, K] float32 with unit column stride."""
    for t, name in ((W, "W"), (m, "m"), (v, "v")):
        gs._require_cuda(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != W.shape:
            raise TypeError("w1_step needs contiguous float32 W, m, v of one shape")
    F, K = W.shape
    if G.dtype != torch.float32 or G.shape != (seg.batch, K) or (K > 1 and G.stride(1) != 1):
        raise ValueError(f"G must be float32 [{seg.batch}, {K}] with unit column stride")
    if not 0 <= b < seg.n_batches:
        raise IndexError("batch index out of range")
    with torch.cuda.device(W.device):
        call("gcg_minibatch_w1_step_f32", F, K, _ptr(W), _ptr(m), _ptr(v), _ptr(G), _ld(G),
             seg.batch, C.c_void_p(seg.batch_seg_ptr.data_ptr() + 4 * b), _ptr(seg.seg_col),
             _ptr(seg.seg_ptr), _ptr(seg.ent_pos), _ptr(seg.ent_val), float(l1), float(l2),
             _ptr(a_t), float(beta1), float(beta2), float(eps), _stream_handle(W.device))
    increment_version(W)
    increment_version(m)
    increment_version(v)


def w1_adamax_step(W: torch.Tensor, m: torch.Tensor, u: torch.Tensor, G: torch.Tensor,
                   seg: BatchSegments, b: int, a_t: torch.Tensor, beta1: float = 0.9,
                   beta2: float = 0.999, eps: float = 1e-8) -> None:
    """w1_step with the second update rule (gcg_minibatch_w1_adamax_step_f32): g = (X[batch])^T . G
    with no penalty, then Lasagne Adamax (m, u) with the step size a_t (device scalar) -- the
    sparse (grid) first layer of loc2lang's no-MDN baseline."""
    for t, name in ((W, "W"), (m, "m"), (u, "u")):
        gs._require_cuda(t, name)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != W.shape:
            raise TypeError("w1_adamax_step needs contiguous float32 W, m, u of one shape")
    F, K = W.shape
    if G.dtype != torch.float32 or G.shape != (seg.batch, K) or (K > 1 and G.stride(1) != 1):
        raise ValueError(f"G must be float32 [{seg.batch}, {K}] with unit column stride")
    if not 0 <= b < seg.n_batches:
        raise IndexError("batch index out of range")
    with torch.cuda.device(W.device):
        call("gcg_minibatch_w1_adamax_step_f32", F, K, _ptr(W), _ptr(m), _ptr(u), _ptr(G), _ld(G),
             seg.batch, C.c_void_p(seg.batch_seg_ptr.data_ptr() + 4 * b), _ptr(seg.seg_col),
             _ptr(seg.seg_ptr), _ptr(seg.ent_pos), _ptr(seg.ent_val), _ptr(a_t), float(beta1),
             float(beta2), float(eps), _stream_handle(W.device))
    increment_version(W)
    increment_version(m)
    increment_version(u)


class MLP(MiniBatchTrainer):
    permutation_only = False  # the reference's order is one, but any in-range order trains
    _plan_epoch = plan_segmented_epoch

    def __init__(self, n_epochs=10, batch_size=1000, init_parameters=None, complete_prob=False,
                 add_hidden=True, regul_coefs=(5e-5, 5e-5), save_results=False,
                 hidden_layer_size=None, drop_out=False, drop_out_coefs=(0.5, 0.5),
                 early_stopping_max_down=100000, loss_name="log", nonlinearity="rectify",
                 device="cuda"):
        if complete_prob:
            raise NotImplementedError("complete_prob (soft labels) is not built")
        if drop_out:
            raise NotImplementedError("MLP trains without dropout: drop_out=True is the class "
                                      "DropoutMLP")
        if loss_name != "log":
            raise NotImplementedError("only the 'log' (categorical cross-entropy) loss is built")
        self.n_epochs = n_epochs
        self.batch_size = int(batch_size)
        self.init_parameters = init_parameters
        self.complete_prob = False
        self.add_hidden = bool(add_hidden)
        self.regul_coefs = list(regul_coefs)
        self.save_results = save_results
        self.hidden_layer_size = hidden_layer_size
        self.drop_out = False
        self.drop_out_coefs = list(drop_out_coefs)
        self.early_stopping_max_down = early_stopping_max_down
        self.loss_name = loss_name
        self.nonlinearity = "rectify"  # the reference forces rectify (mlp.py:123)
        self.device = torch.device(device)
        self.history = []
        # measurement hook (tools/bench_mlp.py): f(self, batch index, G, l1, l2) replaces the
        # fused W1 step
        self._w1_update = None
        self._inputs = {}

    # -- model --------------------------------------------------------------------------
    def _build(self, in_size: int, out_size: int):
        K = self.hidden_layer_size if self.add_hidden else out_size
        init = self.init_parameters
        if init is not None and len(init) != (4 if self.add_hidden else 2):
            raise ValueError("init_parameters must be [W1, b1, W2, b2] (or [W, b] without a "
                             "hidden layer), as lasagne.layers.get_all_param_values gives them")
        param = self._param
        # Lasagne GlorotUniform draws W1 then W2 from numpy's global stream, b = Constant(0.);
        # _construct_dropout: where the reference constructs a dropout layer (DropoutMLP draws
        # its seed there, from the same stream)
        self._construct_dropout("input")
        W1 = _glorot_uniform(in_size, K) if init is None else init[0]
        self.W1 = param(W1, (in_size, K))
        self.b1 = param(np.zeros(K, np.float32) if init is None else init[1], (K,))
        self.params = [self.W1, self.b1]
        if self.add_hidden:
            self._construct_dropout("hidden")
            W2 = _glorot_uniform(K, out_size) if init is None else init[2]
            self.W2 = param(W2, (K, out_size)).requires_grad_(True)
            self.b2 = param(np.zeros(out_size, np.float32) if init is None else init[3],
                            (out_size,)).requires_grad_(True)
            self.params += [self.W2, self.b2]
        self.in_size, self.out_size, self.width = in_size, out_size, K
        self._proj = dense.Projection()
        # Adam state: W1's lives beside it (updated inside the W1 step kernel); b1 (, W2, b2) go
        # through gcg_adam_step_f32 with the same device step size
        self.optimizer = LasagneAdam(self.params[1:], lr=0.002, beta1=0.9, beta2=0.999,
                                     epsilon=1e-8)
        self.m1 = torch.zeros_like(self.W1)
        self.v1 = torch.zeros_like(self.W1)

    # -- what DropoutMLP adds: here, nothing -----------------------------------------------
    def _construct_dropout(self, layer: str) -> None:
        pass

    def _segments(self, perm: torch.Tensor, nnz_sel: int):
        """(segments, values) of a run of batches: the values stand in for X.data in the
        forward (None: X's own)."""
        return BatchSegments(self.Xd, perm, self.batch_size, nnz_sel), None

    def _hidden_train(self, h: torch.Tensor, b: int) -> torch.Tensor:
        """The hidden output of batch b of the epoch as the output layer is trained on it."""
        return h

    def _hidden_backward(self, g: torch.Tensor, gate):
        """(g, db1) from the gradient of _hidden_train's output (gate None: no hidden
        rectify)."""
        return gs.epilogue_backward(g, gate, True)

    def _penalty_coefs(self):
        """(l1, l2) of W1 and of W2: 0.5 shares of the layer's regul_coef (mlp.py:216-224);
        without a hidden layer the one weight is the output layer's."""
        c_out, c_hid = self.regul_coefs
        c1 = c_hid if self.add_hidden else c_out
        return (c1 * 0.5, c1 * 0.5), (c_out * 0.5, c_out * 0.5)

    def _penalty(self) -> torch.Tensor:
        p1, p2 = self._penalty_coefs()
        if self.add_hidden:  # output layer first, as the reference adds them
            return dense.l1l2_penalty([self.W2, self.W1], [p2, p1])
        return dense.l1l2_penalty([self.W1], [p1])

    def _first_layer(self, Xd: gs.DeviceCSR) -> torch.Tensor:
        """rectify(X.W1 + b1) (the hidden layer's deterministic output), or the logits
        X.W + b without a hidden layer -- sparse.spmm, as SparseInputDenseLayer runs it."""
        return gs.spmm(Xd, self.W1.detach(), bias=self.b1.detach(),
                       act="relu" if self.add_hidden else None)

    def _output_loss(self, h: torch.Tensor, y: torch.Tensor):
        """(mean CE, accuracy) of the output layer on the first layer's output."""
        if not self.add_hidden:
            return dense.softmax_xent(h, y)
        if self.out_size <= dense.FUSED_MAX_COLS:
            return self._proj.softmax_xent(h, self.W2, self.b2, y)
        return dense.softmax_xent(self._proj.matmul(h, self.W2, self.b2), y)

    @torch.no_grad()
    def _evaluate(self, Xd: gs.DeviceCSR, y: torch.Tensor):
        """f_val (mlp.py:247): deterministic loss with the penalty, and accuracy."""
        loss, acc = self._output_loss(self._first_layer(Xd), y)
        return loss + self._penalty(), acc

    @torch.no_grad()
    def _probabilities(self, Xd: gs.DeviceCSR) -> torch.Tensor:
        h = self._first_layer(Xd)
        if not self.add_hidden:
            return dense.softmax(h)
        if self.out_size <= dense.FUSED_MAX_COLS:
            return self._proj.probabilities(h, self.W2, self.b2)
        return dense.softmax(self._proj.matmul(h, self.W2, self.b2))

    # -- training -----------------------------------------------------------------------
    def _labels(self, Y, name: str) -> np.ndarray:
        Y = np.asarray(Y)
        if Y.ndim != 1 or not np.issubdtype(Y.dtype, np.integer):
            raise ValueError(f"{name} must be a 1-D integer label array")
        if Y.size and (int(Y.min()) < 0 or int(Y.max()) >= self.out_size):
            raise ValueError(f"{name} holds a label outside [0, {self.out_size}): out_size is "
                             "the number of distinct training labels (mlp.py:132)")
        return Y.astype(np.int32)

    @torch.no_grad()
    def _run_batches(self):
        """Device half of an epoch (the host half: MiniBatchTrainer._prepare_epoch, which
        gathers the epoch's labels): every batch's step, no host synchronisation. Returns the
        last batch's (train loss with the penalty, accuracy) as device scalars."""
        B, K, dev = self.batch_size, self.width, self.device
        X, opt = self.Xd, self.optimizer
        (l1, l2), pen2 = self._penalty_coefs()
        act = "relu" if self.add_hidden else None
        loss = acc = None
        for first, stop, nnz_sel in self._runs:
            seg, vals = self._segments(self._perm[first * B:stop * B], nnz_sel)
            for b in range(first, stop):
                rows = self._perm[b * B:(b + 1) * B]
                y = self._epoch_data[b * B:(b + 1) * B]
                last = b == self._n_batches - 1
                gate = gs.empty_gate(B, K, dev) if self.add_hidden else None
                # the order was range-checked on the host (plan_epoch)
                h = gs.spmm_rows(X, self.W1, self.b1, rows, vals=vals, act=act, gate=gate)
                h = self._hidden_train(h, b)
                opt.zero_grad()
                h.requires_grad_(True)
                with torch.enable_grad():
                    ce, a = self._output_loss(h, y)
                    obj = ce
                    if self.add_hidden:  # W2's penalty gradient; W1's is in the step kernel
                        obj = ce + dense.l1l2_penalty([self.W2], [pen2])
                obj.backward()
                if last:  # the loss the reference reports: the last batch's, with the penalty
                    loss, acc = ce.detach() + self._penalty(), a
                g = h.grad if h.grad.stride(-1) == 1 else h.grad.contiguous()
                g, db1 = self._hidden_backward(g, gate)
                opt.prepare()
                if self._w1_update is not None:
                    self._w1_update(self, b, g, l1, l2)
                else:
                    w1_step(self.W1, self.m1, self.v1, g, seg, b - first, l1, l2, opt.a_t,
                            opt.beta1, opt.beta2, opt.eps)
                self.b1.grad = db1
                opt.apply()
        return loss, acc

    @torch.no_grad()
    def fit(self, X_train, Y_train, X_dev, Y_dev, epoch_orders=None):
        """mlp.py:125-289. epoch_orders (tests, measurement): one order of the training rows per
        epoch instead of the np.random.shuffle draws."""
        in_size = self._check_inputs(X_train, X_dev)
        self.out_size = output_size(Y_train)
        log.info("output size is %d", self.out_size)
        if not self.hidden_layer_size:
            self.hidden_layer_size = default_hidden_size(self.out_size, in_size)
        if self.add_hidden and self.hidden_layer_size < 1:
            raise ValueError("hidden_layer_size must be at least 1")
        y_train, y_dev = self._labels(Y_train, "Y_train"), self._labels(Y_dev, "Y_dev")
        if X_train.shape[0] != y_train.size or X_dev.shape[0] != y_dev.size:
            raise ValueError("X and Y must have the same number of rows")
        self._upload_inputs(X_train, X_dev)
        self._build(in_size, self.out_size)
        self._train_data = torch.from_numpy(y_train).to(self.device)
        y_dev_d = torch.from_numpy(y_dev).to(self.device)
        log.info("training (n_epochs, batch_size) = (%d, %d)", self.n_epochs, self.batch_size)
        self.history = []
        # mlp.py:272-285: a strictly higher dev accuracy keeps the parameters
        best, best_params = run_epochs(
            lambda n: self._train_epoch(None if epoch_orders is None else epoch_orders[n]),
            lambda: self._evaluate(self.Xdev, y_dev_d), self.params, self.history,
            self.n_epochs, higher_accuracy, self.early_stopping_max_down)
        self.best_val_loss = best[0]
        restore(self.params, best_params)
        l_val, acc_val = self._evaluate(self.Xdev, y_dev_d)
        self.best_dev_loss, self.best_dev_acc = float(l_val), float(acc_val)
        log.info("Best dev acc: %f", self.best_dev_acc)
        return self

    # -- reference API ------------------------------------------------------------------
    def predict_proba(self, X_test):
        return self._probabilities(self._input(X_test)).cpu().numpy()

    def predict(self, X_test):
        return self._probabilities(self._input(X_test)).argmax(dim=1).cpu().numpy()

    def accuracy(self, X_test, Y_test):
        Xd = self._input(X_test)
        y = torch.from_numpy(self._labels(Y_test, "Y_test")).to(self.device)
        if y.numel() != Xd.n_rows:
            raise ValueError("X and Y must have the same number of rows")
        _loss, acc = self._evaluate(Xd, y)
        return float(acc)

    def score(self, X_test, Y_test):
        return self.accuracy(X_test, Y_test)

    @torch.no_grad()
    def get_embedding(self, X, as_tensor: bool = False):
        """The hidden layer's deterministic output (mlp.py:201-202, 310-311): a NumPy array, or
        with as_tensor the float32 device tensor itself (what dialect.eval_embeddings takes)."""
        if not self.add_hidden:
            raise ValueError("get_embedding needs add_hidden=True (mlp.py:200-202)")
        emb = self._first_layer(self._input(X))
        return emb if as_tensor else emb.cpu().numpy()

    def get_params(self):
        return [p.detach().cpu().numpy() for p in self.params]


class DropoutMLP(MLP):
    """MLP(drop_out=True, drop_out_coefs=[drop_out_hid, drop_out_in]) of the reference
    (mlp.py:128, 164-183), as main.py trains its classifier (main.py:556-558) and its
    dialect-embedding model (main.py:425-427, 2048 hidden units).

    The input is dropped with p = drop_out_coefs[1] and Lasagne's rescale 1 / (1 - p). The
    hidden dropout layer of mlp.py:179 is dead in the reference: it is bound to self.l_hid1,
    while l_out is built on the local l_hid1, so nothing is dropped after the rectifier -- the
    default here. hidden_dropout=True is this package's addition: p = drop_out_coefs[0] on the
    rectified hidden output in training, what the line evidently meant and what MLPCONV does.
    A coefficient of 0 means no mask for that layer. add_hidden=False is refused (the reference
    fails there with a NameError on l_hid1, mlp.py:189-196).

    Draws, in Lasagne's construction order from numpy's global stream: the input dropout's
    seed, W1, the hidden dropout layer's seed (drawn whether or not hidden_dropout is on: the
    reference constructs that layer), W2. init_parameters skips the two Glorot draws only.

    Masks (dropout.DropoutStream; the step is the number of batches trained so far, across
    segmentation runs and epochs): the input's on stream 0, keyed by (row id in X_train,
    feature), applied where the epoch is segmented (BatchSegments); the hidden one on stream 1,
    keyed by (position in the batch, hidden unit). Evaluation, prediction and get_embedding are
    deterministic (mlp.py:201, 205) and inherited; the reported train loss and accuracy are the
    last batch's from the masked forward (mlp.py:203, 210, 270)."""

    # a row in two batches of a run would share one slot of the dropped values
    permutation_only = True

    def __init__(self, n_epochs=10, batch_size=1000, init_parameters=None, complete_prob=False,
                 add_hidden=True, regul_coefs=(5e-5, 5e-5), save_results=False,
                 hidden_layer_size=None, drop_out=True, drop_out_coefs=(0.5, 0.5),
                 early_stopping_max_down=100000, loss_name="log", nonlinearity="rectify",
                 device="cuda", hidden_dropout=False):
        if not drop_out:
            raise ValueError("DropoutMLP is the drop_out=True trainer; MLP trains without")
        if not add_hidden:
            raise ValueError("drop_out needs add_hidden=True (the reference fails without: "
                             "mlp.py:189-196)")
        super().__init__(n_epochs, batch_size, init_parameters, complete_prob, add_hidden,
                         regul_coefs, save_results, hidden_layer_size, False, drop_out_coefs,
                         early_stopping_max_down, loss_name, nonlinearity, device)
        if len(self.drop_out_coefs) != 2:
            raise ValueError("drop_out_coefs is [drop_out_hid, drop_out_in]")
        for p in self.drop_out_coefs:
            _drop.dropout_threshold(p)  # outside [0, 1): ValueError
        self.drop_out = True
        self.hidden_dropout = bool(hidden_dropout)

    def _construct_dropout(self, layer: str) -> None:
        p_hid, p_in = self.drop_out_coefs  # mlp.py:128
        if layer == "input":
            self.stream_in = _drop.DropoutStream(_drop.draw_seed(), 0, self.device)
            self._drop_in = _drop.make_spec(self.stream_in, p_in)
        else:
            self.stream_hid = _drop.DropoutStream(_drop.draw_seed(), 1, self.device)
            self._drop_hid = _drop.make_spec(self.stream_hid, p_hid) if self.hidden_dropout \
                else None

    def _segments(self, perm: torch.Tensor, nnz_sel: int):
        if self._drop_in is None:
            return super()._segments(perm, nnz_sel)
        seg = BatchSegments(self.Xd, perm, self.batch_size, nnz_sel, self._drop_in,
                            self._vals_drop)
        return seg, self._vals_drop

    def _hidden_train(self, h: torch.Tensor, b: int) -> torch.Tensor:
        if self._drop_hid is None:
            return h
        self.stream_hid.set_step(self._steps_before + b)  # a device fill: no synchronisation
        return _drop.dropout_dense(h, self._drop_hid, out=h)

    def _hidden_backward(self, g: torch.Tensor, gate):
        # the one-pass kernel at every width (epilogue_backward composes the unmasked rule in
        # torch beyond 1024 columns)
        if self._drop_hid is None:
            return gs.relu_backward(g, gate=gate)
        return _drop.dropout_relu_backward(g, self._drop_hid, gate=gate)

    def _run_batches(self):
        out = super()._run_batches()
        self._steps_before += self._n_batches
        return out

    def fit(self, X_train, Y_train, X_dev, Y_dev, epoch_orders=None):
        self._steps_before = 0  # batches trained before the current epoch: the masks' step
        self._vals_drop = None
        return super().fit(X_train, Y_train, X_dev, Y_dev, epoch_orders)

    def _build(self, in_size: int, out_size: int):
        super()._build(in_size, out_size)
        # X's values behind the mask, once per fit: every batch's rows are rewritten by its
        # segmentation call
        if self._drop_in is not None:
            self._vals_drop = torch.zeros_like(self.Xd.data)
