"""What the trainers share around their steps, stated once (it imports none of them).

  LasagneOptimizer   lasagne.updates.adam / adamax on the GPU; a subclass names its fused C entry,
                     its step size and its second state list (mlpconv.LasagneAdam,
                     loc2lang.LasagneAdamax)
  run_epochs         the epoch loop of every fit (train, validate, compare, snapshot, count,
                     stop) with its three improvement rules; restore copies the snapshot back
  MiniBatchTrainer   the host half of a mini-batch epoch and the sparse inputs of fit and
                     predict (mlp.MLP, the two mdn trainers, loc2lang.NNModel_loc2lang)
"""
from __future__ import annotations

import logging
import math

import numpy as np
import scipy.sparse as sps
import torch
from torch.autograd.graph import increment_version

from . import sparse as gs
from ._native import call
from .layers import _as_tensor, _upload_cached
from .sparse import _ptr, _stream_handle

log = logging.getLogger(__name__)


# -- the optimisers --------------------------------------------------------------------------
class LasagneOptimizer:
    """A lasagne.updates rule with two state tensors per parameter (m and a second one) and a
    bias-corrected step size a_t: t += 1, a_t = step_size(t) on the host, then one fused launch
    per parameter. A subclass gives `entry` (the C entry: n, p, g, m, second, a_t, beta1, beta2,
    eps, stream), `second` (the second state list's name, also its key in state()), `lr` (its
    default learning rate) and step_size(t)."""

    def __init__(self, params, lr=None, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.params = list(params)
        self.lr = type(self).lr if lr is None else lr
        self.beta1, self.beta2, self.eps = beta1, beta2, epsilon
        self.t = 0
        self.m = [torch.zeros_like(p) for p in self.params]
        setattr(self, self.second, [torch.zeros_like(p) for p in self.params])
        # a_t lives on the device so a captured HIP graph reads the current step's value
        self.a_t = torch.zeros((), dtype=torch.float32, device=self.params[0].device)

    def prepare(self):
        """Host half of a step: t += 1 and the bias-corrected step size (Python double,
        rounded once to float32 exactly as an eager `a_t * m` would round it)."""
        self.t += 1
        self.a_t.fill_(self.step_size(self.t))

    @torch.no_grad()
    def apply(self, first: int = 0):
        """Device half of a step (capturable): one fused HIP launch per parameter instead of
        ~8 elementwise torch kernels. first: the parameters before it are left to the caller (a
        sparse-input weight updated, with its two states, inside its one-pass step)."""
        for p, m, s in list(zip(self.params, self.m, getattr(self, self.second)))[first:]:
            g = p.grad.contiguous()
            if not p.is_contiguous():
                raise ValueError(f"{type(self).__name__} needs contiguous parameters")
            with torch.cuda.device(p.device):
                call(self.entry, p.numel(), _ptr(p), _ptr(g), _ptr(m), _ptr(s), _ptr(self.a_t),
                     self.beta1, self.beta2, self.eps, _stream_handle(p.device))
            # an in-place write through a raw pointer: bump the version counters as a torch
            # in-place op would, so the padded weight copies (dense._WeightCache) follow
            increment_version(p)
            increment_version(m)
            increment_version(s)

    def step(self):
        self.prepare()
        self.apply()

    def state(self):
        return {"t": self.t, "m": [x.clone() for x in self.m],
                self.second: [x.clone() for x in getattr(self, self.second)]}

    @torch.no_grad()
    def load_state(self, st):
        self.t = st["t"]
        for dst, src in zip(self.m + getattr(self, self.second), st["m"] + st[self.second]):
            dst.copy_(src)

    def zero_grad(self):
        for p in self.params:
            p.grad = None


# -- the epoch loop --------------------------------------------------------------------------
# An improvement rule compares an epoch's dev figures with those of the last snapshot, both
# (loss,) or (loss, accuracy) as floats; before the first snapshot the best is (inf, 0.0).
def lower_loss(val, best) -> bool:
    """mlpconv.py:299, lang2loc.py:440: a strictly lower dev loss."""
    return val[0] < best[0]


def higher_accuracy(val, best) -> bool:
    """mlp.py:272: a strictly higher dev accuracy (never met while the accuracy stays 0)."""
    return val[1] > best[1]


def lower_loss_by_margin(val, best) -> bool:
    """loc2lang.py:260: a lower dev loss, by more than 1e-4 of the new loss."""
    return val[0] < best[0] and (best[0] - val[0]) > (0.0001 * val[0])


def run_epochs(train_epoch, evaluate, params, history, n_epochs, improved,
               early_stopping_max_down, validate_every=1, abort=None, after_epoch=None):
    """The reference's epoch loop, the one every fit runs. train_epoch(n) and evaluate() return
    (loss,) or (loss, accuracy); they are read back -- the training figures first -- after the
    validation is launched (figures that are floats already cost nothing). An epoch that is no
    multiple of validate_every only records its training figures. abort(dev loss) true ends the
    loop before the epoch's record is written: None is returned and nothing is restored.
    Otherwise after_epoch(n) runs, one record per epoch is appended to `history` (accuracy keys
    only where there is an accuracy), improved(val, best) true snapshots `params`, anything else
    counts one down, and more than early_stopping_max_down downs stop the loop. Returns
    (best, best_params): the dev figures at the last snapshot and the snapshot,
    ((inf, 0.0), None) when there was none."""
    best, best_params, n_down = (math.inf, 0.0), None, 0
    for n in range(n_epochs):
        train = train_epoch(n)
        validate = n % validate_every == 0
        val = evaluate() if validate else ()
        train, val = [float(x) for x in train], tuple(float(x) for x in val)
        if validate and abort is not None and abort(val[0]):
            return None
        if after_epoch is not None:
            after_epoch(n)
        history.append({"epoch": n, **dict(zip(("train_loss", "train_acc"), train)),
                        **dict(zip(("val_loss", "val_acc"), val))})
        if not validate:
            continue
        if improved(val, best):
            best, n_down = val, 0
            best_params = [p.detach().clone() for p in params]
        else:
            n_down += 1
        log.info("epoch %d, train %s, dev %s, best dev %s, num_down %d", n, train, val, best,
                 n_down)
        if n_down > early_stopping_max_down:
            log.info("validation results went down. early stopping ...")
            break
    return best, best_params


@torch.no_grad()
def restore(params, best_params) -> None:
    """The best snapshot back into `params`; None (no epoch improved): the last ones stay."""
    if best_params is not None:
        for p, b in zip(params, best_params):
            p.copy_(b)


# -- the host half of a mini-batch epoch -----------------------------------------------------
def n_batches(n: int, batchsize: int) -> int:
    if batchsize <= 0:
        raise ValueError("batch_size must be positive")
    if n < batchsize:
        raise ValueError(f"{n} training rows are fewer than one batch of {batchsize}")
    return (n - batchsize) // batchsize + 1


class MiniBatchTrainer:
    """What the mini-batch trainers share. A trainer has `device`, `batch_size` and, before its
    first epoch, `_n_train` (the training rows) and `_train_data` (a device tensor with one row
    per training row: the labels or targets, loc2lang's coordinates). The sparse-input trainers
    also have `_inputs = {}` (predict's upload cache) and, once built, `in_size`."""

    # an epoch's order must be a true permutation; False (MLP): any in-range order of the right
    # length, checked by mlp.plan_epoch
    permutation_only = True

    def _param(self, x, shape):
        return torch.nn.Parameter(_as_tensor(x, shape, self.device), requires_grad=False)

    def _input(self, X) -> gs.DeviceCSR:
        if isinstance(X, gs.DeviceCSR):
            Xd = X
        elif sps.issparse(X):
            Xd = _upload_cached(self._inputs, X.tocsr() if X.format != "csr" else X, self.device)
        else:
            raise ValueError("Input for this layer must be sparse")
        if hasattr(self, "in_size") and Xd.n_cols != self.in_size:
            raise ValueError(f"X has {Xd.n_cols} columns, the model {self.in_size}")
        return Xd

    def _check_inputs(self, X_train, X_dev) -> int:
        """fit's two inputs are sparse, of one width (returned) and hold at least one batch:
        host checks, before anything is uploaded."""
        for X in (X_train, X_dev):
            if not (isinstance(X, gs.DeviceCSR) or sps.issparse(X)):
                raise ValueError("Input for this layer must be sparse")
        if X_dev.shape[1] != X_train.shape[1]:
            raise ValueError("X_train and X_dev differ in width")
        n_batches(X_train.shape[0], self.batch_size)  # n < B raises
        return X_train.shape[1]

    def _upload_inputs(self, X_train, X_dev) -> None:
        """fit's two sparse inputs on the device as Xd and Xdev, with the host's copy of
        X_train's indptr, from which every segmentation call is sized (copied once)."""
        self.Xd = X_train if isinstance(X_train, gs.DeviceCSR) else \
            gs.DeviceCSR.from_scipy(X_train, self.device)
        self.Xdev = X_dev if isinstance(X_dev, gs.DeviceCSR) else \
            gs.DeviceCSR.from_scipy(X_dev, self.device)
        self._indptr_host = (np.asarray(X_train.indptr) if sps.issparse(X_train) and
                             X_train.format == "csr" else self.Xd.indptr.cpu().numpy()
                             ).astype(np.int64)
        self._n_train = self.Xd.n_rows

    def _plan_epoch(self, order: np.ndarray) -> np.ndarray:
        """The order cut to whole batches, the tail dropped. The sparse-input trainers plan
        their segmentation runs here too (mlp.plan_segmented_epoch)."""
        return order[:n_batches(self._n_train, self.batch_size) * self.batch_size]

    def _prepare_epoch(self, order) -> None:
        """Host half of an epoch: the order checked, cut into whole batches and uploaded
        (`_perm`, int32); the rows of `_train_data` it names gathered once (`_epoch_data`)."""
        n = self._n_train
        order = np.asarray(order)
        if self.permutation_only and (order.ndim != 1 or order.size != n or
                                      not np.array_equal(np.sort(order), np.arange(n))):
            # (with input dropout a row in two batches would share one slot of dropped values)
            raise ValueError(f"an epoch's order must be a permutation of the {n} training rows")
        perm = self._plan_epoch(order)
        self._n_batches = perm.size // self.batch_size
        self._perm = torch.from_numpy(perm.astype(np.int32)).to(self.device)
        self._epoch_data = self._train_data.index_select(0, self._perm.to(torch.int64))

    def _train_epoch(self, order=None):
        if order is None:  # mlp.py:84-85, lang2loc.py:398-400, loc2lang.py:219-221: one draw
            order = np.arange(self._n_train)  # per epoch from numpy's global stream
            np.random.shuffle(order)
        self._prepare_epoch(order)
        return self._run_batches()
