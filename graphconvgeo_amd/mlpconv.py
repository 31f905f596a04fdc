"""MLPCONV -- the reference's GCN trainer (mlpconv.py:121-352) with every product on the GPU.

Same constructor, `fit(X, train_indices, dev_indices, test_indices, Y, H)`,
`predict/predict_proba/accuracy(partition)` as the reference. One epoch is one full-batch
step over all N nodes (mlpconv.py:293-295):

  forward   Z1 = X.W1 (HIP SpMM)  h = rectify(H.Z1 + b1) (HIP SpMM, fused epilogue)
            order "reference": Z2 = h.W2 (fp32 GEMM), logits = (H.Z2 + b2)[train_indices]
              (HIP SpMM, fused rows), then the softmax-CE row kernel (loss, hits; gradient pass
              in backward)
            order "propagate_first": P = (H.h)[train_indices] (HIP SpMM), then ONE MFMA kernel
              for P.W2 + b2, softmax, CE, argmax hits and the logits gradient (csrc/dense_fused.hip)
  loss      mean categorical CE of softmax(logits) + L1/L2 shares on W (mlpconv.py:229-243)
  backward  Theano's rules through the HIP kernels (scatter-add, H.g, X^T.g)
  update    lasagne.updates.adam(lr=4e-3, 0.9, 0.999, 1e-8) (mlpconv.py:263), restated below
            (its epsilon sits outside the bias correction, unlike torch.optim.Adam)

Validation every 10 epochs on dev, best-params restore and early stopping as
mlpconv.py:296-318. The checkpoint is `torch.save` of the best parameters when
`model_file` is given (the reference pickles to ./data/..., mlpconv.py:310-313).
drop_out=True (mlpconv.py:155, 199-201, 210-211; main_mlpconv itself runs with drop_out=False,
tensormain.py:233): `drop_out_hid, drop_out_in = dropout_coefs`; SparseInputDropoutLayer on X,
then lasagne.layers.dropout on the hidden layer, both with counter-based Philox masks that no
kernel stores (graphconvgeo_amd.dropout): training steps draw a new mask per epoch, validation,
the final dev evaluation and predict* run deterministic.
"""
from __future__ import annotations

import logging
import math
from typing import Optional

import numpy as np
import torch

from . import dense
from . import sparse as gs
from .dropout import DropoutStream, SparseInputDropoutLayer, draw_seed
from .layers import GATHER_DTYPES, ConvolutionDenseLayer, SparseConvolutionDenseLayer
from .training import LasagneOptimizer, lower_loss, restore, run_epochs

log = logging.getLogger(__name__)


class LasagneAdam(LasagneOptimizer):
    """lasagne.updates.adam: t += 1; a_t = lr*sqrt(1-b2^t)/(1-b1^t);
    m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g^2; p -= a_t*m/(sqrt(v)+eps)."""

    entry, second, lr = "gcg_adam_step_f32", "v", 4e-3

    def step_size(self, t):
        return self.lr * math.sqrt(1 - self.beta2 ** t) / (1 - self.beta1 ** t)


def trainer_order(order: str, in_size: int, n_classes: int) -> str:
    """The trainer's layer-2 order for `order="auto"` (the default since round 6): propagate
    first -- (H . h)[targets] then P . W2 + b2 -- whenever the fused MFMA output layer takes the
    classes (C <= dense.FUSED_MAX_COLS) or the SpMM is narrower that way (C > K); else the
    reference association. Propagate-first runs the projection over the distinct targets only
    (38 % of the nodes at train = 60 % drawn with replacement) where the reference order runs it
    over every node, so it wins even where its SpMM is wider: measured (bench train_step,
    tools/bench_train.py; profiles/r06/) Twitter-US (C = 256 < K = 300) 9.43 vs 9.93 ms,
    Twitter-World (C = 930) 40.2 vs 50.7 ms."""
    if order != "auto":
        return order
    if n_classes <= dense.FUSED_MAX_COLS or n_classes > in_size:
        return "propagate_first"
    return "reference"


def check_trainer_args(dtype, complete_prob, loss_name, order) -> None:
    """The constructor arguments the full-batch trainers share (MLPCONV and the row-partitioned
    dist_train.RowPartitionedMLPCONV)."""
    if dtype != "float32":
        raise ValueError("the GPU path computes in float32 (mlpconv.py dtype='float32')")
    if complete_prob:
        raise NotImplementedError("complete_prob (soft labels) is not on the graded path")
    if loss_name != "log":
        raise ValueError("only the 'log' (categorical cross-entropy) loss exists in the reference")
    if order not in ("reference", "propagate_first", "auto"):
        raise ValueError("order must be 'reference', 'propagate_first' or 'auto'")


def check_labels(Y) -> np.ndarray:
    """fit's Y as a 1-D array of class ids >= 0."""
    Y = np.asarray(Y)
    if Y.ndim != 1 or not np.issubdtype(Y.dtype, np.integer):
        raise ValueError("Y must be a 1-D integer label array (complete_prob is out of scope)")
    if Y.size and int(Y.min()) < 0:
        raise ValueError("labels must be >= 0 (class ids, data.py:399-432)")
    return Y


def fit_loop(train_step, evaluate, params, history, n_epochs, report_k_epoch,
             early_stopping_max_down):
    """The reference's epoch loop (mlpconv.py:290-318) for both full-batch trainers, so that
    every rank of the partitioned one takes the decisions the single-GPU one takes: training's
    run_epochs with the strictly-lower-dev-loss rule. train_step() -> (loss, acc) runs one epoch
    and is read back at once; evaluate() -> (loss, acc) is the dev set's, called every
    report_k_epoch epochs. At the end the best snapshot (if any) is copied back into `params`
    and the dev set is evaluated once more (mlpconv.py:316-318): that (loss, acc) is returned."""
    _best, best_params = run_epochs(lambda n: [float(x) for x in train_step()], evaluate, params,
                                    history, n_epochs, lower_loss, early_stopping_max_down,
                                    validate_every=report_k_epoch)
    restore(params, best_params)
    l_val, a_val = evaluate()
    return float(l_val), float(a_val)


class MLPCONV:
    def __init__(self, n_epochs=10, batch_size=1000, init_parameters=None, complete_prob=False,
                 add_hidden=True, regul_coefs=(5e-5, 5e-5), save_results=False,
                 hidden_layer_size=None, drop_out=False, dropout_coefs=(0.5, 0.5),
                 early_stopping_max_down=100000, loss_name="log", nonlinearity="rectify",
                 dtype="float32", device="cuda", seed: Optional[int] = None, mode: str = "auto",
                 model_file: Optional[str] = None, report_k_epoch: int = 10,
                 order: str = "auto", use_graph: bool = False, gather_dtype: str = "float32"):
        check_trainer_args(dtype, complete_prob, loss_name, order)
        self.drop_out = bool(drop_out)
        if self.drop_out:
            drop_out_hid, drop_out_in = dropout_coefs  # mlpconv.py:155
            for p in (drop_out_hid, drop_out_in):
                if not 0.0 <= float(p) < 1.0:
                    raise ValueError("dropout_coefs must be in [0, 1)")
        self.n_epochs = n_epochs
        self.batch_size = batch_size  # unused by the reference's full-batch loop, kept for API
        self.init_parameters = init_parameters
        self.regul_coefs = list(regul_coefs)
        self.hidden_layer_size = hidden_layer_size
        self.dropout_coefs = list(dropout_coefs)
        self.early_stopping_max_down = early_stopping_max_down
        self.nonlinearity = "rectify"  # the reference forces rectify (mlpconv.py:149)
        self.dtype = dtype
        self.device = torch.device(device)
        self.seed = seed
        self.mode = mode
        self.model_file = model_file
        self.report_k_epoch = report_k_epoch
        # ConvolutionDenseLayer order: reference | propagate_first | auto (the default,
        # resolved by trainer_order). Neither order is bitwise to the reference's P (the
        # projection runs on MFMA in its own k order); both meet the same float64 bars
        # (tests/test_config3_gpu.py).
        self.order = order
        # "bfloat16": the four H-products of a step (two forward, two backward) gather a
        # bfloat16 copy of their dense operand (layers.GATHER_DTYPES); X . W1 and X^T . dZ1 stay
        # float32. Works with use_graph: the bfloat16 copies are temporaries of torch's
        # allocator like the step's other intermediates, so the capture owns them.
        if gather_dtype not in GATHER_DTYPES:
            raise ValueError(f"gather_dtype must be one of {GATHER_DTYPES}")
        self.gather_dtype = gather_dtype
        self.use_graph = use_graph  # replay each epoch's fwd+bwd+adam as one captured HIP graph
        # repeated targets (drawn with replacement) computed once, weighted by multiplicity
        self.distinct_targets = True
        self.history = []

    # -- model --------------------------------------------------------------------------
    def _build(self, in_size: int, out_size: int, H):
        # Lasagne GlorotUniform draws W1 then W2 from numpy's global stream (mlpconv.py:205-217;
        # main_mlpconv seeds it, tensormain.py:227); `seed` gives a private stream instead
        rng = None if self.seed is None else np.random.RandomState(self.seed)
        # any H (mlpconv.py:152 takes it as given): its symmetry is checked on the device at
        # the first backward (DeviceCSR.check_symmetric) -- a non-symmetric operator such as
        # the row-normalized D^-1 (A+I) of main.py:451-455 back-propagates through its built
        # transpose, as Theano's S.dot gradient H^T . gz does
        Hd = H if isinstance(H, gs.DeviceCSR) else gs.DeviceCSR.from_scipy(H, self.device)
        W1 = W2 = None
        if self.init_parameters is not None:
            W1, _b1, W2, _b2 = self.init_parameters
        # drop_out: the layers in the reference's construction order, each dropout layer drawing
        # its seed from the weights' stream as Lasagne's DropoutLayer.__init__ does (also when
        # init_parameters supplies the weights): input-dropout seed, W1, hidden-dropout seed, W2.
        # [recalled Lasagne 0.2, unpinned]. drop_out=False draws nothing extra.
        p_hid, p_in = self.dropout_coefs if self.drop_out else (0.0, 0.0)
        self.l_in_drop = None
        if self.drop_out:
            self.l_in_drop = SparseInputDropoutLayer(in_size, p=p_in, device=self.device, rng=rng,
                                                     stream_id=0)
        self.l_hid1 = SparseConvolutionDenseLayer(in_size, H=Hd, num_units=self.hidden_layer_size,
                                                  W=W1, nonlinearity="rectify", device=self.device,
                                                  mode=self.mode, rng=rng, dropout=p_hid,
                                                  gather_dtype=self.gather_dtype)
        if self.drop_out and self.l_hid1.dropout_stream is None:  # p_hid == 0: still drawn
            self.l_hid1.dropout_stream = DropoutStream(draw_seed(rng), 1, self.device)
        self.dropout_streams = [] if not self.drop_out else \
            [self.l_in_drop.stream, self.l_hid1.dropout_stream]
        self.l_out = ConvolutionDenseLayer(self.l_hid1, H=self.l_hid1.H, num_units=out_size,
                                           W=W2, nonlinearity=None, device=self.device,
                                           mode=self.mode, rng=rng,
                                           gather_dtype=self.gather_dtype,
                                           order=trainer_order(self.order,
                                                               self.hidden_layer_size, out_size))
        if self.init_parameters is not None:
            with torch.no_grad():
                self.l_hid1.b.copy_(torch.as_tensor(self.init_parameters[1]))
                self.l_out.b.copy_(torch.as_tensor(self.init_parameters[3]))
        self.params = [self.l_hid1.W, self.l_hid1.b, self.l_out.W, self.l_out.b]
        self._proj = dense.Projection()  # padded W2 copies for the fused MFMA output kernel

    def _fused_output(self) -> bool:
        return self.l_out.order == "propagate_first" and \
            self.l_out.num_units <= dense.FUSED_MAX_COLS

    def _hidden(self, deterministic: bool = True) -> torch.Tensor:
        """The hidden layer's output; with drop_out and not deterministic, behind this step's
        input and hidden masks."""
        if not self.drop_out:
            return self.l_hid1(self.Xd)
        X = self.Xd if deterministic else self.l_in_drop(self.Xd)
        return self.l_hid1(X, deterministic=deterministic)

    def _logits(self, rows: gs.RowSelection) -> torch.Tensor:
        h = self._hidden()
        return self.l_out(h, target_indices=rows)  # (H.(h.W2) + b2)[rows], pre-softmax

    def _probabilities(self, rows: gs.RowSelection) -> torch.Tensor:
        h = self._hidden()
        if self._fused_output():
            return self._proj.probabilities(self.l_out.propagate(h, rows), self.l_out.W,
                                            self.l_out.b)
        return dense.softmax(self.l_out(h, target_indices=rows))

    def _penalty(self) -> torch.Tensor:
        # l1 / l2 shares 0.5 of each layer's regul_coef, output layer first (mlpconv.py:235-243)
        c_out, c_hid = self.regul_coefs
        return dense.l1l2_penalty([self.l_out.W, self.l_hid1.W],
                                  [(c_out * 0.5, c_out * 0.5), (c_hid * 0.5, c_hid * 0.5)])

    def _loss_acc(self, rows: gs.RowSelection, y: torch.Tensor, penalty: bool = True,
                  deterministic: bool = True):
        """categorical_crossentropy(softmax(logits), y).mean() (+ penalty) and the argmax
        accuracy (mlpconv.py:227-253), through the HIP softmax-CE kernels. deterministic=False
        (the training step, mlpconv.py:223 vs 246): with this step's dropout masks."""
        h = self._hidden(deterministic)
        T, w = len(rows), None
        d = rows.distinct() if self.distinct_targets else None
        if d is not None:
            # targets drawn with replacement (tensormain.py:226): the output layer runs on the
            # distinct rows, each row's loss / hit / gradient weighted by its multiplicity
            rows, first, w = d
            y = y.index_select(0, first)
        if self._fused_output():
            P = self.l_out.propagate(h, rows)  # (H . h)[rows], K wide
            loss, acc = self._proj.softmax_xent(P, self.l_out.W, self.l_out.b, y, denom=T,
                                                row_weight=w)
        else:
            loss, acc = dense.softmax_xent(self.l_out(h, target_indices=rows), y, denom=T,
                                           row_weight=w)
        if penalty:
            loss = loss + self._penalty()
        return loss, acc

    # -- reference API ------------------------------------------------------------------
    def fit(self, X, train_indices, dev_indices, test_indices, Y, H):
        """mlpconv.py:152-318 (full-batch epochs, validation every report_k_epoch)."""
        Y = check_labels(Y)
        out_size = int(np.max(Y)) + 1
        in_size = X.shape[1]
        if self.hidden_layer_size is None:
            raise ValueError("hidden_layer_size is required")
        self.train_indices = np.asarray(train_indices, dtype=np.int32)
        self.dev_indices = np.asarray(dev_indices, dtype=np.int32)
        self.test_indices = np.asarray(test_indices, dtype=np.int32)
        self.Xd = X if isinstance(X, gs.DeviceCSR) else gs.DeviceCSR.from_scipy(X, self.device)
        self._build(in_size, out_size, H)
        self.rows = {k: gs.RowSelection(v, self.device) for k, v in
                     (("train", self.train_indices), ("dev", self.dev_indices),
                      ("test", self.test_indices))}
        y_train = torch.as_tensor(Y[self.train_indices].astype(np.int32), device=self.device)
        y_dev = torch.as_tensor(Y[self.dev_indices].astype(np.int32), device=self.device)
        opt = LasagneAdam(self.params, lr=4e-3, beta1=0.9, beta2=0.999, epsilon=1e-8)
        self.optimizer = opt
        train_step = self._make_train_step(opt, y_train)

        def evaluate():
            with torch.no_grad():
                return self._loss_acc(self.rows["dev"], y_dev)

        # the epochs, then the dev evaluation with the restored best parameters (mlpconv.py:316-318)
        self.best_dev_loss, self.best_dev_acc = fit_loop(
            train_step, evaluate, self.params, self.history, self.n_epochs, self.report_k_epoch,
            self.early_stopping_max_down)
        if self.model_file:
            # the reference always pickles the best params (mlpconv.py:310-313); here only on
            # request: model_file="reference" writes its path, anything else is a path
            path = self.model_file
            if path == "reference":
                path = (f"./data/Xshape1_{in_size}_hidden_{self.hidden_layer_size}_regul_"
                        f"{self.regul_coefs[0]}_drop_{self.dropout_coefs[0]}.pkl")
            log.info("storing best parameters in %s ...", path)
            torch.save([p.detach().cpu() for p in self.params], path)
            self.model_path = path
        log.info("Best dev acc: %f", self.best_dev_acc)
        return self

    def _make_train_step(self, opt: LasagneAdam, y_train: torch.Tensor):
        """One epoch (mlpconv.py:295): eager, or a captured HIP graph replayed per epoch.

        Capture: one eager warm-up step on a side stream builds every lazy resource (launch
        plans, CSR(X^T), index CSRs, BLAS handles) outside the capture, then parameters and
        Adam state are restored, so the graph path computes exactly the eager trajectory."""
        rows = self.rows["train"]

        streams = self.dropout_streams

        def eager():
            for s in streams:  # host half of the masks: this epoch's step value
                s.advance()
            opt.zero_grad()
            loss, acc = self._loss_acc(rows, y_train, deterministic=False)
            loss.backward()
            opt.step()
            return loss.detach(), acc

        if not self.use_graph or self.n_epochs == 0:
            return eager
        snap_p = [p.detach().clone() for p in self.params]
        snap_o = opt.state()
        snap_s = [s.step for s in streams]
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            eager()
        torch.cuda.current_stream(self.device).wait_stream(side)
        with torch.no_grad():
            for p, s in zip(self.params, snap_p):
                p.copy_(s)
        opt.load_state(snap_o)
        for s, step in zip(streams, snap_s):  # the warm-up's mask step is not a training step
            s.set_step(step)
        opt.zero_grad()
        graph = torch.cuda.CUDAGraph()
        opt.prepare()  # step 1's a_t, written before capture (and before every replay)
        opt.t -= 1
        with torch.cuda.graph(graph):
            loss, acc = self._loss_acc(rows, y_train, deterministic=False)
            loss.backward()
            opt.apply()
        static = (loss.detach(), acc)
        self._graph = graph

        def replay():
            opt.prepare()
            for s in streams:
                s.advance()
            graph.replay()
            # the replay's Adam update moved W2 in place without bumping its version counter:
            # eager calls (validation, predict) must re-copy the padded weight copies
            self._proj.invalidate()
            for p in self.params:
                proj = getattr(p, "_gcg_projection", None)
                if proj is not None:
                    proj.invalidate()
            return static

        return replay

    def _indices(self, partition):
        if partition not in self.rows:
            raise ValueError(f"unknown partition {partition!r}")
        return self.rows[partition]

    @torch.no_grad()
    def predict_proba(self, dataset_partition):
        return self._probabilities(self._indices(dataset_partition)).cpu().numpy()

    @torch.no_grad()
    def predict(self, dataset_partition):
        return self._probabilities(self._indices(dataset_partition)).argmax(dim=1).cpu().numpy()

    @torch.no_grad()
    def accuracy(self, dataset_partition, y_true):
        rows = self._indices(dataset_partition)
        y = torch.as_tensor(np.asarray(y_true).astype(np.int32), device=self.device)
        _loss, acc = self._loss_acc(rows, y)
        return float(acc)

    @torch.no_grad()
    def geo_eval(self, dataset_partition, locs, medians, earth_radius_km=None,
                 threshold_km=161.0):
        """(mean km, median km, acc_at_161) of tensormain.geo_eval (tensormain.py:38-54) for the
        partition's predictions: the distance from each user's true location (`locs`, one
        [lat, lon] row per row of the partition) to the median of the predicted class. The
        predictions of predict() stay on the device (geo.geo_eval)."""
        from . import geo

        pred = self._probabilities(self._indices(dataset_partition)).argmax(dim=1)
        radius = geo.EARTH_RADIUS_KM if earth_radius_km is None else earth_radius_km
        return geo.geo_eval(pred, locs, medians, radius, threshold_km, device=self.device)

    def score(self, X, dataset_partition, y_true):
        """mlpconv.py:348-349 `score(X, dataset_partition, y_true)`. The reference forwards all
        three arguments to the two-argument accuracy() -- a TypeError there; this returns what
        it evidently intends: the accuracy on the partition (X is the model's own input, kept
        for the signature)."""
        return self.accuracy(dataset_partition, y_true)

    def get_params(self):
        return [p.detach().cpu().numpy() for p in self.params]
