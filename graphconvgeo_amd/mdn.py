"""The mixture-density location head -- the reference's lang2loc.py (text to lat/lon).

A sparse bag-of-words goes through a tanh hidden layer to 6 * ncomp outputs, read as a mixture
of ncomp bivariate Gaussians over (lat, lon) (lang2loc.py:143-160) and trained by negative
log-likelihood (lang2loc.py:166-196); a prediction is the component mean where the mixture
density is highest (lang2loc.py:198-244).

  unpack_params     (mus, sigmas, corxy, pis) of a raw output      gcg_mdn_unpack_f32
  mdn_nll           the mean NLL, differentiable in the output     gcg_mdn_nll_f32 (forward and
                                                                   gradient in one launch)
  mdn_predict       the "mixture" / "pi" rule -> (n, 2) lat/lon    gcg_mdn_predict_f32
  geo_eval_latlon   lang2loc.geo_latlon_eval (mean / median km, Acc@161) on geo.geo_eval
  NNModel_lang2loc  the reference's class: constructor arguments, fit, predict

The layout of a raw output row is the reference's output.reshape(-1, 6, ncomp): six planes of
ncomp columns (means lat, lon; sigmas lat, lon; correlation; mixture logits). The transforms
and the stable forms they are evaluated in are stated in include/gcg_spmm.h.

The shared-component model -- the reference's lang2loc_mdnshared.py: one set of ncomp Gaussians
for the whole model (trainable mus [C, 2], raw sigmas [C, 2], raw corxy [C]); the network gives
only the mixture logits [B, C].

  shared_nll        the mean NLL, differentiable in the logits     gcg_mdn_shared_nll_f32 (loss,
                    and the three parameter tensors                both gradients, one call)
  shared_density    Dt [C, C]: component j's density at mean i     gcg_mdn_shared_density_f32
  shared_predict    "mixture" (pis . Dt) / "pi" -> (n, 2) lat/lon  gcg_mdn_shared_predict_f32
  shared_params     f_predict's (mus, sigmas, corxy, pis)
  cluster_params    get_cluster_centers after the clustering: per-cluster mean, std, correlation
  NNModel_lang2locshared   the reference's class
"""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np
import torch

from . import dense, geo
from . import sparse as gs
from ._native import call, device_scalar, workspace, workspace_bytes
from .dropout import DropoutStream, draw_seed, make_spec
from .layers import _as_tensor, _glorot_uniform
from .mlp import BatchSegments, plan_segmented_epoch, w1_step
from .mlpconv import LasagneAdam
from .sparse import _ld, _ptr, _stream_handle
from .training import MiniBatchTrainer, lower_loss, n_batches, restore, run_epochs

log = logging.getLogger(__name__)

MAX_COMPONENTS = 1024
METHODS = {"mixture": 0, "pi": 1}


def _check_output(O: torch.Tensor, n_comp: int) -> torch.Tensor:
    n_comp = int(n_comp)
    if not 1 <= n_comp <= MAX_COMPONENTS:
        raise ValueError(f"n_comp must be in [1, {MAX_COMPONENTS}], got {n_comp}")
    gs._require_cuda(O, "O")
    if O.dtype != torch.float32 or O.dim() != 2 or O.shape[1] != 6 * n_comp:
        raise ValueError(f"O must be a float32 [B, {6 * n_comp}] tensor (6 planes of n_comp)")
    return O if O.stride(1) == 1 else O.contiguous()


def unpack_params(O: torch.Tensor, n_comp: int):
    """lang2loc.unpack_params: (mus [B, 2, C], sigmas [B, 2, C], corxy [B, C], pis [B, C]) of a
    raw output O [B, 6 C], float32 device tensors."""
    O = _check_output(O, n_comp)
    B, C, dev = O.shape[0], int(n_comp), O.device
    mus = torch.empty((B, 2, C), dtype=torch.float32, device=dev)
    sigmas = torch.empty((B, 2, C), dtype=torch.float32, device=dev)
    corxy = torch.empty((B, C), dtype=torch.float32, device=dev)
    pis = torch.empty((B, C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("gcg_mdn_unpack_f32", B, C, _ptr(O), _ld(O), _ptr(mus), _ptr(sigmas), _ptr(corxy),
             _ptr(pis), _stream_handle(dev))
    return mus, sigmas, corxy, pis


def _targets(Y: torch.Tensor, B: int, dev) -> torch.Tensor:
    gs._require_cuda(Y, "Y")
    if Y.dtype != torch.float32 or Y.shape != (B, 2) or Y.device != dev:
        raise ValueError(f"Y must be a float32 [{B}, 2] tensor (lat, lon) on O's device")
    return Y.contiguous()


def nll_forward_backward(O: torch.Tensor, Y: torch.Tensor, want_grad: bool = True,
                         scale: Optional[torch.Tensor] = None, want_rows: bool = False):
    """(loss, dO, loss_rows) from one gcg_mdn_nll_f32 call: the mean NLL (device scalar), the
    gradient of scale * loss with respect to O (None unless want_grad; scale: a device scalar,
    default 1) and the per-row losses (None unless want_rows)."""
    if O.dim() != 2 or O.shape[1] % 6 or O.shape[0] == 0:
        raise ValueError("O must be [B, 6 * n_comp] with B >= 1")
    C = O.shape[1] // 6
    O = _check_output(O, C)
    B, dev = O.shape[0], O.device
    Y = _targets(Y, B, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    rows = torch.empty(B, dtype=torch.float32, device=dev)  # also the home of the mean's input
    dO = gs.empty_dense(B, 6 * C, dev) if want_grad else None
    scale = device_scalar(scale)
    with torch.cuda.device(dev):
        call("gcg_mdn_nll_f32", B, C, _ptr(O), _ld(O), _ptr(Y), _ptr(scale), _ptr(dO),
             _ld(dO) if dO is not None else 0, _ptr(rows), _ptr(loss), None, 0,
             _stream_handle(dev))
    return loss, dO, (rows if want_rows else None)


class _MdnNll(torch.autograd.Function):
    """The forward launch already writes the gradient of the mean (upstream 1); backward scales
    it by the upstream gradient."""

    @staticmethod
    def forward(ctx, O, Y):
        loss, dO, _ = nll_forward_backward(O, Y, want_grad=ctx.needs_input_grad[0])
        ctx.dO = dO
        return loss

    @staticmethod
    def backward(ctx, g):
        return ctx.dO * g, None


def mdn_nll(O: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
    """lang2loc.nll_loss on a raw output O [B, 6 C] and targets Y [B, 2] (lat, lon): the mean
    over the rows of -logsumexp_c(log pi_c + log N(y; mu_c, sigma_c, rho_c)), differentiable
    in O. Device scalar."""
    return _MdnNll.apply(O, Y)


def mdn_predict(O: torch.Tensor, n_comp: int, method: str = "mixture", return_index: bool = False):
    """lang2loc.pred: per row the component mean that maximises the mixture density
    ("mixture") or belongs to the largest pi ("pi"). Returns latlon [B, 2] float32 (device), and
    the chosen component [B] int32 with return_index."""
    if method not in METHODS:
        raise ValueError(f"prediction method must be one of {sorted(METHODS)}")
    O = _check_output(O, n_comp)
    B, dev = O.shape[0], O.device
    latlon = torch.empty((B, 2), dtype=torch.float32, device=dev)
    idx = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("gcg_mdn_predict_f32", B, int(n_comp), _ptr(O), _ld(O), METHODS[method], _ptr(idx),
             _ptr(latlon), _stream_handle(dev))
    return (latlon, idx) if return_index else latlon


# -- the shared-component model (lang2loc_mdnshared.py) ----------------------------------------
def _check_shared(L: torch.Tensor, mus, sigmas_raw, corxy_raw):
    """The logits [B, C] and the three parameter tensors, float32 on one device, contiguous."""
    gs._require_cuda(L, "L")
    if L.dtype != torch.float32 or L.dim() != 2:
        raise ValueError("L must be a float32 [B, n_comp] tensor (the mixture logits)")
    C = L.shape[1]
    if not 1 <= C <= MAX_COMPONENTS:
        raise ValueError(f"n_comp must be in [1, {MAX_COMPONENTS}], got {C}")
    mus, sigmas_raw, corxy_raw = _check_components(mus, sigmas_raw, corxy_raw, C, L.device)
    return (L if L.stride(1) == 1 else L.contiguous()), mus, sigmas_raw, corxy_raw


def _check_components(mus, sigmas_raw, corxy_raw, C: Optional[int] = None, dev=None):
    gs._require_cuda(mus, "mus")
    C = mus.shape[0] if C is None else C
    dev = mus.device if dev is None else dev
    if not 1 <= C <= MAX_COMPONENTS:
        raise ValueError(f"n_comp must be in [1, {MAX_COMPONENTS}], got {C}")
    for t, shape, name in ((mus, (C, 2), "mus"), (sigmas_raw, (C, 2), "sigmas_raw"),
                           (corxy_raw, (C,), "corxy_raw")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or \
                tuple(t.shape) != shape or t.device != dev:
            raise ValueError(f"{name} must be a float32 {list(shape)} tensor on {dev}")
    return mus.contiguous(), sigmas_raw.contiguous(), corxy_raw.contiguous()


def shared_nll_workspace_bytes(B: int, C: int) -> int:
    return workspace_bytes("gcg_mdn_shared_nll_f32_workspace_bytes", B, C)


def shared_nll_forward_backward(L: torch.Tensor, Y: torch.Tensor, mus: torch.Tensor,
                                sigmas_raw: torch.Tensor, corxy_raw: torch.Tensor,
                                want_grad: bool = True, scale: Optional[torch.Tensor] = None,
                                want_rows: bool = False):
    """(loss, dL, dparams, loss_rows) from one gcg_mdn_shared_nll_f32 call: the mean NLL (device
    scalar), the gradients of scale * loss with respect to the logits [B, C] and to the
    component parameters ([5, C]: d mus lat, d mus lon, d sigmas_raw lat, d sigmas_raw lon,
    d corxy_raw) -- both None unless want_grad; scale: a device scalar, default 1 -- and the
    per-row losses (None unless want_rows)."""
    L, mus, sigmas_raw, corxy_raw = _check_shared(L, mus, sigmas_raw, corxy_raw)
    B, C, dev = L.shape[0], L.shape[1], L.device
    if B == 0:
        raise ValueError("L must have at least one row")
    Y = _targets(Y, B, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    rows = torch.empty(B, dtype=torch.float32, device=dev)
    dL = gs.empty_dense(B, C, dev) if want_grad else None
    dparams = torch.empty((5, C), dtype=torch.float32, device=dev) if want_grad else None
    ws, nbytes = workspace("gcg_mdn_shared_nll_f32_workspace_bytes", dev, B, C)
    scale = device_scalar(scale)
    with torch.cuda.device(dev):
        call("gcg_mdn_shared_nll_f32", B, C, _ptr(L), _ld(L), _ptr(Y), _ptr(mus),
             _ptr(sigmas_raw), _ptr(corxy_raw), _ptr(scale), _ptr(dL),
             _ld(dL) if dL is not None else 0, _ptr(dparams), _ptr(rows), _ptr(loss), _ptr(ws),
             nbytes, _stream_handle(dev))
    return loss, dL, dparams, (rows if want_rows else None)


def split_dparams(dparams: torch.Tensor):
    """The [5, C] planes of gcg_mdn_shared_nll_f32 as the gradients of mus [C, 2],
    sigmas_raw [C, 2] and corxy_raw [C]."""
    return (dparams[0:2].t().contiguous(), dparams[2:4].t().contiguous(),
            dparams[4].contiguous())


class _SharedNll(torch.autograd.Function):
    """The forward launch writes the gradients of the mean (upstream 1) for the logits and the
    component parameters; backward scales them by the upstream gradient."""

    @staticmethod
    def forward(ctx, L, Y, mus, sigmas_raw, corxy_raw):
        want = any(ctx.needs_input_grad)
        loss, dL, dparams, _ = shared_nll_forward_backward(L, Y, mus, sigmas_raw, corxy_raw,
                                                           want_grad=want)
        ctx.grads = (dL, *split_dparams(dparams)) if want else None
        return loss

    @staticmethod
    def backward(ctx, g):
        dL, dmus, dsig, dcor = ctx.grads
        return dL * g, None, dmus * g, dsig * g, dcor * g


def shared_nll(L: torch.Tensor, Y: torch.Tensor, mus: torch.Tensor, sigmas_raw: torch.Tensor,
               corxy_raw: torch.Tensor) -> torch.Tensor:
    """lang2loc_mdnshared.nll_loss_sharedparams on the logits L [B, C], targets Y [B, 2] (lat,
    lon) and the shared components (mus [C, 2], raw sigmas [C, 2], raw corxy [C]): the mean over
    the rows of -logsumexp_c(log pi_rc + log N(y_r; mu_c, softplus(sigma_c), softsign(rho_c))),
    differentiable in L and the three parameter tensors. Device scalar."""
    return _SharedNll.apply(L, Y, mus, sigmas_raw, corxy_raw)


def shared_density(mus: torch.Tensor, sigmas_raw: torch.Tensor, corxy_raw: torch.Tensor
                   ) -> torch.Tensor:
    """Dt [C, C] float32: Dt[j, i] = the density of component j at the mean of component i --
    the table the "mixture" rule multiplies the pis with, once per parameter set."""
    mus, sigmas_raw, corxy_raw = _check_components(mus, sigmas_raw, corxy_raw)
    C, dev = mus.shape[0], mus.device
    Dt = torch.empty((C, C), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        call("gcg_mdn_shared_density_f32", C, _ptr(mus), _ptr(sigmas_raw), _ptr(corxy_raw),
             _ptr(Dt), _stream_handle(dev))
    return Dt


def shared_predict(L: torch.Tensor, mus: torch.Tensor, sigmas_raw: torch.Tensor,
                   corxy_raw: torch.Tensor, method: str = "mixture", return_index: bool = False,
                   density: Optional[torch.Tensor] = None):
    """lang2loc_mdnshared.pred_sharedparams: per row the component mean that maximises the
    mixture density pis . Dt ("mixture") or belongs to the largest pi ("pi"). density: a
    shared_density(...) of the same parameters, computed here when None. Returns latlon [B, 2]
    float32 (device), and the chosen component [B] int32 with return_index."""
    if method not in METHODS:
        raise ValueError(f"prediction method must be one of {sorted(METHODS)}")
    L, mus, sigmas_raw, corxy_raw = _check_shared(L, mus, sigmas_raw, corxy_raw)
    B, C, dev = L.shape[0], L.shape[1], L.device
    if method == "mixture":
        if density is None:
            density = shared_density(mus, sigmas_raw, corxy_raw)
        elif density.dtype != torch.float32 or tuple(density.shape) != (C, C) or \
                density.device != dev or not density.is_contiguous():
            raise ValueError(f"density must be a contiguous float32 [{C}, {C}] tensor on {dev}")
    else:
        density = None
    latlon = torch.empty((B, 2), dtype=torch.float32, device=dev)
    idx = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("gcg_mdn_shared_predict_f32", B, C, _ptr(L), _ld(L), _ptr(density), _ptr(mus),
             METHODS[method], _ptr(idx), _ptr(latlon), _stream_handle(dev))
    return (latlon, idx) if return_index else latlon


def shared_params(L: torch.Tensor, mus: torch.Tensor, sigmas_raw: torch.Tensor,
                  corxy_raw: torch.Tensor):
    """f_predict of lang2loc_mdnshared.py:514: (mus [C, 2], sigmas = softplus(raw) [C, 2],
    corxy = softsign(raw) [C], pis = softmax(L) [B, C]), float32 device tensors. The two
    C-sized transforms are torch ops; the softmax is the row kernel (dense.softmax)."""
    L, mus, sigmas_raw, corxy_raw = _check_shared(L, mus, sigmas_raw, corxy_raw)
    return (mus, torch.nn.functional.softplus(sigmas_raw),
            corxy_raw / (1 + corxy_raw.abs()), dense.softmax(L))


def cluster_params(latlon, labels, n_cluster: int, raw: bool = True):
    """The part of lang2loc_mdnshared.get_cluster_centers (:127-185) after the clustering:
    (mus [n, 2], sigmas [n, 2], corxys [n]) float32 NumPy arrays of the clusters 0 .. n - 1 of
    `labels` -- the mean, the standard deviations (np.cov, ddof = 1) and the correlation of each
    cluster's (lat, lon); 1, 1, 0 for a single member or where any of them is NaN (a cluster of
    identical points: 0 / 0). With raw, sigmas and corxys are passed through the inverse
    softplus s + log1p(-exp(-s)) and the inverse softsign c / (1 - |c|), so that the model's
    transforms recover them.

    Deviations: the labels come from the caller (geo.KDTreeClustering: deterministic, on the
    device) where the reference runs MiniBatchKMeans, so mus is the members' mean, not a k-means
    centre; the reference leaves the correlation undefined for a single member, here it is 0.
    No hot path: NumPy on the host. kmeans.get_cluster_centers is the reference's whole
    function, k-means and these statistics on the device."""
    latlon = np.asarray(latlon, dtype=np.float64)
    labels = np.asarray(labels)
    n = int(n_cluster)
    if latlon.ndim != 2 or latlon.shape[1] != 2 or labels.shape != (latlon.shape[0],):
        raise ValueError("latlon must be [n, 2] (lat, lon) with one label per row")
    mus = np.zeros((n, 2), np.float32)
    sigmas = np.zeros((n, 2), np.float32)
    corxys = np.zeros(n, np.float32)
    for i in range(n):
        samples = latlon[labels == i]
        if samples.shape[0] == 0:
            raise ValueError(f"cluster {i} has no member")
        mus[i] = samples.mean(axis=0)
        std = np.array([1.0, 1.0])
        cor = 0.0
        if samples.shape[0] > 1:
            cov = np.cov(samples, rowvar=False)
            with np.errstate(invalid="ignore", divide="ignore"):
                s = np.sqrt(np.array([cov[0, 0], cov[1, 1]]))
                c = cov[0, 1] / (s[0] * s[1])
            if not (np.isnan(s).any() or np.isnan(cov[0, 1]) or np.isnan(c)):
                std, cor = s, float(c)
        if raw:
            with np.errstate(divide="ignore"):
                sigmas[i] = std + np.log1p(-np.exp(-std))
                corxys[i] = cor / (1.0 - abs(cor))
        else:
            sigmas[i], corxys[i] = std, cor
    return mus, sigmas, corxys


def geo_eval_latlon(pred_latlon, locs, earth_radius_km: float = geo.EARTH_RADIUS_KM,
                    threshold_km: float = 161.0, device=None):
    """lang2loc.geo_latlon_eval (lang2loc.py:81-98): (mean km, median km, Acc@161) of the
    haversine distance from every true location to its predicted coordinate -- geo.geo_eval with
    the predictions as the "medians" and arange as the classes."""
    if device is None and isinstance(pred_latlon, torch.Tensor) and pred_latlon.is_cuda:
        device = pred_latlon.device
    classes = torch.arange(len(pred_latlon), dtype=torch.int64)
    return geo.geo_eval(classes, locs, pred_latlon, earth_radius_km, threshold_km, device=device)


class _MdnTrainer(MiniBatchTrainer):
    """What NNModel_lang2loc and NNModel_lang2locshared share: the constructor arguments of the
    reference, the hidden layer tanh(X.W1 + b1), the batch loop (one step per batch, W1 updated
    in one pass over the batch's segments), the dev loss over whole batches, and fit: the shared
    loop (training.run_epochs) with the strict-`<` rule, early stopping and restore. The sparse
    inputs and the host half of an epoch are training.MiniBatchTrainer's. A model states its
    head: _build (its parameters and optimiser), _head_backward (a batch's loss with the
    gradients of everything but W1 and b1), _loss (the deterministic loss of a raw output) and
    _penalty_coefs / _penalty."""

    n_init_parameters = 4
    init_names = "[W1, b1, W2, b2]"
    nan_stops = False  # lang2loc_mdnshared.py:627-629: a NaN dev loss ends fit with None
    _plan_epoch = plan_segmented_epoch

    def __init__(self, n_epochs=10, batch_size=1000, regul_coef=1e-6, input_size=None,
                 output_size=None, hid_size=100, drop_out=False, dropout_coef=0.5,
                 early_stopping_max_down=10, dtype="float32", autoencoder=100,
                 input_sparse=False, reload=False, ncomp=100, sqerror=False, dataset_name="",
                 init_parameters=None, device="cuda"):
        if sqerror:
            raise NotImplementedError("sqerror (the squared-error regressor) is not built")
        if reload:
            raise NotImplementedError("reload (a pickled model file) is not built")
        if dtype != "float32":
            raise ValueError("the GPU path computes in float32 (lang2loc.py dtype='float32')")
        if not 1 <= int(ncomp) <= MAX_COMPONENTS:
            raise ValueError(f"ncomp must be in [1, {MAX_COMPONENTS}]")
        if int(hid_size) < 1:
            raise ValueError("hid_size must be at least 1")
        if drop_out and not 0.0 <= float(dropout_coef) < 1.0:
            raise ValueError("dropout_coef must be in [0, 1)")
        self.n_epochs = n_epochs
        self.batch_size = int(batch_size)
        self.regul_coef = regul_coef
        self.hid_size = int(hid_size)
        self.drop_out = bool(drop_out)
        self.dropout_coef = float(dropout_coef)
        self.early_stopping_max_down = early_stopping_max_down
        self.dtype = dtype
        self.input_size = input_size
        self.output_size = output_size
        self.autoencoder = autoencoder
        self.sparse = input_sparse
        self.reload = False
        self.n_bigaus_comp = int(ncomp)
        self.sqerror = False
        self.dataset_name = dataset_name
        self.init_parameters = init_parameters
        self.device = torch.device(device)
        self.history = []
        self._inputs = {}

    # -- model --------------------------------------------------------------------------
    @property
    def _drops(self) -> bool:
        return self.drop_out and self.dropout_coef > 0  # lang2loc.py:280

    def _build_layers(self, in_size: int, n_out: int):
        """The dropout stream and the two layers, drawn in Lasagne's construction order: the
        dropout layer's seed, then W1, then W2 (GlorotUniform; zero biases). Returns the
        init_parameters past the two layers' four (the head's own)."""
        K, dev = self.hid_size, self.device
        init = self.init_parameters
        if init is not None and len(init) != self.n_init_parameters:
            raise ValueError(f"init_parameters must be {self.init_names}, as "
                             "lasagne.layers.get_all_param_values gives them")
        self._stream = DropoutStream(draw_seed(), 0, dev) if self._drops else None
        self._drop = make_spec(self._stream, self.dropout_coef) if self._drops else None
        self.W1 = self._param(_glorot_uniform(in_size, K) if init is None else init[0],
                              (in_size, K))
        self.b1 = self._param(np.zeros(K, np.float32) if init is None else init[1], (K,))
        self.W2 = self._param(_glorot_uniform(K, n_out) if init is None else init[2],
                              (K, n_out)).requires_grad_(True)
        self.b2 = self._param(np.zeros(n_out, np.float32) if init is None else init[3],
                              (n_out,)).requires_grad_(True)
        self.in_size = in_size
        self._proj = dense.Projection()
        return None if init is None else init[4:]

    def _make_optimizer(self):
        """Adam at lr 1e-3 on every parameter; W1's state lives beside it (updated inside the
        W1 step kernel)."""
        self.optimizer = LasagneAdam(self.params[1:], lr=1e-3, beta1=0.9, beta2=0.999,
                                     epsilon=1e-8)
        self.m1 = torch.zeros_like(self.W1)
        self.v1 = torch.zeros_like(self.W1)

    def _hidden(self, X: gs.DeviceCSR, vals: torch.Tensor, rows: Optional[torch.Tensor]
                ) -> torch.Tensor:
        """tanh(X[rows].W1 + b1) with X's values read from `vals`: the plan-less SpMM (no
        activation in its epilogue), then tanh in place. rows: int32 device row ids,
        range-checked by the caller; None: every row of X."""
        return gs.spmm_rows(X, self.W1, self.b1, rows, vals=vals).tanh_()

    @torch.no_grad()
    def _output(self, Xd: gs.DeviceCSR, n_rows: Optional[int] = None) -> torch.Tensor:
        """The deterministic raw output of the first n_rows rows (default: all)."""
        n = Xd.n_rows if n_rows is None else n_rows
        rows = None
        if n != Xd.n_rows:
            rows = torch.arange(n, dtype=torch.int32, device=self.device)
        h = self._hidden(Xd, Xd.data, rows)
        return self._proj.matmul(h, self.W2.detach(), self.b2.detach())

    @torch.no_grad()
    def _evaluate(self, Xd: gs.DeviceCSR, Y: torch.Tensor) -> torch.Tensor:
        """f_val over the unshuffled batches with the tail dropped (lang2loc.py:433-438): every
        batch has B rows, so the mean of the batch means is the mean over the first
        (n // B) * B rows -- one forward."""
        n = n_batches(Xd.n_rows, self.batch_size) * self.batch_size
        loss = self._loss(self._output(Xd, n), Y[:n])
        pen = self._penalty()
        return loss if pen is None else loss + pen

    # -- training -----------------------------------------------------------------------
    def _coords(self, Y, n: int, name: str) -> torch.Tensor:
        Y = np.asarray(Y)
        if Y.ndim != 2 or Y.shape != (n, 2):
            raise ValueError(f"{name} must have shape ({n}, 2) [lat, lon], got {Y.shape}")
        return torch.from_numpy(np.ascontiguousarray(Y, dtype=np.float32)).to(self.device)

    @torch.no_grad()
    def _run_batches(self) -> torch.Tensor:
        """Device half of an epoch (the host half: MiniBatchTrainer._prepare_epoch, which
        gathers the epoch's targets): every batch's step, no host synchronisation. Returns the
        mean of the batch losses (penalty included) as a device scalar."""
        B, dev = self.batch_size, self.device
        X, opt = self.Xd, self.optimizer
        l1, l2 = self._penalty_coefs()
        total = torch.zeros((), dtype=torch.float32, device=dev)
        for first, stop, nnz_sel in self._runs:
            seg = BatchSegments(X, self._perm[first * B:stop * B], B, nnz_sel, self._drop,
                                self._vals_drop)
            vals = X.data if self._drop is None else self._vals_drop
            for b in range(first, stop):
                rows = self._perm[b * B:(b + 1) * B]
                y = self._epoch_data[b * B:(b + 1) * B]
                h = self._hidden(X, vals, rows)
                opt.zero_grad()
                h.requires_grad_(True)
                nll = self._head_backward(h, y)
                pen = self._penalty()  # of the weights before their update, as f_train reports
                total += nll if pen is None else nll + pen
                hd = h.detach()
                g = torch.addcmul(h.grad, h.grad, hd * hd, value=-1.0)  # dh (1 - h^2)
                opt.prepare()
                w1_step(self.W1, self.m1, self.v1, g, seg, b - first, l1, l2, opt.a_t, opt.beta1,
                        opt.beta2, opt.eps)
                self.b1.grad = gs.colsum(g)
                opt.apply()
        return total / self._n_batches

    @torch.no_grad()
    def fit(self, X_train, Y_train, X_dev, Y_dev, *ignored, epoch_orders=None):
        """lang2loc.py:408-455. The reference's six further arguments (X_test, Y_test, U_train,
        U_dev, U_test, userLocation) are accepted and ignored, as fit ignores them there.
        epoch_orders (tests, measurement): one permutation of the training rows per epoch
        instead of the np.random.shuffle draws."""
        in_size = self._check_inputs(X_train, X_dev)
        if self.input_size is not None and int(self.input_size) != in_size:
            raise ValueError(f"X_train has {in_size} columns, input_size says {self.input_size}")
        if X_dev.shape[0] < self.batch_size:
            raise ValueError(f"{X_dev.shape[0]} dev rows are fewer than one batch of "
                             f"{self.batch_size}: the dev loss is a mean over whole batches")
        self._train_data = self._coords(Y_train, X_train.shape[0], "Y_train")
        y_dev = self._coords(Y_dev, X_dev.shape[0], "Y_dev")
        self._upload_inputs(X_train, X_dev)
        self._build(in_size)
        # X's values behind the mask: every batch's rows are rewritten by its segmentation call
        self._vals_drop = torch.zeros_like(self.Xd.data) if self._drop is not None else None
        log.info("training with %d n_epochs and %d batch_size", self.n_epochs, self.batch_size)
        self.history = []
        out = run_epochs(
            lambda n: (self._train_epoch(None if epoch_orders is None else epoch_orders[n]),),
            lambda: (self._evaluate(self.Xdev, y_dev),), self.params, self.history,
            self.n_epochs, lower_loss, self.early_stopping_max_down,
            abort=np.isnan if self.nan_stops else None)
        if out is None:
            self.nan = True
            return None
        best, best_params = out
        self.best_val_loss = best[0]
        restore(self.params, best_params)  # None: no epoch gave a finite improvement; keep the last
        return self

    def get_params(self):
        return [p.detach().cpu().numpy() for p in self.params]

    def set_params(self, params):
        """lang2loc.py:394-395 (on a fitted model)."""
        with torch.no_grad():
            for p, v in zip(self.params, params):
                p.copy_(_as_tensor(v, tuple(p.shape), self.device))
        self._proj.invalidate()


class NNModel_lang2loc(_MdnTrainer):
    """lang2loc.NNModel_lang2loc (lang2loc.py:100-463) with every product and the loss on the GPU.

    Network: tanh(X.W1 + b1) (SparseInputDenseLayer) then the linear h.W2 + b2 with 6 * ncomp
    units; GlorotUniform weights drawn W1 then W2 (the input dropout's seed first when dropout
    is on), zero biases. Loss: mdn_nll plus regul_coef * 0.5 * (sum|W1| + sum W1^2) when
    regul_coef is truthy -- only the hidden layer is penalised: lang2loc.py:315-318 assign the
    output layer's penalty and then overwrite it, and this follows what runs. Adam, lr 1e-3.

    One epoch (lang2loc.py:426-451): shuffled batches with the tail dropped
    (mlp.iterate_minibatch_indices); the reported train loss is the mean of the batch losses
    (each before its update), accumulated on the device; the dev loss is the mean over the
    unshuffled dev batches with the tail dropped, computed as one deterministic forward over the
    first (n_dev // B) * B dev rows. Strict `l_val < best` keeps the parameters, otherwise a
    counter runs and training stops when it exceeds early_stopping_max_down; the best parameters
    are restored. No host synchronisation between an epoch's first and last batch.

    Step: forward over the batch's rows (plan-less SpMM), tanh, the output GEMM, gcg_mdn_nll_f32
    (loss and gradient in one launch), the backward GEMMs, the tanh backward g * (1 - h^2) with
    its column sums, then one pass over W1 (mlp.w1_step) on the batch's segments.

    Deviations: drop_out=True (with dropout_coef > 0) masks X in training only -- the reference
    evaluates validation and prediction with its single training graph, dropout on
    (lang2loc.py:300, 328-329); here both are deterministic. predict covers every row (the
    reference's driver drops the tail batch, lang2loc.py:604-609). sqerror=True, a truthy
    reload and dense inputs are refused; autoencoder is accepted and unused, as there.
    """

    def _build(self, in_size: int):
        self._build_layers(in_size, 6 * self.n_bigaus_comp)
        self.params = [self.W1, self.b1, self.W2, self.b2]
        self._make_optimizer()

    def _penalty_coefs(self):
        """(l1, l2) of W1: 0.5 shares of regul_coef (lang2loc.py:310-318), 0 when falsy."""
        c = float(self.regul_coef) if self.regul_coef else 0.0
        return c * 0.5, c * 0.5

    def _penalty(self) -> Optional[torch.Tensor]:
        if not self.regul_coef:
            return None
        return dense.l1l2_penalty([self.W1], [self._penalty_coefs()])

    def _loss(self, O: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        return nll_forward_backward(O, Y, want_grad=False)[0]

    def _head_backward(self, h: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        with torch.enable_grad():
            O = self._proj.matmul(h, self.W2, self.b2)
        nll, dO, _ = nll_forward_backward(O.detach(), y)
        O.backward(dO)
        return nll

    # -- reference API ------------------------------------------------------------------
    def predict_params(self, X):
        """f_predict (lang2loc.py:329): mus [n, 2, C], sigmas [n, 2, C], corxy [n, C],
        pis [n, C] as NumPy arrays."""
        O = self._output(self._input(X))
        return tuple(t.cpu().numpy() for t in unpack_params(O, self.n_bigaus_comp))

    def predict(self, X, prediction_method: str = "mixture"):
        """lang2loc.py:460-463: the selected means, n x 2 (lat, lon), for every row of X."""
        O = self._output(self._input(X))
        return mdn_predict(O, self.n_bigaus_comp, prediction_method).cpu().numpy()


class NNModel_lang2locshared(_MdnTrainer):
    """lang2loc_mdnshared.NNModel_lang2locshared (lang2loc_mdnshared.py:201-688) with every
    product and the loss on the GPU.

    Network: tanh(X.W1 + b1) then h.W2 + b2 with ncomp units, the mixture logits
    (lasagne_layers.MDNSharedParams, its softmax folded into the loss). The layer also holds the
    one set of Gaussians every row shares: mus [C, 2] (used raw), sigmas [C, 2] (softplus of
    them) and corxy [C] (softsign). The parameter list has Lasagne's order
    [W1, b1, W2, b2, mus, sigmas, corxy] (get_params, set_params, init_parameters). Without
    init_parameters the draws follow Lasagne's construction order on numpy's global stream: the
    dropout seed (when dropout is on), W1 and W2 GlorotUniform, then -- each only when the
    constructor was not given it -- mus = randn(C, 2), sigmas = uniform(10, 20, (C, 2)),
    corxy = randn(C); cluster_params gives data-derived ones.

    Loss: shared_nll plus regul_coef * 0.5 * (sum|W| + sum W^2) over W1 and W2
    (lang2loc_mdnshared.py:495-506: unlike lang2loc, both layers count; biases and the Gaussian
    parameters are not regularizable). Adam, lr 1e-3, on all seven parameters. Epoch, dev loss,
    model selection, early stopping and restore as NNModel_lang2loc; a NaN dev loss sets
    self.nan and fit returns None (:627-629).

    Step: forward over the batch's rows, tanh, the output GEMM, gcg_mdn_shared_nll_f32 (loss,
    the logits' gradient and the 5 C parameter gradients in one call), the backward GEMMs with
    W2's penalty gradient, the tanh backward with its column sums, then one pass over W1.

    Deviations: those of NNModel_lang2loc (validation and prediction deterministic; predict
    covers every row and takes prediction_method; sqerror, reload and dense inputs refused).
    """

    n_init_parameters = 7
    init_names = "[W1, b1, W2, b2, mus, sigmas, corxy]"
    nan_stops = True

    def __init__(self, n_epochs=10, batch_size=1000, regul_coef=1e-6, input_size=None,
                 output_size=None, hid_size=100, drop_out=False, dropout_coef=0.5,
                 early_stopping_max_down=10, dtype="float32", autoencoder=100,
                 input_sparse=False, reload=False, ncomp=100, sqerror=False, mus=None,
                 sigmas=None, corxy=None, dataset_name="", init_parameters=None, device="cuda"):
        super().__init__(n_epochs=n_epochs, batch_size=batch_size, regul_coef=regul_coef,
                         input_size=input_size, output_size=output_size, hid_size=hid_size,
                         drop_out=drop_out, dropout_coef=dropout_coef,
                         early_stopping_max_down=early_stopping_max_down, dtype=dtype,
                         autoencoder=autoencoder, input_sparse=input_sparse, reload=reload,
                         ncomp=ncomp, sqerror=sqerror, dataset_name=dataset_name,
                         init_parameters=init_parameters, device=device)
        C = self.n_bigaus_comp
        for x, shape, name in ((mus, (C, 2), "mus"), (sigmas, (C, 2), "sigmas"),
                               (corxy, (C,), "corxy")):
            if x is not None and np.shape(x) != shape:
                raise ValueError(f"{name} must have shape {shape}, got {np.shape(x)}")
        self.mus_init, self.sigmas_init, self.corxy_init = mus, sigmas, corxy
        self.nan = False

    def _build(self, in_size: int):
        C = self.n_bigaus_comp
        rest = self._build_layers(in_size, C)
        if rest is None:  # MDNSharedParams' draws, after the DenseLayer's W (lasagne_layers.py:224-240)
            given = (self.mus_init, self.sigmas_init, self.corxy_init)
            rest = [given[0] if given[0] is not None else
                    np.random.randn(C, 2).astype(np.float32)]
            rest.append(given[1] if given[1] is not None else
                        np.random.uniform(low=10, high=20, size=(C, 2)).astype(np.float32))
            rest.append(given[2] if given[2] is not None else
                        np.random.randn(C).astype(np.float32))
        self.mus = self._param(rest[0], (C, 2))
        self.sigmas = self._param(rest[1], (C, 2))
        self.corxy = self._param(rest[2], (C,))
        self.params = [self.W1, self.b1, self.W2, self.b2, self.mus, self.sigmas, self.corxy]
        self._make_optimizer()

    def _penalty_coefs(self):
        """(l1, l2) of W1 and of W2: 0.5 shares of regul_coef (:496-503), 0 when falsy."""
        c = float(self.regul_coef) if self.regul_coef else 0.0
        return c * 0.5, c * 0.5

    def _penalty(self) -> Optional[torch.Tensor]:
        if not self.regul_coef:
            return None
        coefs = self._penalty_coefs()
        return dense.l1l2_penalty([self.W2, self.W1], [coefs, coefs])

    def _components(self):
        return self.mus.detach(), self.sigmas.detach(), self.corxy.detach()

    def _loss(self, L: torch.Tensor, Y: torch.Tensor) -> torch.Tensor:
        return shared_nll_forward_backward(L, Y, *self._components(), want_grad=False)[0]

    def _head_backward(self, h: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        with torch.enable_grad():
            L = self._proj.matmul(h, self.W2, self.b2)
            # W2's penalty gradient; W1's is in the step kernel
            pen2 = dense.l1l2_penalty([self.W2], [self._penalty_coefs()]) \
                if self.regul_coef else None
        nll, dL, dparams, _ = shared_nll_forward_backward(L.detach(), y, *self._components())
        if pen2 is None:
            L.backward(dL)
        else:
            torch.autograd.backward([L, pen2], [dL, torch.ones_like(pen2)])
        self.mus.grad, self.sigmas.grad, self.corxy.grad = split_dparams(dparams)
        return nll

    # -- reference API ------------------------------------------------------------------
    def predict_params(self, X):
        """f_predict (:514): mus [C, 2], sigmas [C, 2], corxy [C], pis [n, C] as NumPy arrays."""
        L = self._output(self._input(X))
        return tuple(t.cpu().numpy() for t in shared_params(L, *self._components()))

    def predict(self, X, prediction_method: str = "mixture"):
        """:676-680 (pred_sharedparams): the selected means, n x 2 (lat, lon), for every row."""
        L = self._output(self._input(X))
        return shared_predict(L, *self._components(), method=prediction_method).cpu().numpy()

