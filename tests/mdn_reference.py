"""torch-CPU restatement of the reference's mixture-density head (lang2loc.py) -- TEST HELPER.

unpack_params / nll_rows restate lang2loc.py:143-196 and pred_scores / pred lang2loc.py:198-244
line by line, in the dtype of their input (float64 is the judge, float32 the yardstick of what
the number format allows), with autograd for the gradients. Two expressions are written in
their stable forms, which are the same functions wherever the reference's are finite: softplus
as max(x, 0) + log1p(exp(-|x|)) and log(softmax(.)) as log_softmax. 1 - rho^2 is formed from
rho as the reference forms it. Theano is not importable here, so parity with the reference
rests on this restatement.

mdn_train is the float64 trainer of lang2loc.py:270-331, 408-455 (Adam lr 1e-3, the hidden
layer's L1/L2 penalty only, the batch order given), optionally fed the dropout masks of
graphconvgeo_amd.dropout.keep_mask_reference.
"""
import math

import numpy as np
import scipy.sparse as sps
import torch

from graphconvgeo_amd.dropout import dropout_scale, keep_mask_reference
from oracle import gcn_oracle as GO

LR = 1e-3
MU_SCALE = (90.0, 180.0)


def softplus(x):
    """max(x, 0) + log1p(exp(-|x|)), with max(x, 0) written as (x + |x|) / 2 (exact in binary
    floating point): autograd then gives the derivative sigmoid(x) at x == 0 too, where
    clamp's and abs's subgradients would add up to 1 instead of 1/2."""
    return (x + x.abs()) / 2 + torch.log1p(torch.exp(-x.abs()))


def unpack_params(O, n_comp, log_pis=False):
    """lang2loc.py:143-160. O: [B, 6 * n_comp]. Returns mus [B, 2, C], sigmas [B, 2, C],
    corxy [B, C], pis [B, C] (log pis with log_pis)."""
    O = O.reshape(-1, 6, n_comp)
    scale = torch.tensor(MU_SCALE, dtype=O.dtype)[None, :, None]
    mus = scale * torch.tanh(O[:, 0:2, :])
    sigmas = 10 * softplus(O[:, 2:4, :])
    corxy = O[:, 4, :] / (1 + O[:, 4, :].abs())  # softsign
    pis = torch.log_softmax(O[:, 5, :], dim=1) if log_pis else torch.softmax(O[:, 5, :], dim=1)
    return mus, sigmas, corxy, pis


def nll_rows(O, Y, n_comp):
    """lang2loc.py:166-196 up to the mean: the loss of every row."""
    mus, sigmas, corxy, logpis = unpack_params(O, n_comp, log_pis=True)
    diff = Y[:, :, None] - mus
    diffprod = diff[:, 0, :] * diff[:, 1, :]
    sigmainvs = 1.0 / sigmas
    sigmainvprods = sigmainvs[:, 0, :] * sigmainvs[:, 1, :]
    diffsigma = diff ** 2 * (1.0 / sigmas ** 2)
    z = diffsigma.sum(dim=1) - 2 * corxy * diffprod * sigmainvprods
    oneminuscorxy2inv = 1.0 / (1.0 - corxy ** 2)
    exponent = -0.5 * z * oneminuscorxy2inv
    new_exponent = exponent + math.log(0.5 / math.pi) + torch.log(sigmainvprods) + \
        torch.log(torch.sqrt(oneminuscorxy2inv)) + logpis
    max_exponent = new_exponent.max(dim=1, keepdim=True).values
    gauss_mix = torch.exp(new_exponent - max_exponent).sum(dim=1)
    return -(max_exponent[:, 0] + torch.log(gauss_mix))


def nll(O, Y, n_comp):
    return nll_rows(O, Y, n_comp).mean()


def nll_and_grad(O, Y, n_comp, dtype):
    """(loss rows, gradient of the mean with respect to O) evaluated in `dtype`, as float64
    NumPy arrays."""
    Ot = torch.tensor(np.asarray(O), dtype=dtype, requires_grad=True)
    Yt = torch.tensor(np.asarray(Y), dtype=dtype)
    rows = nll_rows(Ot, Yt, n_comp)
    rows.mean().backward()
    return rows.detach().double().numpy(), Ot.grad.double().numpy()


def _pred_scores(mus, sigmas, corxy, pis):
    X = mus[:, :, :, None]
    musex = mus[:, :, None, :]
    sigmasex = sigmas[:, :, :, None]
    corxysex = corxy[:, :, None]
    diff = X - musex
    diffprod = diff[:, 0] * diff[:, 1]
    sigmainvs = 1.0 / sigmasex
    sigmainvprods = sigmainvs[:, 0] * sigmainvs[:, 1]
    diffsigma = diff ** 2 / (sigmas ** 2)[:, :, :, None]
    z = diffsigma.sum(dim=1) - 2 * corxysex * diffprod * sigmainvprods
    oneminuscorxy2inv = 1.0 / (1.0 - corxysex ** 2)
    probs = (0.5 / math.pi) * sigmainvprods * torch.sqrt(oneminuscorxy2inv) * \
        torch.exp(-0.5 * z * oneminuscorxy2inv)
    return (pis[:, :, None] * probs).sum(dim=1)


def pred_scores(O, n_comp):
    """lang2loc.py:204-225: piprobsum[b, k], the mixture density at the mean of component k,
    in the reference's non-log form (rows taken a few at a time: the intermediates are
    [rows, 2, C, C])."""
    params = unpack_params(O, n_comp)
    step = max(1, (1 << 21) // (n_comp * n_comp))
    return torch.cat([_pred_scores(*(t[s:s + step] for t in params))
                      for s in range(0, O.shape[0], step)])


def pred(O, n_comp, method="mixture"):
    """lang2loc.py:198-244: (component index [B], selected means [B, 2])."""
    mus, _sigmas, _corxy, pis = unpack_params(O, n_comp)
    idx = (pred_scores(O, n_comp) if method == "mixture" else pis).argmax(dim=1)
    return idx, mus[torch.arange(mus.shape[0]), :, idx]


# -- the mean's fixed order (include/gcg_spmm.h) ---------------------------------------------
def fixed_order_mean(rows: np.ndarray) -> np.float32:
    """The float32 mean of gcg_mdn_nll_f32: thread t of 256 adds the rows t, t + 256, ... in
    order, a halving tree adds the partials, the sum is divided by B."""
    rows = np.asarray(rows, dtype=np.float32)
    part = np.zeros(256, np.float32)
    for t in range(min(256, rows.size)):
        s = np.float32(0)
        for v in rows[t::256]:
            s = np.float32(s + v)
        part[t] = s
    h = 128
    while h:
        part[:h] = part[:h] + part[h:2 * h]
        h //= 2
    return np.float32(part[0] / np.float32(rows.size))


# -- input dropout at segmentation -----------------------------------------------------------
def masked_rows(X, rows, p, seed, step, stream_id=0):
    """X[rows] (float32 CSR, storage order kept) under the package's keep rule: logical row =
    the row's id in X, logical column = its column; keep ? fl32(v * scale) : +0.0."""
    X = sps.csr_matrix(X, dtype=np.float32)
    rows = np.asarray(rows)
    lens = np.diff(X.indptr)[rows]
    src = np.concatenate([np.arange(X.indptr[r], X.indptr[r + 1]) for r in rows] or
                         [np.zeros(0, np.int64)]).astype(np.int64)
    ids = np.repeat(rows, lens)
    cols = X.indices[src]
    keep = keep_mask_reference(ids, cols, p, seed, step, stream_id)
    scale = np.float32(dropout_scale(p))
    data = np.where(keep, (X.data[src] * scale).astype(np.float32), np.float32(0.0))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return sps.csr_matrix((data.astype(np.float32), cols.copy(), indptr),
                          shape=(len(rows), X.shape[1]))


# -- the float64 trainer ---------------------------------------------------------------------
def batches_of(order, batch):
    n = len(order)
    return [np.asarray(order[s:s + batch]) for s in range(0, n - batch + 1, batch)]


def _forward(Xb, params):
    Xb = torch.tensor(np.asarray(Xb.todense()), dtype=torch.float64)
    h = torch.tanh(Xb @ params["W1"] + params["b1"])
    return h @ params["W2"] + params["b2"]


def _penalty(W1, regul_coef):
    if not regul_coef:
        return 0.0
    return regul_coef * 0.5 * W1.abs().sum() + regul_coef * 0.5 * (W1 ** 2).sum()


def mdn_train(X_train, Y_train, X_dev, Y_dev, init, orders, batch, n_comp, regul_coef,
              drop=None):
    """Returns (history, params): per epoch the mean of the batch losses (each before its
    update) and the dev loss over the first (n_dev // batch) * batch rows; the final float64
    parameters (no model selection). drop = (p, seed): batch j of the whole run (counted from
    0 across the epochs) is masked under step j."""
    X_train = sps.csr_matrix(X_train, dtype=np.float32)
    X_dev = sps.csr_matrix(X_dev, dtype=np.float32)
    Yt = torch.tensor(np.asarray(Y_train, dtype=np.float32), dtype=torch.float64)
    Yd = torch.tensor(np.asarray(Y_dev, dtype=np.float32), dtype=torch.float64)
    names = ["W1", "b1", "W2", "b2"]
    params = {k: np.asarray(v, dtype=np.float64) for k, v in zip(names, init)}
    state, hist, step = {}, [], 0
    n_dev = X_dev.shape[0] // batch * batch
    for n, order in enumerate(orders):
        losses = []
        for rows in batches_of(order, batch):
            Xb = X_train[rows] if drop is None else masked_rows(X_train, rows, drop[0], drop[1],
                                                                step)
            step += 1
            p = {k: torch.tensor(v, requires_grad=True) for k, v in params.items()}
            loss = nll(_forward(Xb, p), Yt[rows], n_comp) + _penalty(p["W1"], regul_coef)
            grads = torch.autograd.grad(loss, [p[k] for k in names])
            losses.append(float(loss.detach()))
            params = GO.adam_step(params, {k: g.numpy() for k, g in zip(names, grads)}, state,
                                  lr=LR)
        with torch.no_grad():
            p = {k: torch.tensor(v) for k, v in params.items()}
            l_val = nll(_forward(X_dev[:n_dev], p), Yd[:n_dev], n_comp) + \
                _penalty(p["W1"], regul_coef)
        hist.append({"epoch": n, "train_loss": float(np.mean(losses)), "val_loss": float(l_val)})
    return hist, params
