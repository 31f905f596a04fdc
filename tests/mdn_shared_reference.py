"""torch-CPU restatement of the reference's shared-component mixture-density model
(lang2loc_mdnshared.py) -- TEST HELPER.

nll_rows restates nll_loss_sharedparams (:306-327) with build's transforms (:482-487), density /
pred_scores / pred restate pred_sharedparams (:379-414), line by line, in the dtype of their
input (float64 is the judge, float32 the yardstick of what the number format allows), with
autograd for the gradients. softplus and log(softmax(.)) are written in their stable forms
(mdn_reference.softplus, log_softmax), the same functions wherever the reference's are finite;
1 - rho^2 is formed from rho as the reference forms it.

shared_train is the trainer of :450-514, 593-671 in the given dtype (Adam lr 1e-3 on all seven
parameters, the L1/L2 penalty of W1 and W2, the batch order given), optionally fed the dropout
masks of graphconvgeo_amd.dropout.keep_mask_reference. cluster_params_numpy restates
get_cluster_centers (:127-185) after its clustering.
"""
import math

import numpy as np
import scipy.sparse as sps
import torch

from mdn_reference import LR, batches_of, masked_rows, softplus
from oracle import gcn_oracle as GO

NAMES = ["W1", "b1", "W2", "b2", "mus", "sigmas", "corxy"]


def transforms(sigmas_raw, corxy_raw):
    """:484-485: sigmas = softplus(raw), corxy = softsign(raw)."""
    return softplus(sigmas_raw), corxy_raw / (1 + corxy_raw.abs())


def nll_rows(L, Y, mus, sigmas_raw, corxy_raw):
    """:306-327 up to the mean: the loss of every row. L [B, C] logits (pis = softmax)."""
    sigmas, corxy = transforms(sigmas_raw, corxy_raw)
    logpis = torch.log_softmax(L, dim=1)
    mus_ex = mus[None, :, :]
    X = Y[:, None, :]
    diff = X - mus_ex
    diffprod = diff[:, :, 0] * diff[:, :, 1]
    corxy2 = corxy ** 2
    diff2 = diff ** 2
    sigmas2 = sigmas ** 2
    sigmainvs = 1.0 / sigmas
    sigmainvprods = sigmainvs[:, 0] * sigmainvs[:, 1]
    diffsigma = diff2 / sigmas2
    diffsigmanorm = diffsigma.sum(dim=-1)
    z = diffsigmanorm - 2 * corxy * diffprod * sigmainvprods
    oneminuscorxy2inv = 1.0 / (1.0 - corxy2)
    expterm = -0.5 * z * oneminuscorxy2inv
    new_exponent = math.log(0.5 / math.pi) + torch.log(sigmainvprods) + \
        torch.log(torch.sqrt(oneminuscorxy2inv)) + expterm + logpis
    max_exponent = new_exponent.max(dim=1, keepdim=True).values
    gauss_mix = torch.exp(new_exponent - max_exponent).sum(dim=1)
    return -(max_exponent[:, 0] + torch.log(gauss_mix))


def nll(L, Y, mus, sigmas_raw, corxy_raw):
    return nll_rows(L, Y, mus, sigmas_raw, corxy_raw).mean()


def nll_and_grads(L, Y, mus, sigmas_raw, corxy_raw, dtype):
    """(loss rows, [dL, dmus, dsigmas_raw, dcorxy_raw] of the mean) evaluated in `dtype`, as
    float64 NumPy arrays."""
    ts = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
          for a in (L, mus, sigmas_raw, corxy_raw)]
    Yt = torch.tensor(np.asarray(Y), dtype=dtype)
    rows = nll_rows(ts[0], Yt, *ts[1:])
    rows.mean().backward()
    return rows.detach().double().numpy(), [t.grad.double().numpy() for t in ts]


def density(mus, sigmas_raw, corxy_raw):
    """:394-408: probs[i, j], the density of component j at the mean of component i."""
    sigmas, corxy = transforms(sigmas_raw, corxy_raw)
    X = mus[:, None, :]
    diff = X - mus
    diffprod = diff[:, :, 0] * diff[:, :, 1]
    sigmainvs = 1.0 / sigmas
    sigmainvprods = sigmainvs[:, 0] * sigmainvs[:, 1]
    sigmas2 = sigmas ** 2
    corxy2 = corxy ** 2
    diff2 = diff ** 2
    diffsigma = diff2 / sigmas2
    diffsigmanorm = diffsigma.sum(dim=-1)
    z = diffsigmanorm - 2 * corxy * diffprod * sigmainvprods
    oneminuscorxy2inv = 1.0 / (1.0 - corxy2)
    term = -0.5 * z * oneminuscorxy2inv
    return (0.5 / math.pi) * sigmainvprods * torch.sqrt(oneminuscorxy2inv) * torch.exp(term)


def pred_scores(L, mus, sigmas_raw, corxy_raw):
    """:409-410: piprobsum[b, i] = sum_j pis[b, j] * probs[i, j] (the sum over the last axis of
    pis[:, None, :] * probs, written as the product it is)."""
    return torch.softmax(L, dim=1) @ density(mus, sigmas_raw, corxy_raw).T


def pred(L, mus, sigmas_raw, corxy_raw, method="mixture"):
    """:379-426: (component index [B], selected means [B, 2])."""
    score = pred_scores(L, mus, sigmas_raw, corxy_raw) if method == "mixture" else \
        torch.softmax(L, dim=1)
    idx = score.argmax(dim=1)
    return idx, mus[idx]


# -- get_cluster_centers after the clustering --------------------------------------------------
def cluster_params_numpy(latlon, labels, n_cluster, raw=True):
    """:138-185 with labels in place of kmns.labels_ and the members' mean in place of the
    k-means centre; the 1, 1, 0 fallback also where the correlation itself is NaN, and a
    single member's correlation (undefined there) 0. The raw inverses as the reference writes
    them: log(exp(s) - 1) and c / (1 - c sign(c))."""
    latlon = np.asarray(latlon, dtype=np.float64)
    mus = np.zeros((n_cluster, 2), np.float32)
    sigmas = np.zeros((n_cluster, 2), np.float32)
    corxys = np.zeros(n_cluster, np.float32)
    for i in range(n_cluster):
        samples = latlon[np.where(labels == i)[0]]
        mus[i] = samples.mean(axis=0)
        if samples.shape[0] == 1:
            stdlatlat, stdlonlon, corlatlon = 1, 1, 0
        else:
            covmat = np.cov(samples, rowvar=False)
            stdlatlat, stdlonlon, covlatlon = np.sqrt(covmat[0, 0]), np.sqrt(covmat[1, 1]), covmat[0, 1]
            with np.errstate(invalid="ignore", divide="ignore"):
                corlatlon = covlatlon / (stdlatlat * stdlonlon)
            if np.isnan(stdlatlat) or np.isnan(stdlonlon) or np.isnan(covlatlon) or \
                    np.isnan(corlatlon):
                stdlatlat, stdlonlon, corlatlon = 1, 1, 0
        if raw:
            sigmas[i, 0] = np.log(np.exp(stdlatlat) - 1)
            sigmas[i, 1] = np.log(np.exp(stdlonlon) - 1)
            corxys[i] = corlatlon / (1.0 - corlatlon * np.sign(corlatlon))
        else:
            corxys[i] = corlatlon
            sigmas[i, 0] = stdlatlat
            sigmas[i, 1] = stdlonlon
    return mus, sigmas, corxys


# -- the trainer -------------------------------------------------------------------------------
def _logits(Xb, p, dtype):
    Xb = torch.tensor(np.asarray(Xb.todense()), dtype=dtype)
    h = torch.tanh(Xb @ p["W1"] + p["b1"])
    return h @ p["W2"] + p["b2"]


def penalty(p, regul_coef):
    """:495-506: 0.5 shares of regul_coef on the L1 and L2 norms of the output layer's W and the
    hidden layer's W (biases and the Gaussian parameters are not regularizable)."""
    if not regul_coef:
        return 0.0
    return sum(regul_coef * 0.5 * W.abs().sum() + regul_coef * 0.5 * (W ** 2).sum()
               for W in (p["W2"], p["W1"]))


def loss_of(Xb, Yb, p, regul_coef, dtype):
    return nll(_logits(Xb, p, dtype), Yb, p["mus"], p["sigmas"], p["corxy"]) + \
        penalty(p, regul_coef)


def shared_train(X_train, Y_train, X_dev, Y_dev, init, orders, batch, regul_coef, drop=None,
                 dtype=torch.float64):
    """Returns (history, params): per epoch the mean of the batch losses (each before its
    update) and the dev loss over the first (n_dev // batch) * batch rows; the final parameters
    in `dtype`'s NumPy type (no model selection). init: the seven arrays in NAMES' order.
    drop = (p, seed): batch j of the whole run (counted from 0) is masked under step j."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    X_train = sps.csr_matrix(X_train, dtype=np.float32)
    X_dev = sps.csr_matrix(X_dev, dtype=np.float32)
    Yt = torch.tensor(np.asarray(Y_train, dtype=np.float32), dtype=dtype)
    Yd = torch.tensor(np.asarray(Y_dev, dtype=np.float32), dtype=dtype)
    params = {k: np.asarray(v, dtype=npdt) for k, v in zip(NAMES, init)}
    state, hist, step = {}, [], 0
    n_dev = X_dev.shape[0] // batch * batch
    for n, order in enumerate(orders):
        losses = []
        for rows in batches_of(order, batch):
            Xb = X_train[rows] if drop is None else masked_rows(X_train, rows, drop[0], drop[1],
                                                                step)
            step += 1
            p = {k: torch.tensor(v, requires_grad=True) for k, v in params.items()}
            loss = loss_of(Xb, Yt[rows], p, regul_coef, dtype)
            grads = torch.autograd.grad(loss, [p[k] for k in NAMES])
            losses.append(float(loss.detach()))
            params = GO.adam_step(params, {k: g.numpy() for k, g in zip(NAMES, grads)}, state,
                                  lr=LR)
            params = {k: v.astype(npdt) for k, v in params.items()}
        with torch.no_grad():
            p = {k: torch.tensor(v) for k, v in params.items()}
            l_val = loss_of(X_dev[:n_dev], Yd[:n_dev], p, regul_coef, dtype)
        hist.append({"epoch": n, "train_loss": float(np.mean(losses)), "val_loss": float(l_val)})
    return hist, params


# -- the inputs of the GPU sweep (tests/test_mdn_shared_gpu.py) -------------------------------
def sweep_inputs(B, C, regime):
    """float32 NumPy (L, Y, mus, sigmas_raw, corxy_raw) of one (shape, regime), drawn from one
    torch.Generator().manual_seed(77) in the order the test file states. regime "wide": the
    default initialisation's sigmas, "tight": sigmas_raw ~ N(0, 1)."""
    gen = torch.Generator().manual_seed(77)
    span = torch.tensor([60.0, 170.0])
    L = torch.randn(B, C, generator=gen)
    mus = (torch.rand(C, 2, generator=gen) * 2 - 1) * span
    sig = 10 + 10 * torch.rand(C, 2, generator=gen) if regime == "wide" else \
        torch.randn(C, 2, generator=gen)
    cor = torch.randn(C, generator=gen)
    Yu = (torch.rand(B, 2, generator=gen) * 2 - 1) * span
    pick = torch.randint(0, C, (B,), generator=gen)
    Yn = mus[pick] + 2 * torch.randn(B, 2, generator=gen)
    Y = Yu.clone()
    Y[0::2] = Yn[0::2]  # even rows near a mean, odd rows uniform
    return tuple(t.numpy().astype(np.float32) for t in (L, Y, mus, sig, cor))
