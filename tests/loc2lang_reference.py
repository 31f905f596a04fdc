"""torch-CPU restatement of the reference's location-to-language model (loc2lang.py) -- TEST
HELPER.

bigaus restates BivariateGaussianLayer.get_output_for (lasagne_layers.py:187-214) line by line,
soft_xent_rows restates lasagne.objectives.categorical_crossentropy(softmax(z), y) in its literal
form -sum_j y_j log softmax(z)_j (log-softmax written stably: the same function wherever the
reference's is finite), adamax_step writes lasagne.updates.adamax out elementwise, and train is
the trainer of loc2lang.py:159-288 in the given dtype (the batch orders given, no model
selection). Everything runs in the dtype of its input: float64 is the judge, float32 the
yardstick of what the number format allows. softplus is mdn_reference's stable form; 1 - rho^2
is formed from rho as the reference forms it.
"""
import math

import numpy as np
import scipy.sparse as sps
import torch

from mdn_reference import batches_of, softplus

LR = 2e-3  # loc2lang.py:207


def names(hid):
    return ["mus", "sigmas", "corxy"] + (["Wh", "bh"] if hid else []) + ["Wo", "bo"]


def bigaus(X, mus, sigmas_raw, corxy_raw):
    """lasagne_layers.py:187-214: probs [B, C]."""
    sigmas = softplus(sigmas_raw)
    sigmainvs = 1.0 / sigmas
    sigmainvprods = sigmainvs[:, 0] * sigmainvs[:, 1]
    sigmas2 = sigmas ** 2
    diff = X[:, None, :] - mus[None, :, :]
    diffprod = diff[:, :, 0] * diff[:, :, 1]
    corxy = corxy_raw / (1 + corxy_raw.abs())
    corxy2 = corxy ** 2
    diff2 = diff ** 2
    diffsigma = diff2 / sigmas2
    diffsigmanorm = diffsigma.sum(dim=-1)
    z = diffsigmanorm - 2 * corxy * diffprod * sigmainvprods
    oneminuscorxy2inv = 1.0 / (1.0 - corxy2)
    expterm = -0.5 * z * oneminuscorxy2inv
    return torch.exp(math.log(0.5 / math.pi) + torch.log(sigmainvprods) +
                     torch.log(torch.sqrt(oneminuscorxy2inv)) + expterm)


def bigaus_and_grads(X, mus, sigmas_raw, corxy_raw, dG, dtype):
    """(G, [dmus, dsigmas_raw, dcorxy_raw] of sum(dG * G)) evaluated in `dtype`, as float64
    NumPy arrays."""
    ts = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
          for a in (mus, sigmas_raw, corxy_raw)]
    G = bigaus(torch.tensor(np.asarray(X), dtype=dtype), *ts)
    (G * torch.tensor(np.asarray(dG), dtype=dtype)).sum().backward()
    return G.detach().double().numpy(), [t.grad.double().numpy() for t in ts]


def soft_xent_rows(Z, Yd):
    """categorical_crossentropy(softmax(Z), Yd) per row: -sum_j y_j log p_j, Yd dense."""
    return -(Yd * torch.log_softmax(Z, dim=1)).sum(dim=1)


def soft_xent_and_grad(Z, Yd, dtype, scale=1.0):
    """(loss rows, d (scale * sum of the rows) / dZ) in `dtype`, as float64 NumPy arrays."""
    Zt = torch.tensor(np.asarray(Z), dtype=dtype, requires_grad=True)
    rows = soft_xent_rows(Zt, torch.tensor(np.asarray(Yd), dtype=dtype))
    (scale * rows.sum()).backward()
    return rows.detach().double().numpy(), Zt.grad.double().numpy()


def adamax_step(params, grads, state, lr=LR, beta1=0.9, beta2=0.999, eps=1e-8):
    """lasagne.updates.adamax: t += 1; a = lr/(1-b1^t); m = b1 m + (1-b1) g;
    u = max(b2 u, |g|); p -= a m / (u + eps). NumPy, in the arrays' dtype."""
    t = state.get("t", 0) + 1
    state["t"] = t
    a = lr / (1 - beta1 ** t)
    out = {}
    for k, p in params.items():
        g = grads[k]
        m = state.setdefault("m_" + k, np.zeros_like(p))
        u = state.setdefault("u_" + k, np.zeros_like(p))
        m[...] = beta1 * m + (1 - beta1) * g
        u[...] = np.maximum(beta2 * u, np.abs(g))
        out[k] = p - a * m / (u + eps)
    return out


def logits_of(X, p):
    """loc2lang.py:164-187 up to the softmax."""
    h = bigaus(X, p["mus"], p["sigmas"], p["corxy"])
    if "Wh" in p:
        h = torch.relu(h @ p["Wh"] + p["bh"])
    return h @ p["Wo"] + p["bo"]


def loss_of(X, Yd, p):
    return soft_xent_rows(logits_of(X, p), Yd).mean()


def predict(X, params, dtype=torch.float64):
    p = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in params.items()}
    with torch.no_grad():
        return torch.softmax(logits_of(torch.tensor(np.asarray(X), dtype=dtype), p), dim=1).numpy()


def train(X_train, Y_train, X_dev, Y_dev, init, orders, batch, dtype=torch.float64, lr=LR):
    """Returns (history, params): per epoch the batch losses (each before its update), their
    mean and the dev loss over every dev row; the final parameters in `dtype`'s NumPy type (no
    model selection). init: the arrays in names(hid)'s order; hid is read off their number."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    keys = names(len(init) == 7)
    Yt = torch.tensor(np.asarray(sps.csr_matrix(Y_train).todense(), dtype=np.float32), dtype=dtype)
    Yd = torch.tensor(np.asarray(sps.csr_matrix(Y_dev).todense(), dtype=np.float32), dtype=dtype)
    Xt = torch.tensor(np.asarray(X_train, dtype=np.float32), dtype=dtype)
    Xd = torch.tensor(np.asarray(X_dev, dtype=np.float32), dtype=dtype)
    params = {k: np.asarray(v, dtype=npdt) for k, v in zip(keys, init)}
    state, hist = {}, []
    for n, order in enumerate(orders):
        losses = []
        for rows in batches_of(order, batch):
            p = {k: torch.tensor(v, requires_grad=True) for k, v in params.items()}
            loss = loss_of(Xt[rows], Yt[rows], p)
            grads = torch.autograd.grad(loss, [p[k] for k in keys])
            losses.append(float(loss.detach()))
            params = adamax_step(params, {k: g.numpy() for k, g in zip(keys, grads)}, state,
                                 lr=lr)
            params = {k: v.astype(npdt) for k, v in params.items()}
        with torch.no_grad():
            l_val = loss_of(Xd, Yd, {k: torch.tensor(v) for k, v in params.items()})
        hist.append({"epoch": n, "batch_losses": losses, "train_loss": float(np.mean(losses)),
                     "val_loss": float(l_val)})
    return hist, params


def local_words(preds, k):
    """loc2lang.py:755-759 with scipy: normalize(preds, norm='l1', axis=0), stats.entropy,
    argsort."""
    from scipy import stats
    preds = np.asarray(preds, dtype=np.float64)
    norms = np.abs(preds).sum(axis=0)
    norms[norms == 0] = 1.0
    return np.argsort(stats.entropy(preds / norms), kind="stable")[:k]


# -- the inputs of the GPU sweeps (tests/test_loc2lang_gpu.py) ----------------------------------
def layer_inputs(B, C, regime):
    """float32 NumPy (X, mus, sigmas_raw, corxy_raw, dG) of one (shape, regime) from one
    torch.Generator().manual_seed(91). "wide": the layer's default raw sigma 10, means and points
    ~ N(0, 1) and 10 N(0, 1); "tight": cluster-like sigmas 0.05 .. 1 (raw: the inverse softplus)
    with every point scattered around some mean by that component's sigmas."""
    gen = torch.Generator().manual_seed(91)
    cor = torch.randn(C, generator=gen)
    dG = torch.randn(B, C, generator=gen)
    if regime == "wide":
        mus = 10 * torch.randn(C, 2, generator=gen)
        sig = torch.full((C, 2), 10.0)
        X = 10 * torch.randn(B, 2, generator=gen)
    else:
        span = torch.tensor([60.0, 170.0])
        mus = (torch.rand(C, 2, generator=gen) * 2 - 1) * span
        s = 0.05 + 0.95 * torch.rand(C, 2, generator=gen)
        sig = s + torch.log1p(-torch.exp(-s))
        pick = torch.randint(0, C, (B,), generator=gen)
        X = mus[pick] + s[pick] * torch.randn(B, 2, generator=gen)
    return tuple(t.numpy().astype(np.float32) for t in (X, mus, sig, cor, dG))


def xent_inputs(M, N, spread, seed=5):
    """(Z float32 [M, N], Y scipy CSR float32 [M + 3, N], rows int32 [M]): logits spread * N(0, 1);
    target rows that cycle through empty, one entry, a few, and (N <= 257) full, l1-normalised
    where not empty; rows pairs logits row i with a target row, with repeats and out of order."""
    rng = np.random.default_rng(seed + 1000 * M + N)
    Z = (spread * rng.standard_normal((M, N))).astype(np.float32)
    n_y = M + 3
    data, indices, indptr = [], [], [0]
    for r in range(n_y):
        kind = r % 4
        nnz = (0, 1, min(N, 5), N if N <= 257 else min(N, 40))[kind]
        cols = np.sort(rng.choice(N, size=nnz, replace=False))
        vals = rng.random(nnz) + 0.05
        if nnz:
            vals = vals / vals.sum()
        indices.extend(cols)
        data.extend(vals)
        indptr.append(len(indices))
    Y = sps.csr_matrix((np.asarray(data, np.float32), np.asarray(indices, np.int32),
                        np.asarray(indptr, np.int32)), shape=(n_y, N))
    rows = rng.integers(0, n_y, size=M).astype(np.int32)
    # every kind appears when M >= 4; a single row holds a few entries
    rows[: min(M, 4)] = ((np.arange(min(M, 4)) + 2) % 4)[::-1]
    return Z, Y, rows


MELBOURNES = np.array([[28.0836, -80.6081], [-37.8136, 144.9631]])  # Florida, Australia


def two_regions_data(n_train=400, n_dev=100, seed=11):
    """Points around the two Melbournes (sigma 0.5 degrees, the places alternating) and their
    words: V = 20, words 0-7 belong to the first place, 8-15 to the second, 16-19 to both; a row
    holds 3 of its place's words and 1 common word, 0.25 each. Returns (X_train, Y_train, X_dev,
    Y_dev) with Y as scipy CSR."""
    rng = np.random.default_rng(seed)
    n = n_train + n_dev
    place = np.arange(n) % 2
    X = (MELBOURNES[place] + 0.5 * rng.standard_normal((n, 2))).astype(np.float32)
    Yd = np.zeros((n, 20), np.float32)
    for r in range(n):
        own = 8 * place[r] + rng.choice(8, size=3, replace=False)
        Yd[r, own] = 0.25
        Yd[r, 16 + rng.integers(0, 4)] = 0.25
    Y = sps.csr_matrix(Yd)
    return X[:n_train], Y[:n_train], X[n_train:], Y[n_train:]


def two_regions_init(components, hid, seed=5, V=20):
    """init in names(hid)'s order from cluster_params' (mus, sigmas, corxy) and GlorotUniform
    weights of a RandomState(seed)."""
    rs = np.random.RandomState(seed)
    C = components[0].shape[0]
    init = list(components)
    for fan_in, fan_out in ([(C, hid)] if hid else []) + [(hid or C, V)]:
        a = np.sqrt(6.0 / (fan_in + fan_out))
        init += [rs.uniform(-a, a, size=(fan_in, fan_out)).astype(np.float32),
                 np.zeros(fan_out, np.float32)]
    return init


def own_word_margin(probs):
    """probs [2, 20], the predictions at the two centres: per centre the mass on its own 8 words
    minus the mass on the other place's 8."""
    a, b = probs[:, :8].sum(axis=1), probs[:, 8:16].sum(axis=1)
    return np.array([a[0] - b[0], b[1] - a[1]])


def parity_problem(seed=0, tight=True, hid=8, n=96, n_dev=40, B=32, C=5, V=37, epochs=8):
    """The trainer-parity problem: n training and n_dev dev coordinates around C centres, 0-5
    words per row (l1-normalised), init in names(hid)'s order, one permutation per epoch."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-1, 1, size=(C, 2)) * np.array([50.0, 150.0])
    place = rng.integers(0, C, size=n + n_dev)
    X = (centres[place] + rng.standard_normal((n + n_dev, 2))).astype(np.float32)
    Yd = np.zeros((n + n_dev, V), np.float32)
    for r in range(n + n_dev):
        k = rng.integers(0, 6)
        if k:
            cols = rng.choice(V, size=k, replace=False)
            w = rng.random(k) + 0.1
            Yd[r, cols] = w / w.sum()
    Y = sps.csr_matrix(Yd)
    mus = (centres + 0.3 * rng.standard_normal((C, 2))).astype(np.float32)
    if tight:
        s = rng.uniform(0.8, 1.5, size=(C, 2))
        sigmas = (s + np.log1p(-np.exp(-s))).astype(np.float32)
    else:
        sigmas = np.full((C, 2), 10.0, np.float32)
    corxy = (0.3 * rng.standard_normal(C)).astype(np.float32)
    init = [mus, sigmas, corxy]

    def glorot(a, b):
        lim = np.sqrt(6.0 / (a + b))
        return rng.uniform(-lim, lim, size=(a, b)).astype(np.float32)

    if hid:
        init += [glorot(C, hid), np.zeros(hid, np.float32)]
    init += [glorot(hid or C, V), np.zeros(V, np.float32)]
    orders = [rng.permutation(n) for _ in range(epochs)]
    return X[:n], Y[:n], X[n:], Y[n:], init, orders, B
