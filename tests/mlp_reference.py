"""float64 NumPy restatement of the reference's mini-batch MLP (mlp.py:96-311) -- TEST HELPER.

The per-batch step is the GCN oracle's with H = identity: oracle.gcn_oracle.gcn_forward /
gcn_loss / gcn_backward on the batch's rows, then adam_step(lr=0.002) (mlp.py:244). Without a
hidden layer the model is a sparse softmax regression (mlp.py:192-194), written out here.
Batches follow iterate_minibatches (mlp.py:81-91): order[s:s+B] for s in range(0, n-B+1, B), the
tail dropped; the reported train loss is the last batch's (before its update), the validation
loss / accuracy are f_val on dev after the epoch's last update (mlp.py:268-280).
"""
import numpy as np
import scipy.sparse as sps

from oracle import gcn_oracle as O

LR = 0.002


def batches_of(order, batch):
    n = len(order)
    return [np.asarray(order[s:s + batch]) for s in range(0, n - batch + 1, batch)]


def _softreg_loss(P, y, W, c_out):
    ce = -np.log(P[np.arange(P.shape[0]), y]).mean()
    return ce + np.abs(W).sum() * c_out * 0.5 + (W ** 2).sum() * c_out * 0.5


def _evaluate(X, y, params, regul_coefs, add_hidden):
    X = sps.csr_matrix(X, dtype=np.float64)
    n = X.shape[0]
    if add_hidden:
        f = O.gcn_forward(X, sps.identity(n, format="csr"), params["W1"], params["b1"],
                          params["W2"], params["b2"], np.arange(n))
        loss = O.gcn_loss(f["P"], y, params["W1"], params["W2"], regul_coefs)
        return float(loss), float((f["logits"].argmax(axis=1) == y).mean())
    logits = X @ params["W1"] + params["b1"]
    P = O.softmax(logits)
    return float(_softreg_loss(P, y, params["W1"], regul_coefs[0])), \
        float((logits.argmax(axis=1) == y).mean())


def mlp_train(X_train, Y_train, X_dev, Y_dev, init, orders, batch, regul_coefs,
              add_hidden=True):
    """Returns (history, params): per epoch train_loss / train_acc (last batch) and val_loss /
    val_acc; the final float64 parameters (no model selection)."""
    X_train = sps.csr_matrix(X_train, dtype=np.float64)
    Y_train, Y_dev = np.asarray(Y_train), np.asarray(Y_dev)
    names = ["W1", "b1", "W2", "b2"] if add_hidden else ["W1", "b1"]
    params = {k: np.asarray(v, dtype=np.float64) for k, v in zip(names, init)}
    eye = sps.identity(batch, format="csr")
    idx = np.arange(batch)
    state, hist = {}, []
    for n, order in enumerate(orders):
        loss = acc = None
        for rows in batches_of(order, batch):
            Xb, y = X_train[rows], Y_train[rows]
            if add_hidden:
                f = O.gcn_forward(Xb, eye, params["W1"], params["b1"], params["W2"], params["b2"],
                                  idx)
                loss = O.gcn_loss(f["P"], y, params["W1"], params["W2"], regul_coefs)
                acc = (f["logits"].argmax(axis=1) == y).mean()
                g = O.gcn_backward(Xb, eye, params["W1"], params["W2"], f, idx, y, regul_coefs)
            else:
                c_out = regul_coefs[0]
                W = params["W1"]
                logits = Xb @ W + params["b1"]
                P = O.softmax(logits)
                loss = _softreg_loss(P, y, W, c_out)
                acc = (logits.argmax(axis=1) == y).mean()
                G = P.copy()
                G[idx, y] -= 1.0
                G /= batch
                g = {"W1": Xb.T @ G + c_out * 0.5 * np.sign(W) + c_out * W, "b1": G.sum(axis=0)}
            params = O.adam_step(params, {k: g[k] for k in params}, state, lr=LR)
        l_val, a_val = _evaluate(X_dev, Y_dev, params, regul_coefs, add_hidden)
        hist.append({"epoch": n, "train_loss": float(loss), "train_acc": float(acc),
                     "val_loss": l_val, "val_acc": a_val})
    return hist, params
