"""float64 NumPy restatement of the mini-batch MLP's step under given dropout masks (the
reference's MLP(drop_out=True), mlp.py:164-183, 203-226) -- TEST HELPER.

A mask is given as its multiplier: keep * scale (scale = 1 / (1 - p), Lasagne's rescale), 0 where
the element is dropped; None stands for all ones. The input's multiplier has the batch's shape
[B, F] (only the stored entries of X matter), the hidden one [B, K]. The model is
mlp_reference's with a hidden layer:

    pre1 = (X * m_in) . W1 + b1,  h = rectify(pre1),  hd = h * m_hid,  P = softmax(hd . W2 + b2)
    loss = mean CE + the L1/L2 penalty of W2 and W1 (oracle.gcn_oracle.gcn_loss)

and the gradients follow Theano's rules as oracle.gcn_oracle.gcn_backward states them (the
rectify gradient is 0.5 * (1 + sgn(pre1))); a mask multiplies the gradient where it multiplied
the value. The loop around the step -- batches, Adam, the reported figures, the deterministic
validation -- is mlp_reference.mlp_train's.
"""
import numpy as np
import scipy.sparse as sps

import mlp_reference as R
from oracle import gcn_oracle as O


def dropout_step(Xb, y, params, regul_coefs, m_in=None, m_hid=None):
    """(loss, accuracy, gradients) of one batch under the two multipliers."""
    c_out, c_hid = regul_coefs
    Xb = sps.csr_matrix(Xb, dtype=np.float64)
    if m_in is not None:
        Xb = sps.csr_matrix(Xb.multiply(np.asarray(m_in, dtype=np.float64)))
    W1, b1, W2, b2 = (params[k] for k in ("W1", "b1", "W2", "b2"))
    B = Xb.shape[0]
    m_hid = np.ones((B, W1.shape[1])) if m_hid is None else np.asarray(m_hid, dtype=np.float64)
    pre1 = Xb @ W1 + b1
    hd = O.relu(pre1) * m_hid
    logits = hd @ W2 + b2
    P = O.softmax(logits)
    loss = O.gcn_loss(P, y, W1, W2, regul_coefs)
    acc = (logits.argmax(axis=1) == y).mean()
    G = P.copy()
    G[np.arange(B), y] -= 1.0
    G /= B
    g_pre1 = (G @ W2.T) * m_hid * 0.5 * (1.0 + np.sign(pre1))
    grads = {"W2": hd.T @ G + c_out * 0.5 * np.sign(W2) + c_out * W2, "b2": G.sum(axis=0),
             "W1": Xb.T @ g_pre1 + c_hid * 0.5 * np.sign(W1) + c_hid * W1,
             "b1": g_pre1.sum(axis=0)}
    return float(loss), float(acc), grads


def mlp_dropout_train(X_train, Y_train, X_dev, Y_dev, init, orders, batch, regul_coefs,
                      mask_in=None, mask_hid=None):
    """mlp_reference.mlp_train with masks: mask_in(step, rows) and mask_hid(step) return the
    multipliers of the batch trained as step number `step` (counted from 0 across epochs), or
    None. Returns (history, params)."""
    X_train = sps.csr_matrix(X_train, dtype=np.float64)
    Y_train, Y_dev = np.asarray(Y_train), np.asarray(Y_dev)
    params = {k: np.asarray(v, dtype=np.float64) for k, v in zip(("W1", "b1", "W2", "b2"), init)}
    state, hist, step = {}, [], 0
    for n, order in enumerate(orders):
        loss = acc = None
        for rows in R.batches_of(order, batch):
            loss, acc, g = dropout_step(X_train[rows], Y_train[rows], params, regul_coefs,
                                        None if mask_in is None else mask_in(step, rows),
                                        None if mask_hid is None else mask_hid(step))
            params = O.adam_step(params, g, state, lr=R.LR)
            step += 1
        l_val, a_val = R._evaluate(X_dev, Y_dev, params, regul_coefs, True)
        hist.append({"epoch": n, "train_loss": loss, "train_acc": acc, "val_loss": l_val,
                     "val_acc": a_val})
    return hist, params


def stream_masks(model, F, K, batch):
    """(mask_in, mask_hid) for mlp_dropout_train: the multipliers a fitted DropoutMLP applied,
    regenerated from its streams' seeds with the NumPy statement of the rule
    (DropoutStream.keep_mask). A layer without a mask gives None."""
    def mask_in(step, rows):
        keep = model.stream_in.keep_mask(np.asarray(rows)[:, None], np.arange(F)[None, :],
                                         model._drop_in.p, step)
        return keep * np.float64(np.float32(model._drop_in.scale))

    def mask_hid(step):
        keep = model.stream_hid.keep_mask(np.arange(batch)[:, None], np.arange(K)[None, :],
                                          model._drop_hid.p, step)
        return keep * np.float64(np.float32(model._drop_hid.scale))

    return (mask_in if model._drop_in is not None else None,
            mask_hid if model._drop_hid is not None else None)
