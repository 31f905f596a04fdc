"""float64 restatement of oracle.gcn_oracle.mlpconv_train with an optional rounding of the four
dense operands the H-products gather (MLPCONV(gather_dtype="bfloat16")): Z1 and Z2 in the
forward, the pre-activation gradients g_pre2 and g_pre1 in the backward. The rounding is
treated as the identity by the backward, and the bias gradients read the unrounded gradient,
as the layers do. Without a rounding function every operation is oracle.mlpconv_train's.

bf16r is torch's CPU round-to-nearest-even conversion, the independent witness of the GPU
conversion kernel (tests/test_spmm_bf16_gpu.py)."""
import numpy as np
import scipy.sparse as sps
import torch

from oracle import gcn_oracle as O


def bf16r(x):
    """x rounded to bfloat16 and widened again (through float32), in x's dtype."""
    x = np.asarray(x)
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    return torch.from_numpy(x32).to(torch.bfloat16).float().numpy().astype(x.dtype)


def _forward(Xd, Hd, p, idx, rnd):
    Z1 = Xd @ p["W1"]
    pre1 = Hd @ rnd(Z1) + p["b1"]
    h = O.relu(pre1)
    Z2 = h @ p["W2"]
    pre2 = Hd @ rnd(Z2) + p["b2"]
    logits = pre2[idx]
    return {"pre1": pre1, "h": h, "pre2": pre2, "logits": logits, "P": O.softmax(logits)}


def _backward(Xd, Hd, p, f, idx, y, regul_coefs, rnd):
    c_out, c_hid = regul_coefs
    T = idx.size
    g_logits = f["P"].copy()
    g_logits[np.arange(T), y] -= 1.0
    g_logits /= T
    g_pre2 = np.zeros(f["pre2"].shape, dtype=np.float64)
    np.add.at(g_pre2, idx, g_logits)
    g_b2 = g_pre2.sum(axis=0)
    g_Z2 = Hd.T @ rnd(g_pre2)
    g_W2 = f["h"].T @ g_Z2 + c_out * 0.5 * np.sign(p["W2"]) + c_out * p["W2"]
    g_h = g_Z2 @ p["W2"].T
    g_pre1 = g_h * 0.5 * (1.0 + np.sign(f["pre1"]))
    g_b1 = g_pre1.sum(axis=0)
    g_Z1 = Hd.T @ rnd(g_pre1)
    g_W1 = Xd.T @ g_Z1 + c_hid * 0.5 * np.sign(p["W1"]) + c_hid * p["W1"]
    return {"W1": g_W1, "b1": g_b1, "W2": g_W2, "b2": g_b2}


def mlpconv_train(X, H, Y, train_idx, dev_idx, W1, b1, W2, b2, n_epochs, regul_coefs,
                  report_k_epoch=10, round_operand=None):
    """oracle.mlpconv_train's loop; round_operand (e.g. bf16r) is applied to the four gathered
    operands. Returns (history, params) as the oracle does."""
    rnd = (lambda a: a) if round_operand is None else round_operand
    Xd = sps.csr_matrix(X, dtype=np.float64)
    Hd = sps.csr_matrix(H, dtype=np.float64)
    params = {"W1": W1.astype(np.float64), "b1": b1.astype(np.float64),
              "W2": W2.astype(np.float64), "b2": b2.astype(np.float64)}
    Y = np.asarray(Y)
    train_idx, dev_idx = np.asarray(train_idx), np.asarray(dev_idx)
    state, hist = {}, []
    for n in range(n_epochs):
        f = _forward(Xd, Hd, params, train_idx, rnd)
        y = Y[train_idx]
        loss = O.gcn_loss(f["P"], y, params["W1"], params["W2"], regul_coefs)
        acc = float((f["logits"].argmax(axis=1) == y).mean())
        g = _backward(Xd, Hd, params, f, train_idx, y, regul_coefs, rnd)
        rec = {"epoch": n, "train_loss": float(loss), "train_acc": acc}
        params = O.adam_step(params, g, state)
        if n % report_k_epoch == 0:
            fv = _forward(Xd, Hd, params, dev_idx, rnd)
            yd = Y[dev_idx]
            rec["val_loss"] = float(O.gcn_loss(fv["P"], yd, params["W1"], params["W2"],
                                               regul_coefs))
            rec["val_acc"] = float((fv["logits"].argmax(axis=1) == yd).mean())
        hist.append(rec)
    return hist, params


def rounding_sensitivity(X, H, Y, train_idx, dev_idx, init, n_epochs, regul_coefs):
    """d = max over epochs of |loss_rounded - loss_plain| / max(1, |loss_plain|): how far the
    float64 model's own loss trajectory moves under the bf16 rounding of the four operands."""
    plain, _ = mlpconv_train(X, H, Y, train_idx, dev_idx, *init, n_epochs=n_epochs,
                             regul_coefs=regul_coefs)
    rounded, _ = mlpconv_train(X, H, Y, train_idx, dev_idx, *init, n_epochs=n_epochs,
                               regul_coefs=regul_coefs, round_operand=bf16r)
    a = np.array([h["train_loss"] for h in plain])
    b = np.array([h["train_loss"] for h in rounded])
    return float((np.abs(b - a) / np.maximum(1.0, np.abs(a))).max())
