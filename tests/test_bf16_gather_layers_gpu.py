"""gather_dtype="bfloat16" through the layers and the MLPCONV trainer: the H-products gather a
bfloat16 copy of their dense operand (forward) or of the incoming gradient (backward), rounded
once; everything else stays float32. Bitwise against the oracle on the rounded operands, and
the trainer's loss trajectory against the float64 oracle within a bar derived from the float64
model's own sensitivity to that rounding (tests/bf16_gather_reference.py)."""
import functools

import numpy as np
import pytest
import torch

from bf16_gather_reference import bf16r
from graphconvgeo_amd import sparse as gs
from graphconvgeo_amd.layers import (ConvolutionDenseLayer, SparseConvolutionDenseLayer,
                                     csr_matmul)
from graphconvgeo_amd.mlpconv import MLPCONV
from oracle import gcn_oracle as O
from test_mlpconv_gpu import problem
from test_spmm_gpu import to_dev

pytestmark = pytest.mark.gpu

# d = max_epoch |loss_rounded64 - loss_plain64| / max(1, |loss_plain64|) of the float64 model on
# problem() (n = 4000, k = 48, c = 9), 10 epochs, regul_coefs (1e-5, 1e-5): measured on the CPU
# with bf16_gather_reference.rounding_sensitivity (8.7545e-06; profiles/bf16_gather/README.md).
ROUNDING_SENSITIVITY_D = 8.7545e-06
TRAJECTORY_BAR = 4 * ROUNDING_SENSITIVITY_D + 1e-4  # + the float32 bar of test_mlpconv_gpu.py


def test_layer_forward_bitwise(cuda):
    H, X, _Y, _tr, _dev, _te, (W1, b1, _W2, _b2) = problem(n=2000, e=12000, f=150, k=40, c=5)
    b1 = np.random.default_rng(1).standard_normal(40).astype(np.float32) * 0.1
    layer = SparseConvolutionDenseLayer(150, H=H, num_units=40, W=W1, b=b1, device=cuda,
                                        mode="ordered", gather_dtype="bfloat16")
    with torch.no_grad():
        got = layer(X).cpu().numpy()
    want = O.relu(O.spmm_f32(H, bf16r(O.spmm_f32(X, W1)), bias=b1))
    assert np.array_equal(got, want)
    plain = SparseConvolutionDenseLayer(150, H=H, num_units=40, W=W1, b=b1, device=cuda,
                                        mode="ordered")
    with torch.no_grad():
        assert not np.array_equal(plain(X).cpu().numpy(), want)  # the rounding is real


@pytest.mark.parametrize("operator", ["symmetric", "rownorm"])
def test_layer_backward_bitwise(cuda, operator):
    H, _X, _Y, _tr, _dev, _te, _init = problem(n=2000, e=12000, f=150, k=40, c=5)
    if operator == "rownorm":
        A1 = H.copy()
        A1.data[:] = 1.0
        H = O.row_normalize_l1(A1)  # not symmetric: the backward runs on the built transpose
    n, K = H.shape[0], 40
    rng = np.random.default_rng(3)
    Z = rng.standard_normal((n, K)).astype(np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    A = gs.DeviceCSR.from_scipy(H, cuda)

    def run(rows, **kw):
        Zd = to_dev(Z, cuda).requires_grad_()
        bd = to_dev(b, cuda).requires_grad_()
        Y = csr_matmul(A, Zd, bd, None, rows, "ordered", **kw)
        g = np.random.default_rng(4).standard_normal(tuple(Y.shape)).astype(np.float32)
        Y.backward(to_dev(g, cuda))
        return Y.detach().cpu().numpy(), Zd.grad.cpu().numpy(), bd.grad.cpu().numpy(), g

    Y, gZ, gb, g = run(None, gather_dtype="bfloat16")
    assert np.array_equal(Y, O.spmm_f32(H, bf16r(Z), bias=b))
    assert np.array_equal(gZ, O.spmm_f32(H.T.tocsr(), bf16r(g)))
    assert np.array_equal(gb, run(None)[2])  # the bias gradient reads the float32 gradient
    rows = np.random.default_rng(5).integers(0, n, size=700).astype(np.int32)
    rows[:4] = 5
    sel = gs.RowSelection(rows, cuda)
    Y, gZ, gb, g = run(sel, gather_dtype="bfloat16")
    assert np.array_equal(Y, O.spmm_f32(H, bf16r(Z), bias=b, rows=rows))
    assert np.array_equal(gZ, O.spmm_f32(H[rows].T.tocsr(), bf16r(g)))
    assert np.array_equal(gb, run(sel)[2])


def test_float32_untouched(cuda):
    H, _X, _Y, _tr, _dev, _te, _init = problem(n=2000, e=12000, f=150, k=40, c=5)
    n, K = H.shape[0], 40
    rng = np.random.default_rng(7)
    Z = rng.standard_normal((n, K)).astype(np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    g = rng.standard_normal((n, K)).astype(np.float32)
    A = gs.DeviceCSR.from_scipy(H, cuda)
    outs = []
    for kw in ({}, {"gather_dtype": "float32"}):
        Zd = to_dev(Z, cuda).requires_grad_()
        bd = to_dev(b, cuda).requires_grad_()
        Y = csr_matmul(A, Zd, bd, "relu", None, "ordered", **kw)
        Y.backward(to_dev(g, cuda))
        outs.append((Y.detach(), Zd.grad, bd.grad))
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    assert np.array_equal(outs[0][0].cpu().numpy(), O.spmm_f32(H, Z, bias=b, act="relu"))


COEFS = (1e-5, 1e-5)


@functools.lru_cache(maxsize=None)
def trainer_reference():
    """problem() and the float64 oracle's loss trajectory on it, computed once."""
    prob = problem()
    H, X, Y, train, dev, _test, init = prob
    hist, _ = O.mlpconv_train(X, H, Y, train, dev, *init, n_epochs=10, regul_coefs=COEFS)
    ref = np.array([h["train_loss"] for h in hist])
    ref.setflags(write=False)
    return prob, ref


@pytest.mark.parametrize("order", ["reference", "propagate_first"])
def test_trainer_bf16_gather(cuda, order):
    (H, X, Y, train, dev, test, init), ref = trainer_reference()
    coefs = COEFS
    kw = dict(n_epochs=10, hidden_layer_size=48, regul_coefs=coefs, init_parameters=init,
              device=cuda, order=order, gather_dtype="bfloat16")
    runs = [MLPCONV(**kw).fit(X, train, dev, test, Y, H) for _ in range(2)]
    graph = MLPCONV(use_graph=True, **kw).fit(X, train, dev, test, Y, H)
    got = [h["train_loss"] for h in runs[0].history]
    assert got == [h["train_loss"] for h in runs[1].history]  # deterministic
    assert got == [h["train_loss"] for h in graph.history]  # a replayed graph == eager
    for pa, pb in zip(runs[0].get_params(), graph.get_params()):
        assert np.array_equal(pa, pb)
    assert runs[0].l_out.order == order and runs[0].l_out.gather_dtype == "bfloat16"
    assert ref[-1] < ref[0] and got[-1] < got[0]  # it trains
    err = np.abs(np.array(got) - ref).max() / max(1.0, np.abs(ref).max())
    print(f"bf16-gather trainer ({order}): max loss error {err:.3e}, bar {TRAJECTORY_BAR:.3e}")
    assert err <= TRAJECTORY_BAR, (got, ref)
    plain = MLPCONV(**{**kw, "gather_dtype": "float32"}).fit(X, train, dev, test, Y, H)
    assert got != [h["train_loss"] for h in plain.history]  # the option changes the operands


def test_trainer_bf16_gather_with_dropout(cuda):
    """drop_out=True with the bf16 gather: the masks apply to the float32 outputs as before; the
    run is deterministic, finite, and not the float32-gather run."""
    H, X, Y, train, dev, test, init = problem(n=2000, e=12000, f=150, k=16, c=5)
    kw = dict(n_epochs=6, hidden_layer_size=16, regul_coefs=COEFS, init_parameters=init,
              device=cuda, seed=1, drop_out=True, dropout_coefs=(0.5, 0.25))
    runs = [MLPCONV(gather_dtype="bfloat16", **kw).fit(X, train, dev, test, Y, H)
            for _ in range(2)]
    got = [h["train_loss"] for h in runs[0].history]
    assert got == [h["train_loss"] for h in runs[1].history] and np.all(np.isfinite(got))
    plain = [h["train_loss"] for h in MLPCONV(**kw).fit(X, train, dev, test, Y, H).history]
    assert got != plain and np.abs(np.array(got) - np.array(plain)).max() < 1e-2


def test_gather_dtype_validation(cuda, monkeypatch):
    H, _X, _Y, _tr, _dev, _te, _init = problem(n=500, e=2000, f=50, k=8, c=3)
    with pytest.raises(ValueError):
        MLPCONV(hidden_layer_size=8, gather_dtype="float16")
    with pytest.raises(ValueError):
        ConvolutionDenseLayer(8, H=H, num_units=3, device=cuda, gather_dtype="bf16")
    A = gs.DeviceCSR.from_scipy(H, cuda)
    Z = torch.randn(500, 8, device=cuda)
    with pytest.raises(ValueError):
        csr_matmul(A, Z, gather_dtype="half")

    with monkeypatch.context() as m:
        m.setattr(torch.compiler, "is_compiling", lambda: True)
        with pytest.raises(NotImplementedError, match="torch.compile"):
            csr_matmul(A, Z, gather_dtype="bfloat16")
    # propagate() and the generic layer pass the option on
    layer = ConvolutionDenseLayer(8, H=A, num_units=3, device=cuda, mode="ordered",
                                  order="propagate_first", gather_dtype="bfloat16")
    with torch.no_grad():
        P = layer.propagate(Z).cpu().numpy()
    assert np.array_equal(P, O.spmm_f32(H, bf16r(Z.cpu().numpy())))
