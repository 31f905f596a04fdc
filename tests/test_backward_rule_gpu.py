"""The backward of act(A . Z + b)[rows] is one rule, whoever states it: the eager layer
(layers.csr_matmul), the registered op (ops.spmm_csr, called directly) and the partitioned
trainer's GPUOps.relu_backward give the same bits, and all of them Theano's gradient in float64:

    g  = gY * 0.5 * (1 + sgn(pre))   with rectify (g / 2 at a pre-activation of exactly 0)
    db = colsum(g)        dZ = (A[rows])^T . g   (repeated rows add)

A, Z and b hold short binary fractions, so the pre-activations are exact in float32 and their
signs are the float64 reference's. Row 0 of A is empty: with b = 0 (or no b) its pre-activation
is exactly 0. K = 5 takes the scalar path of the one-pass kernel (K % 4 != 0), K = 300 the
dwordx4 path, K = 1028 is past its 1024 columns."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

from graphconvgeo_amd import layers, ops
from graphconvgeo_amd import sparse as gs
from graphconvgeo_amd.dist_train import GPUOps

pytestmark = pytest.mark.gpu

N = 96


@functools.lru_cache(maxsize=None)
def graph():
    """Seeded non-symmetric 96 x 96 CSR, about 5 nonzeros per row, row 0 empty."""
    rng = np.random.default_rng(11)
    rows = np.repeat(np.arange(1, N), 5)
    cols = rng.integers(0, N, size=rows.size)
    vals = rng.integers(1, 9, size=rows.size) * rng.choice([-0.25, 0.25], size=rows.size)
    A = sps.csr_matrix((vals.astype(np.float32), (rows, cols)), shape=(N, N))
    A.sum_duplicates()
    assert A.indptr[1] == 0 and (abs(A - A.T) > 0).nnz > 0
    return A


@functools.lru_cache(maxsize=None)
def operands(K):
    rng = np.random.default_rng(100 + K)
    Z = (rng.integers(-8, 9, size=(N, K)) / 8.0).astype(np.float32)
    targets = rng.integers(0, N, size=40).astype(np.int32)  # drawn with replacement
    targets[:3] = (0, 0, 5)  # the empty row, twice
    assert np.unique(targets).size < targets.size
    gY = {n: rng.standard_normal((n, K)).astype(np.float32) for n in (N, 40)}
    return Z, targets, gY


def theano_rule(A, Z, b, act, targets, gY):
    """float64 (g, db, dZ)."""
    S = A.astype(np.float64) if targets is None else A.astype(np.float64)[targets]
    pre = S @ Z.astype(np.float64) + (0.0 if b is None else b.astype(np.float64))
    g = gY.astype(np.float64)
    if act is not None:
        g = g * 0.5 * (1.0 + np.sign(pre))
    return g, g.sum(axis=0), S.T @ g


def within(got, ref):
    return np.abs(got.cpu().numpy() - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("use_rows", [False, True], ids=["all_rows", "targets"])
@pytest.mark.parametrize("use_bias", [False, True], ids=["no_bias", "zero_bias"])
@pytest.mark.parametrize("act", [None, "relu"], ids=["linear", "rectify"])
@pytest.mark.parametrize("K", [5, 300, 1028])
def test_one_backward_rule(cuda, K, act, use_bias, use_rows):
    A_host = graph()
    Z_host, targets, gYs = operands(K)
    A = gs.DeviceCSR.from_scipy(A_host, cuda)
    rows = gs.RowSelection(targets, cuda) if use_rows else None
    gY_host = gYs[40 if use_rows else N]
    gY = torch.from_numpy(gY_host).to(cuda)
    b_host = np.zeros(K, np.float32) if use_bias else None
    g_ref, db_ref, dZ_ref = theano_rule(A_host, Z_host, b_host, act,
                                        targets if use_rows else None, gY_host)
    if act is not None:  # the g / 2 rule is exercised: row 0's pre-activation is exactly 0
        assert np.array_equal(g_ref[0], 0.5 * gY_host[0].astype(np.float64))

    def run(product):
        Z = torch.from_numpy(Z_host).to(cuda).requires_grad_()
        b = torch.zeros(K, device=cuda).requires_grad_() if use_bias else None
        product(A, Z, b, act, rows).backward(gY)
        return Z.grad, (None if b is None else b.grad)

    dZ_eager, db_eager = run(layers.csr_matmul)
    dZ_op, db_op = run(ops.spmm_csr)
    assert torch.equal(dZ_eager, dZ_op)
    assert within(dZ_eager, dZ_ref)
    if use_bias:
        assert torch.equal(db_eager, db_op)
        assert within(db_eager, db_ref)

    if act is not None and K <= 1024:
        # the partitioned trainer's statement, on the gate bytes of the same forward
        n_out = 40 if use_rows else N
        gate = gs.empty_gate(n_out, K, cuda)
        Z = torch.from_numpy(Z_host).to(cuda)
        gs.spmm(A, Z, bias=torch.zeros(K, device=cuda) if use_bias else None, act="relu",
                rows=rows, gate=gate)
        g, db = GPUOps.relu_backward(gY, gate, bias_grad=True)
        assert np.array_equal(g.cpu().numpy(), g_ref.astype(np.float32))  # g, g / 2, 0: exact
        if use_bias:
            assert torch.equal(db, db_eager)
        dZ = gs.spmm(A.rows_transpose(rows), g) if use_rows else A.tmatmul(g)
        assert torch.equal(dZ, dZ_eager)
