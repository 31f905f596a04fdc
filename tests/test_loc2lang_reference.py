"""CPU checks of the location-to-language restatement (tests/loc2lang_reference.py) against
scipy -- Theano and Lasagne are not importable, so the restatement is judged by what is -- and of
what graphconvgeo_amd.loc2lang does on the host: the ABI entries' declarations and argument
validation, and the wrapper's ValueErrors, none of which needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sps
import torch
from scipy import stats

import loc2lang_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gcg_bigaus_layer_f32", "gcg_bigaus_layer_backward_f32_workspace_bytes",
           "gcg_bigaus_layer_backward_f32", "gcg_softmax_xent_csr_f32", "gcg_adamax_step_f32")


# -- the restatement against scipy ---------------------------------------------------------------
@pytest.mark.parametrize("regime", ["wide", "tight"])
def test_density_matches_scipy_multivariate_normal(regime):
    X, mus, sig, cor, _ = R.layer_inputs(7, 5, regime)
    got = R.bigaus(*(torch.tensor(a, dtype=torch.float64) for a in (X, mus, sig, cor))).numpy()
    s = np.logaddexp(sig.astype(np.float64), 0.0)
    rho = cor.astype(np.float64) / (1 + np.abs(cor.astype(np.float64)))
    for c in range(5):
        off = rho[c] * s[c, 0] * s[c, 1]
        cov = np.array([[s[c, 0] ** 2, off], [off, s[c, 1] ** 2]])
        want = stats.multivariate_normal.pdf(X.astype(np.float64), mean=mus[c].astype(np.float64),
                                             cov=cov)
        assert np.allclose(got[:, c], want, rtol=1e-9, atol=1e-300), (regime, c)
    assert got.max() > 0


def test_soft_cross_entropy_is_minus_sum_y_log_softmax():
    Z, Y, rows = R.xent_inputs(9, 37, 3.0)
    Yd = np.asarray(Y[rows].todense(), dtype=np.float64)
    got = R.soft_xent_rows(torch.tensor(Z, dtype=torch.float64), torch.tensor(Yd)).numpy()
    z = Z.astype(np.float64)
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    want = -(Yd * np.log(p)).sum(axis=1)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert (got[Yd.sum(axis=1) == 0] == 0).all() and (Yd.sum(axis=1) == 0).any()
    # the gradient of the sum of the rows: T softmax - y
    _, g = R.soft_xent_and_grad(Z, Yd, torch.float64)
    assert np.allclose(g, Yd.sum(axis=1, keepdims=True) * p - Yd, rtol=1e-10, atol=1e-12)


def test_adamax_first_step_is_lr_sign():
    p = {"w": np.array([1.0, -2.0, 3.0])}
    g = {"w": np.array([0.5, -1e-3, 7.0])}
    out = R.adamax_step(p, g, {})
    assert np.allclose(out["w"], p["w"] - R.LR * np.sign(g["w"]), rtol=1e-6)


def test_local_words_against_scipy_entropy():
    from graphconvgeo_amd import loc2lang as L
    rng = np.random.default_rng(4)
    preds = rng.random((30, 12))
    preds[:, 3] = 0.0
    preds[5, 3] = 1.0       # one place only: entropy 0, the most local word
    preds[:, 7] = 0.25      # uniform: the highest entropy
    norm = preds / np.abs(preds).sum(axis=0)
    ent = stats.entropy(norm)
    want = np.argsort(ent, kind="stable")
    assert want[0] == 3 and want[-1] == 7
    for k in (1, 5, 12):
        assert np.array_equal(L.local_words(preds, k), want[:k])
        assert np.array_equal(R.local_words(preds, k), want[:k])
    assert np.array_equal(L.local_words(torch.tensor(preds, dtype=torch.float32), 4),
                          np.argsort(stats.entropy(norm.astype(np.float32)), kind="stable")[:4])


# -- float32 against float64: what Adamax allows ---------------------------------------------------
@pytest.mark.parametrize("hid", [8, 0])
@pytest.mark.parametrize("tight", [True, False])
def test_float32_and_float64_trainers_agree(hid, tight):
    """At step 1 Adamax moves a parameter by lr * sign(g): a gradient that float32 rounds across
    zero would move it by 2 lr. On the parity problem (n = 96, B = 32, C = 5, V = 37, 0-5 words
    per row, 8 epochs = 24 steps) no parameter does."""
    Xtr, Ytr, Xdev, Ydev, init, orders, B = R.parity_problem(hid=hid, tight=tight)
    h64, p64 = R.train(Xtr, Ytr, Xdev, Ydev, init, orders, B)
    h32, p32 = R.train(Xtr, Ytr, Xdev, Ydev, init, orders, B, dtype=torch.float32)
    assert len(h64) == 8 and len(h64[0]["batch_losses"]) == 3
    assert h64[-1]["train_loss"] < h64[0]["train_loss"]
    for a, b in zip(h64, h32):
        assert abs(a["val_loss"] - b["val_loss"]) <= 1e-5 * max(1.0, abs(a["val_loss"]))
    for k in R.names(hid):
        dev = np.abs(p32[k] - p64[k]).max()
        print(k, "float32 against float64:", dev)
        assert np.allclose(p32[k], p64[k], rtol=1e-4, atol=1e-5), (k, dev)


# -- the ABI ---------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_built():
    from graphconvgeo_amd import _build, _native
    header = open(os.path.join(ROOT, "include", "gcg_spmm.h")).read()
    for name in ENTRIES:
        assert name + "(" in header and name in _native.SIGNATURES
    assert any(os.path.basename(s) == "softmax_csr.hip" for s in _build.SOURCES)
    import graphconvgeo_amd
    assert graphconvgeo_amd.NNModel_loc2lang is graphconvgeo_amd.loc2lang.NNModel_loc2lang


def test_abi_argument_validation_without_gpu(native_lib):
    lib = native_lib
    a, b, c, d, e = (C.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))
    odd = C.c_void_p(0x10002)
    fwd = lib.gcg_bigaus_layer_f32
    assert fwd(4, 0, a, b, c, d, e, 4, None) == 1            # C < 1
    assert fwd(4, 1025, a, b, c, d, e, 1028, None) == 1      # C > 1024
    assert b"1 <= C <= 1024" in lib.gcg_last_error()
    assert fwd(-1, 3, a, b, c, d, e, 3, None) == 1
    assert fwd(4, 3, a, b, c, d, e, 2, None) == 1            # ldg < C
    assert fwd(4, 3, None, b, c, d, e, 3, None) == 1
    assert fwd(4, 3, a, b, c, d, odd, 3, None) == 2
    assert fwd(0, 3, None, None, None, None, None, 3, None) == 0   # B = 0: no launch
    nb = C.c_size_t(0)
    wsb = lib.gcg_bigaus_layer_backward_f32_workspace_bytes
    assert wsb(4, 0, C.byref(nb)) == 1 and wsb(4, 3, None) == 1
    assert wsb(1000, 100, C.byref(nb)) == 0
    # P [5, C] and 250 workgroups' [5, C] partials, doubles (R = 4 rows at B <= 2048)
    assert nb.value == 8 * 5 * 100 * (1 + 250)
    assert wsb(5000, 7, C.byref(nb)) == 0 and nb.value == 8 * 35 * (1 + 417)   # R = 12
    bwd = lib.gcg_bigaus_layer_backward_f32
    big = C.c_size_t(1 << 20)
    assert bwd(4, 3, a, b, c, d, e, 2, None, a, b, big, None) == 1       # lddg < C
    assert bwd(4, 3, a, b, c, d, None, 3, None, a, b, big, None) == 1    # no dG
    assert bwd(4, 3, a, b, c, d, e, 3, None, None, b, big, None) == 1    # no dparams
    assert bwd(4, 3, a, b, c, d, e, 3, None, a, b, C.c_size_t(8), None) == 6   # workspace
    assert bwd(4, 3, a, b, c, d, e, 3, None, a, None, big, None) == 6
    assert bwd(4, 3, a, b, c, d, e, 3, None, a, C.c_void_p(0x20004), big, None) == 2
    assert bwd(0, 3, None, None, None, None, None, 3, None, None, None, C.c_size_t(0), None) == 0
    xent = lib.gcg_softmax_xent_csr_f32
    one = C.c_float(1.0)
    assert xent(4, 0, a, 4, 4, b, c, d, None, one, None, e, 4, a, None) == 1          # N < 1
    assert xent(4, (1 << 24) + 1, a, 1 << 25, 4, b, c, d, None, one, None, None, 0, a, None) == 1
    assert b"2^24" in lib.gcg_last_error()
    assert xent(4, 8, a, 7, 4, b, c, d, None, one, None, e, 8, a, None) == 1          # ldl < N
    assert xent(4, 8, a, 8, 4, b, c, d, None, one, None, e, 7, a, None) == 1          # ldo < N
    assert xent(4, 8, None, 8, 4, b, c, d, None, one, None, e, 8, a, None) == 1
    assert xent(4, 8, a, 8, 4, b, None, d, None, one, None, e, 8, a, None) == 1       # no indices
    assert xent(4, 8, a, 8, 4, b, c, d, None, one, None, e, 8, None, None) == 1       # no loss_rows
    assert xent(4, 8, a, 8, 3, b, c, d, None, one, None, e, 8, a, None) == 1          # y_rows < M
    assert xent(4, 8, a, 8, 0, None, None, None, None, one, None, None, 0, None, None) == 1
    assert xent(4, 8, a, 8, 4, b, c, d, odd, one, None, e, 8, a, None) == 2
    assert xent(0, 8, None, 8, 0, None, None, None, None, one, None, None, 0, None, None) == 0
    amax = lib.gcg_adamax_step_f32
    f = (C.c_float(0.9), C.c_float(0.999), C.c_float(1e-8))
    assert amax(-1, a, b, c, d, e, *f, None) == 1
    assert amax(4, a, b, c, d, None, *f, None) == 1           # no step_dev
    assert amax(4, a, None, c, d, e, *f, None) == 1
    assert amax(0, None, None, None, None, None, *f, None) == 0


# -- the wrapper's checks, before any launch -------------------------------------------------------
def test_wrapper_refuses_bad_targets_and_rows_on_the_host():
    from graphconvgeo_amd import loc2lang as L
    good = sps.csr_matrix(np.array([[0, 0.5, 0.5], [0, 0, 0], [1.0, 0, 0]], np.float32))
    out = L.check_targets(good)
    assert out.dtype == np.float32 and out.indices.dtype == np.int32 and out.nnz == 3
    assert np.array_equal(L.check_targets(good.toarray()).toarray(), good.toarray())
    bad_col = sps.csr_matrix((np.ones(2, np.float32), np.array([0, 3], np.int32),
                              np.array([0, 1, 2], np.int32)), shape=(2, 3))
    with pytest.raises(ValueError, match="outside"):
        L.check_targets(bad_col)
    with pytest.raises(ValueError, match="outside"):
        L.target_csr(bad_col, "cuda")   # checked on the host, before the device is touched
    dup = sps.csr_matrix((np.ones(3, np.float32), np.array([1, 1, 2], np.int32),
                          np.array([0, 3], np.int32)), shape=(1, 3))
    assert not dup.has_canonical_format
    with pytest.raises(ValueError, match="twice"):
        L.check_targets(dup)
    with pytest.raises(ValueError, match="twice"):
        L.target_csr(dup, "cuda")
    unsorted = sps.csr_matrix((np.ones(2, np.float32), np.array([2, 0], np.int32),
                               np.array([0, 2], np.int32)), shape=(1, 3))
    assert L.check_targets(unsorted).nnz == 2   # order does not matter, only uniqueness
    assert np.array_equal(L.check_rows([2, 0, 2, 1], 3, 4), np.array([2, 0, 2, 1], np.int32))
    for rows in ([0, 3, 1, 1], [0, -1, 1, 1]):
        with pytest.raises(ValueError, match="outside"):
            L.check_rows(rows, 3, 4)
    with pytest.raises(ValueError, match="integer row ids"):
        L.check_rows([0, 1, 2], 3, 4)
    with pytest.raises(ValueError, match="integer row ids"):
        L.check_rows(np.zeros(4), 3, 4)


def test_model_refusals_need_no_gpu():
    from graphconvgeo_amd import loc2lang as L
    with pytest.raises(NotImplementedError, match="nomdn"):
        L.NNModel_loc2lang(nomdn=True)
    with pytest.raises(NotImplementedError, match="reload"):
        L.NNModel_loc2lang(reload=True)
    with pytest.raises(ValueError, match="float32"):
        L.NNModel_loc2lang(dtype="float64")
    with pytest.raises(NotImplementedError, match="grid"):
        L.NNModel_loc2lang(input_size=7000)
    with pytest.raises(ValueError, match="n_gaus_comp"):
        L.NNModel_loc2lang(n_gaus_comp=1025)
    with pytest.raises(ValueError, match="hid_size"):
        L.NNModel_loc2lang(hid_size=1025)
    with pytest.raises(ValueError, match="mus must have shape"):
        L.NNModel_loc2lang(n_gaus_comp=4, mus=np.zeros((3, 2)))
    clf = L.NNModel_loc2lang(n_gaus_comp=4, hid_size=0)   # no output_size: built by fit
    assert clf.params is None and clf.names == ["mus", "sigmas", "corxy", "Wo", "bo"]
    with pytest.raises(RuntimeError, match="no parameters"):
        clf.get_params()
