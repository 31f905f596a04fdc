"""CPU tests of the mixture-density location head (graphconvgeo_amd.mdn; reference lang2loc.py):
the torch restatement the GPU tests are judged by (tests/mdn_reference.py) against
hand-computable cases, the exported symbols, the host-side argument validation of the new C
calls, the constructor of NNModel_lang2loc, and the keep rule of the dropout segmentation
stated in NumPy. No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps
import torch
from scipy.stats import multivariate_normal

import mdn_reference as R
from graphconvgeo_amd import dropout as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("gcg_mdn_nll_f32", "gcg_mdn_unpack_f32", "gcg_mdn_predict_f32",
             "gcg_minibatch_segment_dropout")


def draw(B, C, scale=1.0, seed=77):
    gen = torch.Generator().manual_seed(seed)
    O = scale * torch.randn(B, 6 * C, generator=gen, dtype=torch.float64)
    Y = (torch.rand(B, 2, generator=gen, dtype=torch.float64) * 2 - 1) * \
        torch.tensor([60.0, 170.0], dtype=torch.float64)
    return O, Y


# -- the restatement ---------------------------------------------------------------------------
def test_single_component_is_the_bivariate_normal_density():
    O, Y = draw(9, 1)
    mus, sigmas, corxy, pis = (t.numpy() for t in R.unpack_params(O, 1))
    got = R.nll_rows(O, Y, 1).numpy()
    assert np.array_equal(pis, np.ones((9, 1)))
    for r in range(9):
        s1, s2, rho = sigmas[r, 0, 0], sigmas[r, 1, 0], corxy[r, 0]
        cov = [[s1 * s1, rho * s1 * s2], [rho * s1 * s2, s2 * s2]]
        want = -multivariate_normal(mean=mus[r, :, 0], cov=cov).logpdf(Y[r].numpy())
        assert abs(got[r] - want) <= 1e-10 * max(1.0, abs(want)), (r, got[r], want)


def test_transforms_and_ranges():
    O, _ = draw(5, 7, scale=3.0)
    mus, sigmas, corxy, pis = R.unpack_params(O, 7)
    assert mus.shape == (5, 2, 7) and sigmas.shape == (5, 2, 7)
    assert corxy.shape == pis.shape == (5, 7)
    assert mus[:, 0].abs().max() < 90 and mus[:, 1].abs().max() < 180
    assert sigmas.min() > 0 and corxy.abs().max() < 1
    assert np.allclose(pis.sum(dim=1).numpy(), 1.0, rtol=0, atol=1e-14)
    x = torch.tensor([-800.0, -3.0, 0.0, 3.0, 800.0], dtype=torch.float64)
    assert torch.isfinite(R.softplus(x)).all() and R.softplus(x)[-1] == 800.0
    mid = x[1:4]  # the stable form is the function itself where the naive one is finite
    assert np.allclose(R.softplus(mid).numpy(), np.log(1 + np.exp(mid.numpy())), rtol=1e-15)


def test_loss_is_invariant_under_a_permutation_of_the_components():
    C_ = 6
    O, Y = draw(11, C_)
    perm = torch.tensor([3, 0, 5, 1, 4, 2])
    Op = O.reshape(-1, 6, C_)[:, :, perm].reshape(-1, 6 * C_)
    a, b = R.nll_rows(O, Y, C_).numpy(), R.nll_rows(Op, Y, C_).numpy()
    assert np.allclose(a, b, rtol=1e-13, atol=0)
    ia, la = R.pred(O, C_)
    ib, lb = R.pred(Op, C_)
    assert np.array_equal(perm[ib].numpy(), ia.numpy()) and torch.equal(la, lb)


def test_prediction_scores_are_the_mixture_density_at_the_means():
    C_ = 4
    O, _ = draw(3, C_)
    mus, sigmas, corxy, pis = (t.numpy() for t in R.unpack_params(O, C_))
    got = R.pred_scores(O, C_).numpy()
    for r in range(3):
        for c in range(C_):
            want = 0.0
            for k in range(C_):
                s1, s2, rho = sigmas[r, 0, k], sigmas[r, 1, k], corxy[r, k]
                cov = [[s1 * s1, rho * s1 * s2], [rho * s1 * s2, s2 * s2]]
                want += pis[r, k] * multivariate_normal(mean=mus[r, :, k], cov=cov).pdf(mus[r, :, c])
            assert abs(got[r, c] - want) <= 1e-10 * want
    idx, sel = R.pred(O, C_, "pi")
    assert np.array_equal(idx.numpy(), pis.argmax(axis=1))
    assert np.array_equal(sel.numpy(), mus[np.arange(3), :, pis.argmax(axis=1)])


def test_fixed_order_mean_is_a_mean():
    rows = np.random.default_rng(0).normal(5, 2, size=1000).astype(np.float32)
    assert abs(float(R.fixed_order_mean(rows)) - rows.astype(np.float64).mean()) < 1e-5
    assert R.fixed_order_mean(np.array([3.5], np.float32)) == np.float32(3.5)


# -- the ABI -----------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported(native_lib):
    from graphconvgeo_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcg_spmm.h")).read(),
                  flags=re.S)
    declared = set(re.findall(r"\b(gcg_[a-z0-9_]+)\s*\(", text))
    nm = subprocess.run(["nm", "-D", "--defined-only", _native.lib_path()], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\bT (gcg_[a-z0-9_]+)$", nm, flags=re.M))
    for name in NEW_CALLS:
        assert name in declared and name in exported and name in _native.SIGNATURES, name


def test_mdn_calls_validate_on_the_host(native_lib):
    lib = native_lib
    o, y, g, l, w = (C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))
    INVALID, WORKSPACE, OK = 1, 6, 0
    nll = lib.gcg_mdn_nll_f32
    assert nll(4, 0, o, 6, y, None, g, 6, l, l, None, 0, None) == INVALID          # C = 0
    assert nll(4, 1025, o, 6150, y, None, g, 6150, l, l, None, 0, None) == INVALID  # C = 1025
    assert nll(4, 3, o, 17, y, None, g, 18, l, l, None, 0, None) == INVALID         # ldo < 6C
    assert nll(4, 3, o, 18, y, None, g, 17, l, l, None, 0, None) == INVALID         # ldd < 6C
    assert nll(-1, 3, o, 18, y, None, g, 18, l, l, None, 0, None) == INVALID
    assert nll(4, 3, None, 18, y, None, g, 18, l, l, None, 0, None) == INVALID      # null O
    assert nll(4, 3, o, 18, None, None, g, 18, l, l, None, 0, None) == INVALID      # null Y
    assert nll(4, 3, o, 18, y, None, g, 18, l, None, None, 0, None) == INVALID      # null loss
    assert "gcg_mdn_nll_f32" in lib.gcg_last_error().decode()
    # without loss_rows the row losses live in the workspace: B floats
    assert nll(4, 3, o, 18, y, None, g, 18, None, l, None, 0, None) == WORKSPACE
    assert nll(4, 3, o, 18, y, None, g, 18, None, l, w, 15, None) == WORKSPACE
    assert nll(0, 3, None, 18, None, None, None, 0, None, None, None, 0, None) == OK  # empty

    unpack = lib.gcg_mdn_unpack_f32
    assert unpack(4, 0, o, 6, g, g, g, g, None) == INVALID
    assert unpack(4, 1025, o, 6150, g, g, g, g, None) == INVALID
    assert unpack(4, 3, o, 17, g, g, g, g, None) == INVALID
    assert unpack(4, 3, o, 18, g, g, None, g, None) == INVALID
    assert unpack(0, 3, None, 18, None, None, None, None, None) == OK

    pred = lib.gcg_mdn_predict_f32
    assert pred(4, 0, o, 6, 0, None, g, None) == INVALID
    assert pred(4, 1025, o, 6150, 0, None, g, None) == INVALID
    assert pred(4, 3, o, 17, 0, None, g, None) == INVALID
    assert pred(4, 3, o, 18, 2, None, g, None) == INVALID                           # method
    assert pred(4, 3, None, 18, 0, None, g, None) == INVALID
    assert pred(4, 3, o, 18, 0, None, None, None) == INVALID                        # null latlon
    assert "gcg_mdn_predict_f32" in lib.gcg_last_error().decode()
    assert pred(0, 3, None, 18, 1, None, None, None) == OK


def test_segment_dropout_validates_on_the_host(native_lib):
    seg = native_lib.gcg_minibatch_segment_dropout
    p = [C.c_void_p(0x10000 * (i + 1)) for i in range(12)]
    ip, ix, va, pe, bs, sc, sp, ep, ev, vd, ws, st = p

    def call(n_sel=64, batch=32, nnz_sel=100, step=st, vals_drop=vd, indptr=ip, wsb=0):
        return seg(257, 97, indptr, ix, va, pe, n_sel, batch, nnz_sel, bs, sc, sp, ep, ev,
                   vals_drop, ws, wsb, 1 << 31, 2.0, 7, step, 0, None)

    assert call(n_sel=65) == 1          # n_sel % batch != 0
    assert call(batch=0) == 1
    assert call(step=None) == 1         # null step scalar
    assert call(vals_drop=None) == 1    # null vals_drop with entries selected
    assert call(indptr=None) == 1
    assert "gcg_minibatch_segment_dropout" in native_lib.gcg_last_error().decode()
    assert call() == 6                  # every argument in order: the workspace is too small


# -- the constructor ---------------------------------------------------------------------------
def test_constructor_defaults_and_refusals():
    from graphconvgeo_amd.mdn import NNModel_lang2loc
    m = NNModel_lang2loc(device="cpu")
    assert (m.n_epochs, m.batch_size, m.regul_coef, m.hid_size) == (10, 1000, 1e-6, 100)
    assert (m.drop_out, m.dropout_coef, m.early_stopping_max_down) == (False, 0.5, 10)
    assert (m.dtype, m.autoencoder, m.n_bigaus_comp, m.sqerror) == ("float32", 100, 100, False)
    assert m.input_size is None and m.output_size is None and m.dataset_name == ""
    # the reference's keyword call (lang2loc.py:589-592)
    m = NNModel_lang2loc(n_epochs=10000, batch_size=200, regul_coef=1e-6, input_size=50,
                         output_size=2, hid_size=200, drop_out=True, dropout_coef=0.5,
                         early_stopping_max_down=5, input_sparse=True, reload=False, ncomp=300,
                         autoencoder=False, sqerror=False, dataset_name="cmu", device="cpu")
    assert m._drops and m.n_bigaus_comp == 300 and m.sparse is True
    assert not NNModel_lang2loc(drop_out=True, dropout_coef=0, device="cpu")._drops
    with pytest.raises(NotImplementedError, match="sqerror"):
        NNModel_lang2loc(sqerror=True, device="cpu")
    with pytest.raises(NotImplementedError, match="reload"):
        NNModel_lang2loc(reload=True, device="cpu")
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="ncomp"):
            NNModel_lang2loc(ncomp=bad, device="cpu")
    with pytest.raises(ValueError, match="dropout_coef"):
        NNModel_lang2loc(drop_out=True, dropout_coef=1.0, device="cpu")
    with pytest.raises(ValueError, match="must be sparse"):
        NNModel_lang2loc(device="cpu").fit(np.zeros((4, 3)), np.zeros((4, 2)), np.zeros((4, 3)),
                                           np.zeros((4, 2)))


# -- the keep rule of the dropout segmentation ------------------------------------------------
def test_segmentation_keep_rule_in_numpy():
    """What gcg_minibatch_segment_dropout writes, stated with dropout.keep_mask_reference: an
    entry is masked as the element (row id in X, column) under step0 + its batch's index."""
    rng = np.random.default_rng(5)
    X = sps.random(40, 23, density=0.3, format="csr", dtype=np.float32, random_state=3)
    X.data[:] = rng.random(X.nnz).astype(np.float32) + 0.5
    order, B, p, seed, step0 = rng.permutation(40), 8, 0.4, 1234567, 5
    scale = np.float32(D.dropout_scale(p))
    kept = 0
    for b in range(5):
        rows = order[b * B:(b + 1) * B]
        Xb = R.masked_rows(X, rows, p, seed, step0 + b)
        assert np.array_equal(Xb.indptr, X[rows].indptr)
        assert np.array_equal(Xb.indices, X[rows].indices)
        for i, r in enumerate(rows):  # element by element, position in the batch irrelevant
            cols = X.indices[X.indptr[r]:X.indptr[r + 1]]
            keep = D.keep_mask_reference(np.full(cols.size, r), cols, p, seed, step0 + b, 0)
            v = X.data[X.indptr[r]:X.indptr[r + 1]]
            want = np.where(keep, v * scale, np.float32(0)).astype(np.float32)
            got = Xb.data[Xb.indptr[i]:Xb.indptr[i + 1]]
            assert np.array_equal(got.view(np.int32), want.view(np.int32))
            kept += int(keep.sum())
        # another step draws another mask for the same rows
        other = R.masked_rows(X, rows, p, seed, step0 + b + 1)
        assert not np.array_equal(other.data, Xb.data)
    assert 0.5 < kept / X.nnz < 0.7  # 1 - p = 0.6 of the 40 rows' entries
    same = R.masked_rows(X, order[:B], 0.0, seed, step0)
    assert np.array_equal(same.data.view(np.int32), X[order[:B]].data.view(np.int32))
