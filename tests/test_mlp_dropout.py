"""CPU tests of the dropout MLP (graphconvgeo_amd.mlp.DropoutMLP; reference mlp.py:96-311 with
drop_out=True): the constructor, the argument checks of gcg_rectify_backward_wide_f32 by status
code (no launch), and the float64 restatement of the step under masks
(tests/mlp_dropout_reference.py) against mlp_reference and against central differences."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import mlp_dropout_reference as DR
import mlp_reference as R
from graphconvgeo_amd import mlp as M

OK, INVALID, MISALIGNED, WORKSPACE = 0, 1, 2, 6


# -- constructor ---------------------------------------------------------------------------------
def test_constructor_defaults_are_the_references():
    clf = M.DropoutMLP()
    assert (clf.n_epochs, clf.batch_size, clf.add_hidden, clf.regul_coefs) == \
        (10, 1000, True, [5e-5, 5e-5])
    assert clf.drop_out is True and clf.drop_out_coefs == [0.5, 0.5]
    assert clf.early_stopping_max_down == 100000 and clf.hidden_dropout is False
    assert clf.hidden_layer_size is None and clf.init_parameters is None
    assert clf.permutation_only  # a repeated row would share one slot of the dropped values
    assert M.DropoutMLP(hidden_dropout=True, drop_out_coefs=[0.3, 0.0]).hidden_dropout is True


@pytest.mark.parametrize("coefs", [[1.0, 0.5], [0.5, 1.0], [-0.1, 0.5], [0.5, 1.5], [0.5]])
def test_bad_coefficients_raise(coefs):
    with pytest.raises(ValueError):
        M.DropoutMLP(drop_out_coefs=coefs)


def test_options_that_are_not_built_raise():
    with pytest.raises(ValueError, match="add_hidden"):
        M.DropoutMLP(add_hidden=False)
    with pytest.raises(ValueError):
        M.DropoutMLP(drop_out=False)
    with pytest.raises(NotImplementedError):
        M.DropoutMLP(complete_prob=True)
    with pytest.raises(NotImplementedError):
        M.DropoutMLP(loss_name="hinge")
    with pytest.raises(NotImplementedError, match="DropoutMLP"):
        M.MLP(drop_out=True)


# -- the wide entry's argument checks --------------------------------------------------------------
A16, B16, W16, S16, G16 = (C.c_void_p(x) for x in (0x10000, 0x2000000, 0x4000000, 0x50000,
                                                   0x60000))
THR, SCALE, SEED = C.c_uint32(1 << 31), C.c_float(2.0), C.c_uint64(77)
DROP = (THR, SCALE, SEED, S16, 1, 0, None)       # a mask: step_dev given
NODROP = (THR, SCALE, SEED, None, 1, 0, None)    # step_dev NULL: no mask


def test_wide_backward_abi_without_gpu(native_lib):
    f = native_lib.gcg_rectify_backward_wide_f32
    nb = C.c_size_t()
    assert native_lib.gcg_relu_backward_f32_workspace_bytes(8, 2048, C.byref(nb)) == OK
    assert nb.value == 4 * 2048  # one row block: general in K
    ws = (W16, nb.value)
    assert f(8, 2048, None, 2048, G16, 2048, B16, 2048, None, *ws, *DROP) == INVALID   # null gY
    assert f(8, 2048, A16, 2048, G16, 2048, None, 2048, None, *ws, *DROP) == INVALID   # null g_out
    assert f(8, 2048, A16, 2047, G16, 2048, B16, 2048, None, *ws, *DROP) == INVALID    # ldg < K
    assert f(8, 2048, A16, 2048, G16, 2048, B16, 2044, None, *ws, *NODROP) == INVALID  # ldo < K
    assert f(-1, 2048, A16, 2048, G16, 2048, B16, 2048, None, *ws, *DROP) == INVALID
    assert f(8, -1, A16, 2048, G16, 2048, B16, 2048, None, *ws, *DROP) == INVALID
    assert f(8, 2048, A16, 2048, G16, 2048, B16, 2048, None, *ws, THR, SCALE, SEED, S16, 1, -1,
             None) == INVALID                                                         # row0 < 0
    # neither a gate nor a mask: column sums are gcg_column_sum_f32's
    assert f(8, 2048, A16, 2048, None, 0, B16, 2048, None, *ws, *NODROP) == INVALID
    assert f(0, 2048, None, 2048, None, 0, None, 2048, None, None, 0, *NODROP) == INVALID
    # the gate: ldgate >= K, ldgate % 4 == 0, a 4-B base -- with and without a mask
    for tail in (DROP, NODROP):
        assert f(8, 2048, A16, 2048, C.c_void_p(0x60001), 2048, B16, 2048, None, *ws, *tail) \
            == MISALIGNED
        assert f(8, 2048, A16, 2048, G16, 2047, B16, 2048, None, *ws, *tail) == MISALIGNED
        assert f(8, 1026, A16, 1028, G16, 1026, B16, 1028, None, *ws, *tail) == MISALIGNED
    # K > 256 needs 16-B rows
    assert f(8, 1028, A16, 1029, G16, 1028, B16, 1032, None, *ws, *DROP) == MISALIGNED
    assert f(8, 1028, A16, 1028, G16, 1028, B16, 1029, None, *ws, *NODROP) == MISALIGNED
    assert f(8, 1028, C.c_void_p(0x10004), 1028, G16, 1028, B16, 1028, None, *ws, *DROP) \
        == MISALIGNED
    assert f(8, 1028, C.c_void_p(0x10002), 1028, G16, 1028, B16, 1028, None, *ws, *DROP) \
        == MISALIGNED
    # the workspace: required, gcg_relu_backward_f32_workspace_bytes(M, K), not a byte less.
    # K = 1025 gets this far, so the sizes passed validation: no 1024-column cap here
    for K in (1025, 2048):
        ld = (K + 3) // 4 * 4
        assert native_lib.gcg_relu_backward_f32_workspace_bytes(1030, K, C.byref(nb)) == OK
        assert nb.value == 4 * 3 * K  # three row blocks of 512
        for tail, gate in ((DROP, G16), (DROP, None), (NODROP, G16)):
            args = (1030, K, A16, ld, gate, ld, B16, ld, None)
            assert f(*args, W16, nb.value - 1, *tail) == WORKSPACE
            assert f(*args, None, nb.value, *tail) == WORKSPACE
    # empty problems: no launch (M == 0 with a bias_grad zeroes it: the GPU tests)
    assert f(0, 2048, None, 2048, G16, 2048, None, 2048, None, None, 0, *NODROP) == OK
    assert f(0, 2048, None, 2048, None, 0, None, 2048, None, None, 0, *DROP) == OK
    assert f(8, 0, None, 0, G16, 0, None, 0, None, None, 0, *NODROP) == OK


# -- the float64 restatement -----------------------------------------------------------------------
def small_problem(n=90, f=40, k=7, c=4, seed=0):
    rng = np.random.default_rng(seed)
    X = sps.random(n, f, density=0.25, format="csr", dtype=np.float64, random_state=seed)
    Y = rng.integers(0, c, size=n)
    init = (rng.normal(0, 0.3, (f, k)), rng.normal(0, 0.1, k), rng.normal(0, 0.3, (k, c)),
            rng.normal(0, 0.1, c))
    return X, Y, init


def test_all_ones_masks_restate_mlp_reference():
    """One step and then two epochs with all-ones (and with no) masks: mlp_reference.mlp_train's
    figures and parameters to 1e-12."""
    X, Y, init = small_problem()
    coefs = (1e-3, 2e-3)
    rng = np.random.default_rng(1)
    for orders, B in (([np.arange(60)], 60), ([rng.permutation(60), rng.permutation(60)], 25)):
        want_h, want_p = R.mlp_train(X[:60], Y[:60], X[60:], Y[60:], init, orders, B, coefs)
        for ones in (True, False):
            m_in = (lambda step, rows: np.ones((B, 40))) if ones else None
            m_hid = (lambda step: np.ones((B, 7))) if ones else None
            got_h, got_p = DR.mlp_dropout_train(X[:60], Y[:60], X[60:], Y[60:], init, orders, B,
                                                coefs, m_in, m_hid)
            for a, b in zip(got_h, want_h):
                assert a["epoch"] == b["epoch"] and a["train_acc"] == b["train_acc"]
                for key in ("train_loss", "val_loss", "val_acc"):
                    assert abs(a[key] - b[key]) <= 1e-12, key
            for k in want_p:
                assert np.abs(got_p[k] - want_p[k]).max() <= 1e-12, k


def test_gradient_matches_central_differences_under_masks():
    """Every entry of b1, b2 and W2 and 40 random entries of W1: the analytic gradient under an
    input mask (p = 0.4, scale 1 / 0.6) and a hidden mask (p = 0.5, scale 2) against
    (L(x + e) - L(x - e)) / 2e, e = 1e-6, in float64. The loss is piecewise smooth with third
    derivatives of order 1 here, so the difference quotient is off by ~e^2 = 1e-12 plus
    rounding ~1e-16 / e = 1e-10: the bound is 1e-8 * max(1, |g|). No pre-activation lies
    within e of the rectifier's kink (asserted)."""
    X, Y, init = small_problem(seed=3)
    coefs = (1e-3, 2e-3)
    rng = np.random.default_rng(5)
    B = 50
    Xb, y = X[:B], Y[:B]
    m_in = (rng.random((B, 40)) >= 0.4) / 0.6
    m_hid = (rng.random((B, 7)) >= 0.5) * 2.0
    assert 0.2 < (m_in == 0).mean() < 0.6 and 0.3 < (m_hid == 0).mean() < 0.7
    params = {k: np.array(v, dtype=np.float64) for k, v in zip(("W1", "b1", "W2", "b2"), init)}
    pre1 = sps.csr_matrix(Xb.multiply(m_in)) @ params["W1"] + params["b1"]
    assert np.abs(pre1).min() > 1e-4
    _, _, g = DR.dropout_step(Xb, y, params, coefs, m_in, m_hid)
    e = 1e-6
    for name in ("W1", "b1", "W2", "b2"):
        p = params[name]
        flat = np.arange(p.size) if p.size <= 40 else rng.choice(p.size, 40, replace=False)
        for i in flat:
            idx = np.unravel_index(i, p.shape)
            old = p[idx]
            p[idx] = old + e
            up = DR.dropout_step(Xb, y, params, coefs, m_in, m_hid)[0]
            p[idx] = old - e
            down = DR.dropout_step(Xb, y, params, coefs, m_in, m_hid)[0]
            p[idx] = old
            num = (up - down) / (2 * e)
            assert abs(num - g[name][idx]) <= 1e-8 * max(1.0, abs(num)), (name, idx)
    # and the masks matter: without them the gradient is another one
    _, _, g0 = DR.dropout_step(Xb, y, params, coefs)
    assert np.abs(g0["W1"] - g["W1"]).max() > 1e-3
