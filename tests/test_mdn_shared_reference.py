"""CPU tests of the shared-component mixture-density model (graphconvgeo_amd.mdn; reference
lang2loc_mdnshared.py): the torch restatement the GPU tests are judged by
(tests/mdn_shared_reference.py) against scipy's bivariate normal, cluster_params against a NumPy
restatement of get_cluster_centers, the exported symbols and the host-side argument validation
of the new C calls, and the constructor of NNModel_lang2locshared. No GPU compute here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy.special import logsumexp
from scipy.stats import multivariate_normal

import mdn_shared_reference as S
from mdn_reference import softplus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("gcg_mdn_shared_nll_f32_workspace_bytes", "gcg_mdn_shared_nll_f32",
             "gcg_mdn_shared_density_f32", "gcg_mdn_shared_predict_f32")


def draw(B, C_, regime="tight"):
    return tuple(torch.tensor(a, dtype=torch.float64) for a in S.sweep_inputs(B, C_, regime))


def cov_of(sigmas, corxy, k):
    s1, s2, rho = sigmas[k, 0], sigmas[k, 1], corxy[k]
    return [[s1 * s1, rho * s1 * s2], [rho * s1 * s2, s2 * s2]]


# -- the restatement ---------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["wide", "tight"])
def test_single_component_is_the_bivariate_normal_density(regime):
    L, Y, mus, sig, cor = draw(9, 1, regime)
    sigmas, corxy = (t.numpy() for t in S.transforms(sig, cor))
    got = S.nll_rows(L, Y, mus, sig, cor).numpy()
    dist = multivariate_normal(mean=mus[0].numpy(), cov=cov_of(sigmas, corxy, 0))
    for r in range(9):
        want = -dist.logpdf(Y[r].numpy())
        assert abs(got[r] - want) <= 1e-10 * max(1.0, abs(want)), (r, got[r], want)


def test_loss_is_the_mixture_log_density():
    L, Y, mus, sig, cor = draw(5, 4)
    sigmas, corxy = (t.numpy() for t in S.transforms(sig, cor))
    pis = torch.softmax(L, dim=1).numpy()
    got = S.nll_rows(L, Y, mus, sig, cor).numpy()
    for r in range(5):
        terms = [np.log(pis[r, k]) + multivariate_normal(
            mean=mus[k].numpy(), cov=cov_of(sigmas, corxy, k)).logpdf(Y[r].numpy())
            for k in range(4)]
        want = -logsumexp(terms)
        assert np.isfinite(want) and abs(got[r] - want) <= 1e-9 * max(1.0, abs(want))


def test_prediction_scores_are_the_mixture_density_at_the_means():
    C_ = 4
    L, _, mus, sig, cor = draw(3, C_, "wide")
    sigmas, corxy = (t.numpy() for t in S.transforms(sig, cor))
    pis = torch.softmax(L, dim=1).numpy()
    got = S.pred_scores(L, mus, sig, cor).numpy()
    table = S.density(mus, sig, cor).numpy()
    for i in range(C_):
        for j in range(C_):
            want = multivariate_normal(mean=mus[j].numpy(), cov=cov_of(sigmas, corxy, j)).pdf(mus[i].numpy())
            assert abs(table[i, j] - want) <= 1e-10 * want
    for r in range(3):
        for i in range(C_):
            want = sum(pis[r, j] * table[i, j] for j in range(C_))
            assert abs(got[r, i] - want) <= 1e-12 * want
    idx, sel = S.pred(L, mus, sig, cor, "pi")
    assert np.array_equal(idx.numpy(), pis.argmax(axis=1))
    assert np.array_equal(sel.numpy(), mus.numpy()[pis.argmax(axis=1)])
    idx, sel = S.pred(L, mus, sig, cor)
    assert np.array_equal(idx.numpy(), got.argmax(axis=1)) and torch.equal(sel, mus[idx])


def test_loss_is_invariant_under_a_permutation_of_the_components():
    L, Y, mus, sig, cor = draw(11, 6)
    perm = torch.tensor([3, 0, 5, 1, 4, 2])
    a = S.nll_rows(L, Y, mus, sig, cor).numpy()
    b = S.nll_rows(L[:, perm], Y, mus[perm], sig[perm], cor[perm]).numpy()
    assert np.allclose(a, b, rtol=1e-13, atol=0)


def test_float32_trainer_follows_the_float64_trainer():
    """The yardstick the GPU trainer test uses exists and is close: two Adam steps."""
    import scipy.sparse as sps
    rng = np.random.default_rng(0)
    X = sps.random(8, 5, density=0.6, format="csr", dtype=np.float32, random_state=1)
    Y = rng.normal(0, 3, (8, 2)).astype(np.float32)
    init = [rng.normal(0, 0.3, s).astype(np.float32) for s in ((5, 4), (4,), (4, 3), (3,))] + \
        [rng.normal(0, 3, (3, 2)).astype(np.float32), np.full((3, 2), 2.0, np.float32),
         np.zeros(3, np.float32)]
    orders = [np.arange(8)]
    h64, p64 = S.shared_train(X, Y, X, Y, init, orders, 4, 1e-4)
    h32, p32 = S.shared_train(X, Y, X, Y, init, orders, 4, 1e-4, dtype=torch.float32)
    assert abs(h64[0]["train_loss"] - h32[0]["train_loss"]) < 1e-5 * abs(h64[0]["train_loss"])
    for k in S.NAMES:
        assert p32[k].dtype == np.float32 and p64[k].dtype == np.float64
        assert np.allclose(p32[k], p64[k], rtol=1e-4, atol=1e-5), k
        assert not np.array_equal(p64[k], np.asarray(init[S.NAMES.index(k)], np.float64)), k


# -- cluster_params ----------------------------------------------------------------------------
def clustered_points():
    rng = np.random.default_rng(4)
    pts = [rng.multivariate_normal([40, -74], [[2.0, 0.8], [0.8, 1.0]], size=30),
           np.array([[-33.9, 151.2]]),                       # a single member
           np.tile([[51.5, -0.1]], (4, 1)),                   # identical points
           rng.multivariate_normal([10, 20], [[0.5, -0.3], [-0.3, 3.0]], size=12)]
    labels = np.concatenate([np.full(len(p), i) for i, p in enumerate(pts)])
    latlon = np.vstack(pts)
    order = rng.permutation(len(labels))
    return latlon[order], labels[order]


@pytest.mark.parametrize("raw", [False, True])
def test_cluster_params_match_the_numpy_restatement(raw):
    from graphconvgeo_amd.mdn import cluster_params
    latlon, labels = clustered_points()
    got = cluster_params(latlon, labels, 4, raw=raw)
    want = S.cluster_params_numpy(latlon, labels, 4, raw=raw)
    for g, w, shape in zip(got, want, ((4, 2), (4, 2), (4,))):
        assert g.shape == shape and g.dtype == np.float32
        assert np.allclose(g, w, rtol=1e-6, atol=1e-6)
    if not raw:  # the fallback of the single member and of the identical points
        assert np.array_equal(got[1][1:3], np.ones((2, 2))) and not got[2][1:3].any()
        assert np.allclose(got[0][2], [51.5, -0.1], atol=1e-5)
        for i in (0, 3):  # the full clusters: numpy's own correlation and ddof = 1 deviations
            pts = latlon[labels == i]
            assert abs(got[2][i] - np.corrcoef(pts, rowvar=False)[0, 1]) < 1e-6
            assert np.allclose(got[1][i], pts.std(axis=0, ddof=1), rtol=1e-6)


def test_raw_inverses_round_trip():
    from graphconvgeo_amd.mdn import cluster_params
    latlon, labels = clustered_points()
    _, s, c = cluster_params(latlon, labels, 4, raw=False)
    _, s_raw, c_raw = cluster_params(latlon, labels, 4, raw=True)
    back_s, back_c = S.transforms(torch.tensor(s_raw, dtype=torch.float64),
                                  torch.tensor(c_raw, dtype=torch.float64))
    assert np.abs(back_s.numpy() - s).max() <= 1e-6
    assert np.abs(back_c.numpy() - c).max() <= 1e-6
    assert np.allclose(softplus(torch.tensor([0.5413248546129181], dtype=torch.float64)), 1.0)
    with pytest.raises(ValueError, match="no member"):
        cluster_params(latlon, labels, 5)


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


def test_shared_calls_validate_on_the_host(native_lib):
    lib = native_lib
    l, y, m, s, c, g, o, w = (C.c_void_p(0x10000 * (i + 1)) for i in range(8))
    INVALID, MISALIGNED, WORKSPACE, OK = 1, 2, 6, 0
    size = C.c_size_t()
    ws_bytes = lib.gcg_mdn_shared_nll_f32_workspace_bytes
    assert ws_bytes(4, 0, C.byref(size)) == INVALID
    assert ws_bytes(4, 1025, C.byref(size)) == INVALID
    assert ws_bytes(4, 3, None) == INVALID
    assert ws_bytes(4, 3, C.byref(size)) == OK
    assert size.value == 4 * ((10 + 5) * 3 + 4)      # constants, one workgroup's partial, rows
    assert ws_bytes(1000, 100, C.byref(size)) == OK
    assert size.value == 4 * ((10 + 5 * 250) * 100 + 1000)   # 4 rows per workgroup
    assert ws_bytes(5000, 100, C.byref(size)) == OK
    assert size.value == 4 * ((10 + 5 * 417) * 100 + 5000)   # 12 rows per workgroup
    assert ws_bytes(4, 3, C.byref(size)) == OK
    n = size.value

    nll = lib.gcg_mdn_shared_nll_f32

    def call(B=4, C_=3, L=l, ldl=3, Y=y, mus=m, sig=s, cor=c, dL=g, lddl=3, dp=o, rows=o,
             loss=o, ws=w, wsb=n):
        return nll(B, C_, L, ldl, Y, mus, sig, cor, None, dL, lddl, dp, rows, loss, ws, wsb, None)

    assert call(C_=0) == INVALID and call(C_=1025, ldl=1025, lddl=1025) == INVALID
    assert call(B=-1) == INVALID
    assert call(ldl=2) == INVALID and call(lddl=2) == INVALID
    for null in ("L", "Y", "mus", "sig", "cor", "loss"):
        assert call(**{null: None}) == INVALID, null
    assert "gcg_mdn_shared_nll_f32" in lib.gcg_last_error().decode()
    assert call(mus=C.c_void_p(0x30002)) == MISALIGNED
    assert call(ws=None) == WORKSPACE and call(wsb=n - 1) == WORKSPACE
    assert call(B=0, L=None, Y=None, loss=None, ws=None, wsb=0) == OK  # empty

    dens = lib.gcg_mdn_shared_density_f32
    assert dens(0, m, s, c, g, None) == INVALID and dens(1025, m, s, c, g, None) == INVALID
    assert dens(3, None, s, c, g, None) == INVALID and dens(3, m, s, c, None, None) == INVALID

    pred = lib.gcg_mdn_shared_predict_f32
    assert pred(4, 0, l, 3, g, m, 0, None, o, None) == INVALID
    assert pred(4, 1025, l, 1025, g, m, 0, None, o, None) == INVALID
    assert pred(4, 3, l, 2, g, m, 0, None, o, None) == INVALID          # ldl < C
    assert pred(4, 3, l, 3, g, m, 2, None, o, None) == INVALID          # method
    assert pred(4, 3, None, 3, g, m, 0, None, o, None) == INVALID
    assert pred(4, 3, l, 3, None, m, 0, None, o, None) == INVALID       # mixture needs Dt
    assert pred(4, 3, l, 3, g, None, 0, None, o, None) == INVALID
    assert pred(4, 3, l, 3, g, m, 0, None, None, None) == INVALID       # null latlon
    assert "gcg_mdn_shared_predict_f32" in lib.gcg_last_error().decode()
    assert pred(0, 3, None, 3, None, None, 1, None, None, None) == OK


# -- the constructor ---------------------------------------------------------------------------
def test_constructor_defaults_refusals_and_export():
    import graphconvgeo_amd
    from graphconvgeo_amd.mdn import NNModel_lang2loc, NNModel_lang2locshared, _MdnTrainer
    assert graphconvgeo_amd.NNModel_lang2locshared is NNModel_lang2locshared
    assert "NNModel_lang2locshared" in graphconvgeo_amd.__all__
    assert issubclass(NNModel_lang2loc, _MdnTrainer) and issubclass(NNModel_lang2locshared, _MdnTrainer)
    m = NNModel_lang2locshared(device="cpu")
    assert (m.n_epochs, m.batch_size, m.regul_coef, m.hid_size) == (10, 1000, 1e-6, 100)
    assert (m.drop_out, m.dropout_coef, m.early_stopping_max_down) == (False, 0.5, 10)
    assert (m.dtype, m.autoencoder, m.n_bigaus_comp, m.sqerror, m.nan) == ("float32", 100, 100, False, False)
    assert m.mus_init is None and m.sigmas_init is None and m.corxy_init is None
    # the reference driver's keyword call
    mus = np.zeros((300, 2), np.float32)
    m = NNModel_lang2locshared(n_epochs=10000, batch_size=200, regul_coef=1e-6, input_size=50,
                               output_size=2, hid_size=200, drop_out=True, dropout_coef=0.5,
                               early_stopping_max_down=5, input_sparse=True, reload=False,
                               ncomp=300, autoencoder=False, sqerror=False, mus=mus,
                               sigmas=np.ones((300, 2), np.float32),
                               corxy=np.zeros(300, np.float32), dataset_name="cmu", device="cpu")
    assert m._drops and m.n_bigaus_comp == 300 and m.mus_init is mus
    with pytest.raises(NotImplementedError, match="sqerror"):
        NNModel_lang2locshared(sqerror=True, device="cpu")
    with pytest.raises(NotImplementedError, match="reload"):
        NNModel_lang2locshared(reload=True, device="cpu")
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="ncomp"):
            NNModel_lang2locshared(ncomp=bad, device="cpu")
    with pytest.raises(ValueError, match="mus must have shape"):
        NNModel_lang2locshared(ncomp=4, mus=np.zeros((3, 2)), device="cpu")
    with pytest.raises(ValueError, match="corxy must have shape"):
        NNModel_lang2locshared(ncomp=4, corxy=np.zeros((4, 1)), device="cpu")
    with pytest.raises(ValueError, match="must be sparse"):
        NNModel_lang2locshared(device="cpu").fit(np.zeros((4, 3)), np.zeros((4, 2)),
                                                 np.zeros((4, 3)), np.zeros((4, 2)))
