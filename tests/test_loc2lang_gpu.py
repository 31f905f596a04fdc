"""GPU tests of the location-to-language model (graphconvgeo_amd.loc2lang; the Gaussian-layer
kernels of csrc/mdn.hip, csrc/softmax_csr.hip, the Adamax kernel of csrc/csr_ops.hip; reference
loc2lang.py). The judge for numbers is tests/loc2lang_reference.py in float64; the bar for a
kernel is what the same restatement achieves in float32 on the same inputs: error <= 4 x the
float32 restatement's + 1e-6."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import loc2lang_reference as R
from graphconvgeo_amd import dense, geo
from graphconvgeo_amd import loc2lang as L
from graphconvgeo_amd import mdn as M
from graphconvgeo_amd._native import call
from graphconvgeo_amd.sparse import _ptr, _stream_handle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "profiles", "loc2lang", "accuracy.jsonl")
LAYER_SHAPES = [(B, C_) for B in (1, 7, 67, 130) for C_ in (1, 3, 64, 65, 100, 257, 1024)]
XENT_SHAPES = [(M_, N) for M_ in (1, 5, 67) for N in (1, 3, 255, 256, 257, 1024, 4097, 70001)]
REGIMES = ("wide", "tight")
SPREADS = (1.0, 30.0)
PLANES = ("dmus_lat", "dmus_lon", "dsigmas_lat", "dsigmas_lon", "dcorxy")
_layer_cache, _xent_cache = {}, {}


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def planes_of(grads):
    """The restatement's [dmus, dsigmas_raw, dcorxy_raw] as the kernel's five planes [5, C]."""
    dmus, dsig, dcor = grads
    return np.stack([dmus[:, 0], dmus[:, 1], dsig[:, 0], dsig[:, 1], dcor])


@pytest.fixture(scope="module")
def accuracy_log():
    records = {}
    yield records
    want = len(REGIMES) * len(LAYER_SHAPES) + len(SPREADS) * len(XENT_SHAPES)
    if len(records) == want:  # both sweeps ran whole: rewrite the file
        os.makedirs(os.path.dirname(ACCURACY), exist_ok=True)
        with open(ACCURACY, "w") as f:
            for key in sorted(records):
                f.write(json.dumps(records[key]) + "\n")


# -- 1. the Gaussian layer -----------------------------------------------------------------------
def layer_inputs(B, C_):
    """Per regime: R.layer_inputs' arrays with the float64 and float32 restatements' G and
    gradient planes (computed once, never modified)."""
    key = (B, C_)
    if key not in _layer_cache:
        out = {}
        for regime in REGIMES:
            arrays = R.layer_inputs(B, C_, regime)
            out[regime] = (arrays, R.bigaus_and_grads(*arrays, torch.float64),
                           R.bigaus_and_grads(*arrays, torch.float32))
        _layer_cache[key] = out
    return _layer_cache[key]


def run_layer(cuda, X, mus, sig, cor, pad=0):
    B, C_ = X.shape[0], mus.shape[0]
    Xd, md, sd, cd = (torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (X, mus, sig, cor))
    G = torch.full((B, C_ + pad), 7.0, dtype=torch.float32, device=cuda)
    call("gcg_bigaus_layer_f32", B, C_, _ptr(Xd), _ptr(md), _ptr(sd), _ptr(cd), _ptr(G), C_ + pad,
         _stream_handle(cuda))
    if pad:  # the padding columns are never written
        assert bool((G[:, C_:] == 7.0).all())
    return G[:, :C_].cpu().numpy()


def run_backward(cuda, X, mus, sig, cor, dG, pad=0, scale=None):
    B, C_ = X.shape[0], mus.shape[0]
    Xd, md, sd, cd = (torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in (X, mus, sig, cor))
    dGd = torch.full((B, C_ + pad), float("nan"), dtype=torch.float32, device=cuda)
    dGd[:, :C_] = torch.from_numpy(dG)
    dparams = torch.full((5, C_), 7.0, dtype=torch.float32, device=cuda)
    nbytes = L.bigaus_backward_workspace_bytes(B, C_)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=cuda)
    scale_d = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=cuda)
    call("gcg_bigaus_layer_backward_f32", B, C_, _ptr(Xd), _ptr(md), _ptr(sd), _ptr(cd), _ptr(dGd),
         C_ + pad, _ptr(scale_d), _ptr(dparams), _ptr(ws), nbytes, _stream_handle(cuda))
    return dparams.cpu().numpy()


@pytest.mark.parametrize("B,C_", LAYER_SHAPES)
def test_layer_and_gradients_within_four_times_float32(cuda, accuracy_log, B, C_):
    """G and each of the five gradient planes separately: the largest error against float64 over
    the case's max|ref| <= 4 x the float32 restatement's + 1e-6. A padded ldg / lddg (the
    gradient's padding holding NaN) gives the same bits."""
    for regime, (arrays, (G64, g64), (G32, g32)) in layer_inputs(B, C_).items():
        assert np.isfinite(G32).all() and G64.max() > 0
        G = run_layer(cuda, *arrays[:4])
        assert same_bits(G, run_layer(cuda, *arrays[:4], pad=3))
        dp = run_backward(cuda, *arrays)
        assert same_bits(dp, run_backward(cuda, *arrays, pad=5))
        rec = {"kernel": "bigaus_layer", "B": B, "C": C_, "regime": regime}
        cases = [("G", G, G64, G32)] + [(n, dp[j], planes_of(g64)[j], planes_of(g32)[j])
                                        for j, n in enumerate(PLANES)]
        for name, got, ref, f32 in cases:
            assert got.shape == ref.shape
            top = np.abs(ref).max()
            if top == 0:
                assert not got.any(), name
                rec[name + "_err_kernel"] = rec[name + "_err_f32"] = 0.0
                continue
            rec[name + "_err_kernel"] = float(np.abs(got - ref).max() / top)
            rec[name + "_err_f32"] = float(np.abs(f32 - ref).max() / top)
        print(rec)
        accuracy_log[("bigaus", B, C_, regime)] = rec
        for name in ("G",) + PLANES:
            assert rec[name + "_err_kernel"] <= 4 * rec[name + "_err_f32"] + 1e-6, (name, rec)


def test_layer_scale_reproducibility_rows_and_autograd(cuda):
    """scale_dev multiplies every plane; dparams at 1000 x 100 (250 workgroups) is bitwise the
    same in two calls; a row of G is bitwise what a one-row call gives; autograd through
    bigaus_layer gives the restatement's gradients and none for X."""
    arrays, (G64, g64), _ = layer_inputs(67, 65)["tight"]
    p1 = run_backward(cuda, *arrays)
    p3 = run_backward(cuda, *arrays, scale=-2.5)
    assert np.allclose(p3, -2.5 * p1, rtol=1e-6, atol=1e-30)
    G = run_layer(cuda, *arrays[:4])
    for r in (0, 1, 33, 66):
        assert same_bits(run_layer(cuda, arrays[0][r:r + 1], *arrays[1:4]), G[r:r + 1]), r
    big = R.layer_inputs(1000, 100, "tight")
    a, b = run_backward(cuda, *big), run_backward(cuda, *big)
    assert same_bits(a, b) and np.isfinite(a).all() and a.any()
    ts = [torch.from_numpy(x).to(cuda) for x in arrays]
    for t in ts[:4]:
        t.requires_grad_(True)
    out = L.bigaus_layer(*ts[:4])
    assert same_bits(out.detach().cpu().numpy(), G)
    (3.0 * (out * ts[4]).sum()).backward()
    assert ts[0].grad is None
    want = planes_of(g64)
    got = np.stack([ts[1].grad[:, 0].cpu().numpy(), ts[1].grad[:, 1].cpu().numpy(),
                    ts[2].grad[:, 0].cpu().numpy(), ts[2].grad[:, 1].cpu().numpy(),
                    ts[3].grad.cpu().numpy()])
    assert ts[1].grad.shape == (65, 2) and ts[3].grad.shape == (65,)
    for j in range(5):
        assert np.abs(got[j] - 3.0 * want[j]).max() <= 1e-5 * np.abs(3.0 * want[j]).max(), j
    layer = L.BivariateGaussianLayer(65, *(arrays[i] for i in (1, 2, 3)), device=cuda)
    assert same_bits(layer(ts[0].detach()).detach().cpu().numpy(), G)


# -- 2. the soft cross-entropy -------------------------------------------------------------------
def xent_inputs(M_, N):
    """Per spread: (Z, Y, rows), the dense Y[rows] and the float64 / float32 restatements' row
    losses and gradient of their sum (computed once, never modified)."""
    key = (M_, N)
    if key not in _xent_cache:
        out = {}
        for spread in SPREADS:
            Z, Y, rows = R.xent_inputs(M_, N, spread)
            Yd = np.asarray(Y[rows].todense())
            out[spread] = ((Z, Y, rows), R.soft_xent_and_grad(Z, Yd, torch.float64),
                           R.soft_xent_and_grad(Z, Yd, torch.float32))
        _xent_cache[key] = out
    return _xent_cache[key]


def run_xent(cuda, Z, Y, rows, pad=0, pad_value=0.0, scale=1.0, scale_dev=None, grad=True,
             alias=False, target=True):
    """One gcg_softmax_xent_csr_f32 call on row strides N + pad: (loss_rows, out) as NumPy."""
    M_, N = Z.shape
    Zd = torch.full((M_, N + pad), pad_value, dtype=torch.float32, device=cuda)
    Zd[:, :N] = torch.from_numpy(Z)
    Yd = L.target_csr(Y, cuda) if target else None
    rd = None if rows is None else torch.from_numpy(rows).to(cuda)
    out = None
    if grad:
        out = Zd if alias else torch.full((M_, N + pad), 7.0, dtype=torch.float32, device=cuda)
    loss = torch.full((M_,), 7.0, dtype=torch.float32, device=cuda)
    sd = None if scale_dev is None else torch.tensor([scale_dev], dtype=torch.float32, device=cuda)
    y_args = (Yd.n_rows, _ptr(Yd.indptr), _ptr(Yd.indices), _ptr(Yd.data)) if target else \
        (0, None, None, None)
    call("gcg_softmax_xent_csr_f32", M_, N, _ptr(Zd), N + pad, *y_args, _ptr(rd),
         float(scale), _ptr(sd), _ptr(out), N + pad, _ptr(loss), _stream_handle(cuda))
    if grad and pad and not alias:
        assert bool((out[:, N:] == 7.0).all())
    return loss.cpu().numpy(), None if out is None else out[:, :N].cpu().numpy()


@pytest.mark.parametrize("M_,N", XENT_SHAPES)
def test_soft_xent_within_four_times_float32(cuda, accuracy_log, M_, N):
    """loss_rows over max(1, |ref|) and the gradient over max|ref|: error against float64
    <= 4 x the float32 restatement's + 1e-6; target rows empty, with one entry, a few, and
    (N <= 257) full, reached through rows with repeats and out of order. The losses alone
    (out NULL), out written over the logits, and a padded row stride give the same bits."""
    for spread, ((Z, Y, rows), (l64, g64), (l32, g32)) in xent_inputs(M_, N).items():
        loss, g = run_xent(cuda, Z, Y, rows)
        only, none = run_xent(cuda, Z, Y, rows, grad=False)
        assert none is None and same_bits(only, loss)
        la, ga = run_xent(cuda, Z, Y, rows, alias=True)
        assert same_bits(la, loss) and same_bits(ga, g)
        lp, gp = run_xent(cuda, Z, Y, rows, pad=3, pad_value=float("nan"))
        assert same_bits(lp, loss) and same_bits(gp, g)

        def loss_err(r):
            return float((np.abs(r - l64) / np.maximum(1.0, np.abs(l64))).max())

        rec = {"kernel": "softmax_xent_csr", "M": M_, "N": N, "spread": spread,
               "loss_err_kernel": loss_err(loss), "loss_err_f32": loss_err(l32)}
        top = np.abs(g64).max()
        if top == 0:
            assert not g.any()
            rec["grad_err_kernel"] = rec["grad_err_f32"] = 0.0
        else:
            rec["grad_err_kernel"] = float(np.abs(g - g64).max() / top)
            rec["grad_err_f32"] = float(np.abs(g32 - g64).max() / top)
        print(rec)
        accuracy_log[("xent", M_, N, spread)] = rec
        for name in ("loss", "grad"):
            assert rec[name + "_err_kernel"] <= 4 * rec[name + "_err_f32"] + 1e-6, (name, rec)
        empty = np.asarray(Y[rows].sum(axis=1)).ravel() == 0
        assert not loss[empty].any() and not g[empty].any()


def test_soft_xent_rows_scale_and_reproducibility(cuda):
    """rows NULL equals rows = arange on the gathered target; scale and scale_dev multiply the
    gradient; two calls agree bitwise; a row's loss and gradient are bitwise those of a one-row
    call (independent of M and of the row's position, 16-B aligned or not)."""
    (Z, Y, rows), _, _ = xent_inputs(67, 4097)[30.0]
    loss, g = run_xent(cuda, Z, Y, rows)
    l2, g2 = run_xent(cuda, Z, Y, rows)
    assert same_bits(loss, l2) and same_bits(g, g2)
    Yg = sps.csr_matrix(Y[rows])
    l0, g0 = run_xent(cuda, Z, Yg, None)
    assert same_bits(l0, loss) and same_bits(g0, g)
    ls, gs_ = run_xent(cuda, Z, Y, rows, scale=0.5, scale_dev=-3.0)
    assert same_bits(ls, loss) and np.allclose(gs_, -1.5 * g, rtol=1e-6, atol=1e-30)
    for r in (0, 1, 2, 3, 40, 66):  # N = 4097 odd: rows 1, 2, 3 start off a 16-B boundary
        l1, g1 = run_xent(cuda, Z[r:r + 1], Y, rows[r:r + 1])
        assert same_bits(l1, loss[r:r + 1]) and same_bits(g1, g[r:r + 1]), r
    # a row id out of range on the device: a NaN loss and a zero gradient row, nothing indexed
    bad = rows.copy()
    bad[5], bad[9] = Y.shape[0], -1
    lb, gb = run_xent(cuda, Z, Y, bad)
    ok = np.ones(67, bool)
    ok[[5, 9]] = False
    assert np.isnan(lb[~ok]).all() and not gb[~ok].any()
    assert same_bits(lb[ok], loss[ok]) and same_bits(gb[ok], g[ok])


@pytest.mark.parametrize("N", [1, 3, 257, 4097, 70001])
def test_softmax_wide_against_float64(cuda, N):
    """y_indptr NULL: out = softmax(logits), against torch.softmax in float64; rows sum to 1
    within 1e-6; NaN in the ldl padding reaches nothing."""
    for spread in SPREADS:
        Z = R.xent_inputs(5, N, spread)[0]
        want = torch.softmax(torch.tensor(Z, dtype=torch.float64), dim=1).numpy()
        _, got = run_xent(cuda, Z, None, None, pad=2, pad_value=float("nan"), target=False)
        assert np.abs(got - want).max() <= 1e-6 and np.abs(got.sum(axis=1) - 1).max() <= 1e-6
        Zd = torch.from_numpy(Z).to(cuda)
        assert same_bits(L.softmax_wide(Zd).cpu().numpy(), got)
        assert same_bits(L.softmax_wide(Zd, out=Zd).cpu().numpy(), got)


@pytest.mark.parametrize("N", [3, 257, 1024, 4096])
def test_one_hot_targets_agree_with_the_label_kernel(cuda, N):
    """One-hot target rows: the mean loss and its gradient agree with dense.softmax_xent (integer
    labels, N <= 4096) within the bar of the sweep."""
    rng = np.random.default_rng(N)
    for spread in SPREADS:
        Z = (spread * rng.standard_normal((67, N))).astype(np.float32)
        labels = rng.integers(0, N, size=67)
        Y = sps.csr_matrix((np.ones(67, np.float32), (np.arange(67), labels)), shape=(67, N))
        l64, g64 = R.soft_xent_and_grad(Z, Y.toarray(), torch.float64, scale=1 / 67)
        l32, g32 = R.soft_xent_and_grad(Z, Y.toarray(), torch.float32, scale=1 / 67)
        za = torch.from_numpy(Z).to(cuda).requires_grad_(True)
        zb = torch.from_numpy(Z).to(cuda).requires_grad_(True)
        la = L.softmax_xent_csr(za, L.target_csr(Y, cuda))
        lb, _ = dense.softmax_xent(zb, torch.from_numpy(labels).to(cuda))
        la.backward()
        lb.backward()
        bar_l = 4 * abs(l32.mean() - l64.mean()) / max(1.0, abs(l64.mean())) + 1e-6
        top = np.abs(g64).max()
        bar_g = 4 * np.abs(g32 - g64).max() / top + 1e-6
        assert abs(float(la) - l64.mean()) <= bar_l * max(1.0, abs(l64.mean()))
        assert abs(float(la) - float(lb)) <= bar_l * max(1.0, abs(l64.mean()))
        ga, gb = za.grad.cpu().numpy(), zb.grad.cpu().numpy()
        assert np.abs(ga - g64).max() <= bar_g * top
        assert np.abs(ga - gb).max() <= bar_g * top


def test_soft_xent_autograd_rows_and_denominator(cuda):
    (Z, Y, rows), (l64, g64), _ = xent_inputs(67, 1024)[1.0]
    Yd = L.target_csr(Y, cuda)
    z = torch.from_numpy(Z).to(cuda).requires_grad_(True)
    loss = L.softmax_xent_csr(z, Yd, rows=rows)             # host rows: validated
    (2.0 * loss).backward()
    assert abs(float(loss) - l64.mean()) <= 1e-5 * abs(l64.mean())
    assert np.abs(z.grad.cpu().numpy() - 2.0 * g64 / 67).max() <= 1e-6 * np.abs(g64).max()
    z2 = torch.from_numpy(Z).to(cuda)
    l_dev = L.softmax_xent_csr(z2, Yd, rows=torch.from_numpy(rows).to(cuda), denom=100)
    assert abs(float(l_dev) - l64.sum() / 100) <= 1e-5 * abs(l64.sum() / 100)
    bad = rows.copy()
    bad[3] = Y.shape[0]
    with pytest.raises(ValueError, match="outside"):
        L.softmax_xent_csr(z2, Yd, rows=bad)
    with pytest.raises(ValueError, match="integer row ids"):
        L.softmax_xent_csr(z2, Yd, rows=rows[:5])
    dup = sps.csr_matrix((np.ones(3, np.float32), np.array([1, 1, 2], np.int32),
                          np.array([0, 3], np.int32)), shape=(1, 1024))
    from graphconvgeo_amd.sparse import DeviceCSR
    raw = DeviceCSR(*(torch.from_numpy(a).to(cuda) for a in (dup.indptr, dup.indices, dup.data)),
                    dup.shape)
    with pytest.raises(ValueError, match="twice"):
        L.softmax_xent_csr(z2[:1], raw)


# -- 3. Adamax -----------------------------------------------------------------------------------
def test_fused_adamax_matches_elementwise_formula(cuda):
    """gcg_adamax_step_f32 (one launch per parameter) against lasagne.updates.adamax written out
    elementwise in float64, over five steps (loc2lang.py:207)."""
    g0 = torch.Generator(device=cuda).manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g0, device=cuda))
          for s in ((300, 7), (1,), ((1 << 20) + 3,))]
    ref = [p.detach().double().clone() for p in ps]
    m = [torch.zeros_like(r) for r in ref]
    u = [torch.zeros_like(r) for r in ref]
    opt = L.LasagneAdamax(ps)
    assert opt.lr == 2e-3
    for t in range(1, 6):
        grads = [torch.randn(p.shape, generator=g0, device=cuda) for p in ps]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step()
        a = 2e-3 / (1 - 0.9 ** t)
        for i, g in enumerate(grads):
            g = g.double()
            m[i] = 0.9 * m[i] + 0.1 * g
            u[i] = torch.maximum(0.999 * u[i], g.abs())
            ref[i] = ref[i] - a * m[i] / (u[i] + 1e-8)
        for p, r in zip(ps, ref):
            err = float((p.detach().double() - r).abs().max())
            print("adamax step", t, tuple(p.shape), err)
            assert err < 1e-6, t
    assert all(p._version >= 5 for p in ps)
    assert all(x._version >= 5 for x in opt.m + opt.u)
    st = opt.state()
    opt2 = L.LasagneAdamax(ps)
    opt2.load_state(st)
    assert opt2.t == 5 and all(torch.equal(a_, b_) for a_, b_ in zip(opt2.u, opt.u))
    opt.zero_grad()
    assert all(p.grad is None for p in ps)


# -- 4. the trainer ------------------------------------------------------------------------------
def model(cuda, hid, init, B, **kw):
    kw.setdefault("n_epochs", 8)
    return L.NNModel_loc2lang(batch_size=B, hid_size=hid, n_gaus_comp=init[0].shape[0],
                              init_parameters=init, device=cuda, **kw)


@pytest.mark.parametrize("hid", [8, 0])
@pytest.mark.parametrize("tight", [True, False])
def test_trajectory_matches_the_float64_trainer(cuda, hid, tight):
    """3 batches per epoch, 8 epochs = 24 Adamax steps, the same orders fed to both: every batch
    loss and dev loss within 1e-4 max(1, |ref|), every final parameter within rtol 1e-4,
    atol 1e-5 of the float64 trainer (the float32 CPU trainer is, tests/test_loc2lang_reference.py)."""
    Xtr, Ytr, Xdev, Ydev, init, orders, B = R.parity_problem(hid=hid, tight=tight)
    clf = model(cuda, hid, init, B, early_stopping_max_down=8)
    ppl_test, ppl_dev = clf.fit(Xtr, Ytr, Xdev, Ydev, Xdev[:7], Ydev[:7], epoch_orders=orders)
    hist, params = R.train(Xtr, Ytr, Xdev, Ydev, init, orders, B)
    assert len(clf.history) == 8
    got_b = np.array(clf.epoch_batch_losses)
    ref_b = np.array([h["batch_losses"] for h in hist])
    got_v = np.array([h["val_loss"] for h in clf.history])
    ref_v = np.array([h["val_loss"] for h in hist])
    print("batch", np.abs(got_b - ref_b).max(), "dev", np.abs(got_v - ref_v).max())
    assert got_b.shape == ref_b.shape == (8, 3)
    assert np.all(np.abs(got_b - ref_b) <= 1e-4 * np.maximum(1.0, np.abs(ref_b)))
    assert np.all(np.abs(got_v - ref_v) <= 1e-4 * np.maximum(1.0, np.abs(ref_v)))
    got_t = np.array([h["train_loss"] for h in clf.history])
    assert np.allclose(got_t, ref_b.mean(axis=1), rtol=1e-4)
    assert ref_b[-1].mean() < ref_b[0].mean()  # it trains
    for name, got in zip(R.names(hid), clf.last_params):  # after the last step, before restore
        dev_gpu = np.abs(got - params[name]).max()
        print(name, "deviation from float64:", dev_gpu)
        assert got.shape == params[name].shape
        assert np.allclose(got, params[name], rtol=1e-4, atol=1e-5), name
    # natural-log loss, base 2, as the reference computes its perplexity
    assert ppl_dev == np.power(2, clf.dev_loss) and ppl_test == np.power(2, clf.test_loss)
    assert abs(ppl_dev - 2 ** clf.dev_loss) <= 1e-12 * ppl_dev
    assert clf.dev_loss == clf.best_val_loss  # the best parameters are back


@pytest.fixture(scope="module")
def problem():
    return R.parity_problem(hid=8, tight=True)


def test_selection_rule_restore_early_stop_and_api(cuda, problem):
    Xtr, Ytr, Xdev, Ydev, init, orders, B = problem
    # A step size of 0.5 is far too large for the problem: the float64 trainer's dev loss is
    # 2.713 after the first epoch and rises from there (2.777, 2.840, ...), so the first epoch is
    # kept and training stops after the third.
    clf = model(cuda, 8, init, B, n_epochs=8, early_stopping_max_down=1)
    clf._build(37)
    clf.optimizer.lr = 0.5
    ppl_test, ppl_dev = clf.fit(Xtr, Ytr.toarray(), Xdev, Ydev, Xdev, Ydev, epoch_orders=orders)
    vals = [h["val_loss"] for h in clf.history]
    best, kept, down, stopped = float("inf"), None, 0, False
    for i, v in enumerate(vals):  # the reference's rule, restated
        assert not stopped
        if v < best and best - v > 1e-4 * v:
            best, kept, down = v, i, 0
        else:
            down += 1
            stopped = down > 1
    print(vals, kept)
    assert stopped and len(vals) == 3 and kept == 0
    assert not all(np.array_equal(a, b) for a, b in zip(clf.last_params, clf.get_params()))
    assert clf.best_val_loss == best
    assert clf.dev_loss == best and ppl_dev == np.power(2, best)  # the best parameters are back
    assert ppl_test == ppl_dev and isinstance(float(ppl_test), float)
    probs = clf.predict(Xdev)
    assert probs.shape == (40, 37) and probs.dtype == np.float32
    assert np.abs(probs.sum(axis=1) - 1).max() <= 1e-5 and probs.min() >= 0
    want = R.predict(Xdev, dict(zip(R.names(8), clf.get_params())))
    assert np.abs(probs - want).max() <= 1e-5
    g = clf.gaus_output(Xdev)
    assert g.shape == (40, 5) and (g >= 0).all()
    got = clf.get_params()
    assert [p.shape for p in got] == [(5, 2), (5, 2), (5,), (5, 8), (8,), (8, 37), (37,)]
    clf.set_params(init)
    assert all(np.array_equal(a, b) for a, b in zip(clf.get_params(), init))
    assert np.abs(clf.predict(Xdev) - R.predict(Xdev, dict(zip(R.names(8), init)))).max() <= 1e-5
    # no epoch: the parameters stay (the reference would crash on set_all_param_values(None))
    clf0 = model(cuda, 8, init, B, n_epochs=0)
    clf0.fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev)
    assert all(np.array_equal(a, b) for a, b in zip(clf0.get_params(), init))
    assert clf0.history == [] and clf0.best_val_loss == float("inf")


def test_refusals(cuda, problem):
    Xtr, Ytr, Xdev, Ydev, init, orders, B = problem
    with pytest.raises(NotImplementedError, match="grid"):
        model(cuda, 8, init, B).fit(sps.csr_matrix(Xtr), Ytr, Xdev, Ydev, Xdev, Ydev)
    with pytest.raises(ValueError, match="permutation"):
        model(cuda, 8, init, B, n_epochs=1).fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev,
                                                epoch_orders=[np.zeros(96, np.int64)])
    with pytest.raises(ValueError, match="init_parameters must be"):
        model(cuda, 0, init, B).fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev)
    with pytest.raises(ValueError, match="fewer than one batch"):
        model(cuda, 8, init, 97).fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev)
    with pytest.raises(ValueError, match="differ in width"):
        model(cuda, 8, init, B).fit(Xtr, Ytr, Xdev, Ydev[:, :30], Xdev, Ydev)
    with pytest.raises(ValueError, match="output_size says"):
        model(cuda, 8, init, B, output_size=37).fit(Xtr, Ytr[:, :30], Xdev, Ydev[:, :30], Xdev,
                                                    Ydev[:, :30])
    with pytest.raises(ValueError, match=r"shape \(n, 2\)"):
        model(cuda, 8, init, B).fit(Xtr[:, :1], Ytr, Xdev, Ydev, Xdev, Ydev)


def test_default_init_draws_in_lasagne_construction_order(cuda):
    C_, V = 6, 11
    given = np.full((C_, 2), 3.0, np.float32)
    for hid in (4, 0):
        for mus in (None, given):
            np.random.seed(77)
            clf = L.NNModel_loc2lang(output_size=V, hid_size=hid, n_gaus_comp=C_, mus=mus,
                                     device=cuda)
            rs = np.random.RandomState(77)
            want = [rs.randn(C_, 2).astype(np.float32) if mus is None else given,
                    np.full((C_, 2), 10.0, np.float32), rs.randn(C_).astype(np.float32)]
            for a, b in ([(C_, hid)] if hid else []) + [(hid or C_, V)]:
                lim = np.sqrt(6.0 / (a + b))
                want += [rs.uniform(-lim, lim, size=(a, b)).astype(np.float32),
                         np.zeros(b, np.float32)]
            got = clf.get_params()
            assert len(got) == len(want) == (7 if hid else 5)
            for g, w in zip(got, want):
                assert np.array_equal(g, w)
    np.random.seed(5)
    layer = L.BivariateGaussianLayer(C_, device=cuda)
    rs = np.random.RandomState(5)
    assert np.array_equal(layer.mus.detach().cpu().numpy(), rs.randn(C_, 2).astype(np.float32))
    assert bool((layer.sigmas == 10).all())
    assert np.array_equal(layer.corxy.detach().cpu().numpy(), rs.randn(C_).astype(np.float32))


@pytest.mark.parametrize("hid", [8, 0])
def test_epoch_runs_without_host_synchronisation(cuda, hid):
    Xtr, Ytr, Xdev, Ydev, init, orders, B = R.parity_problem(hid=hid, tight=True)
    clf = model(cuda, hid, init, B, n_epochs=1)
    clf.fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev, epoch_orders=orders)  # builds every lazy resource
    clf._prepare_epoch(orders[1])
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = clf._run_batches()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert np.isfinite(float(loss)) and len(clf.batch_losses) == 3


def test_evaluation_chunks_do_not_change_the_loss(cuda, problem, monkeypatch):
    """40 dev rows in chunks of 7: the mean over all rows, not over whole chunks. The GEMMs in
    front of the loss may tile a 7-row problem differently from a 40-row one, so the bound is
    float32 rounding (1e-6 relative), not equality."""
    Xtr, Ytr, Xdev, Ydev, init, orders, B = problem
    clf = model(cuda, 8, init, B, n_epochs=0)
    clf.fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev)
    whole, probs = clf.dev_loss, clf.predict(Xdev)
    p64 = R.predict(Xdev, dict(zip(R.names(8), init)))
    ref = float(-(Ydev.toarray() * np.log(p64)).sum(axis=1).mean())
    assert abs(whole - ref) <= 1e-5 * ref
    monkeypatch.setattr(L, "EVAL_CHUNK_BYTES", 4 * 40 * 8)  # 7 rows of 40 floats per chunk
    assert clf._chunk_rows() == 7
    x, Yd = clf._split(Xdev, Ydev, "dev")
    assert abs(clf._evaluate(x, Yd) - whole) <= 1e-6 * whole
    assert np.abs(clf.predict(Xdev) - probs).max() <= 1e-6


# -- 5. two regions ------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", [0, 8])
def test_two_regions(cuda, hid):
    """400 training and 100 dev points around the two Melbournes (sigma 0.5 degrees), V = 20 (8
    words per place, 4 common; 3 own + 1 common word per row), C = 4 components from two k-d-tree
    regions per place (geo.KDTreeClustering, bucket 100) through cluster_params, B = 50, 60
    epochs = 480 Adamax steps. The float64 CPU trainer on the same data runs first and is shown
    to learn: its dev loss falls 3.007 -> 2.835 (no hidden layer) / 2.748 (hid 8), and at each
    centre the predicted mass on the place's own 8 words exceeds that on the other place's by
    0.57 / 0.34 (no hidden layer) and 0.63 / 0.49 (hid 8); asserted of it: a fall of more than
    0.15 and margins of at least 0.3. Of the GPU fit: the dev-loss history within 1e-4 relative
    of float64's, and the same margins."""
    Xtr, Ytr, Xdev, Ydev = R.two_regions_data()
    tree = geo.KDTreeClustering(100).fit(Xtr, device=cuda)
    labels, C_ = tree.clusters.cpu().numpy(), tree.num_clusters
    assert C_ == 4
    comp = M.cluster_params(Xtr, labels, C_, raw=True)
    near = np.abs(comp[0][:, None, :] - R.MELBOURNES[None]).max(axis=-1) < 3.0
    assert near[:, 0].sum() == 2 and near[:, 1].sum() == 2
    init = R.two_regions_init(comp, hid)
    rs = np.random.RandomState(7)
    orders = [rs.permutation(400) for _ in range(60)]
    hist, p64 = R.train(Xtr, Ytr, Xdev, Ydev, init, orders, 50)
    ref = np.array([h["val_loss"] for h in hist])
    margin64 = R.own_word_margin(R.predict(R.MELBOURNES, p64))
    print("float64: dev", ref[0], ref[-1], "margins", margin64)
    assert ref[0] - ref[-1] > 0.15 and margin64.min() >= 0.3

    clf = L.NNModel_loc2lang(n_epochs=60, batch_size=50, hid_size=hid, n_gaus_comp=C_,
                             early_stopping_max_down=60, init_parameters=init, device=cuda)
    clf.fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev, epoch_orders=orders)
    got = np.array([h["val_loss"] for h in clf.history])
    print("gpu: dev", got[0], got[-1], "largest deviation", np.abs(got - ref).max())
    assert got.shape == ref.shape == (60,)
    assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref))
    margin =R.own_word_margin(clf.predict(R.MELBOURNES))
    print("gpu: margins", margin)
    assert margin.min() >= 0.3
