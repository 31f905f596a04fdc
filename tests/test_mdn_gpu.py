"""GPU tests of the mixture-density location head (graphconvgeo_amd.mdn, csrc/mdn.hip, the
dropout segmentation of csrc/minibatch.hip; reference lang2loc.py). The judge for numbers is
tests/mdn_reference.py in float64; the bar for the fused NLL is what the same restatement
achieves in float32 on the same inputs."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import mdn_reference as R
from graphconvgeo_amd import dropout as D
from graphconvgeo_amd import mdn as M
from graphconvgeo_amd import mlp
from graphconvgeo_amd import sparse as gs
from graphconvgeo_amd._native import call
from graphconvgeo_amd.sparse import _ptr, _stream_handle
from graphconvgeo_amd.synth import glorot_uniform, synthetic_features
from test_mlp_gpu import ragged_csr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "profiles", "mdn", "accuracy.jsonl")
BATCHES = (1, 7, 67, 130)
COMPONENTS = (1, 3, 64, 65, 100, 257, 1024)
SHAPES = [(B, C_) for B in BATCHES for C_ in COMPONENTS]
_cache = {}


def inputs(B, C_):
    """O ~ N(0, 1) and 3 N(0, 1), y uniform in [-60, 60] x [-170, 170], one generator seeded 77
    per shape; with the float64 and float32 restatements' losses and gradients (computed once,
    never modified)."""
    key = (B, C_)
    if key not in _cache:
        gen = torch.Generator().manual_seed(77)
        out = {}
        for scale in (1.0, 3.0):
            O = (scale * torch.randn(B, 6 * C_, generator=gen)).numpy().astype(np.float32)
            Y = ((torch.rand(B, 2, generator=gen) * 2 - 1) *
                 torch.tensor([60.0, 170.0])).numpy().astype(np.float32)
            out[scale] = (O, Y, R.nll_and_grad(O, Y, C_, torch.float64),
                          R.nll_and_grad(O, Y, C_, torch.float32))
        _cache[key] = out
    return _cache[key]


def run_nll(cuda, O, Y, C_, pad=0, grad=True, rows=True, scale=None):
    """One gcg_mdn_nll_f32 call on row strides 6C + pad: (loss, loss_rows, dO) as NumPy."""
    B = O.shape[0]
    Od = torch.zeros((B, 6 * C_ + pad), dtype=torch.float32, device=cuda)
    Od[:, :6 * C_] = torch.from_numpy(O)
    Yd = torch.from_numpy(Y).to(cuda)
    dO = torch.full((B, 6 * C_ + pad), 7.0, dtype=torch.float32, device=cuda) if grad else None
    lr = torch.empty(B, dtype=torch.float32, device=cuda) if rows else None
    ws = None if rows else torch.empty(B, dtype=torch.float32, device=cuda)
    loss = torch.empty((), dtype=torch.float32, device=cuda)
    sd = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=cuda)
    call("gcg_mdn_nll_f32", B, C_, _ptr(Od), 6 * C_ + pad, _ptr(Yd), _ptr(sd), _ptr(dO),
         6 * C_ + pad, _ptr(lr), _ptr(loss), _ptr(ws), 0 if ws is None else 4 * B,
         _stream_handle(cuda))
    if grad and pad:  # the padding columns are never written
        assert bool((dO[:, 6 * C_:] == 7.0).all())
    return (loss.cpu().numpy(), None if lr is None else lr.cpu().numpy(),
            None if dO is None else dO[:, :6 * C_].cpu().numpy())


# -- 1. NLL and gradient -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy_log():
    records = {}
    yield records
    if len(records) == 2 * len(SHAPES):  # the whole sweep ran: rewrite the file
        os.makedirs(os.path.dirname(ACCURACY), exist_ok=True)
        with open(ACCURACY, "w") as f:
            for key in sorted(records):
                f.write(json.dumps(records[key]) + "\n")


@pytest.mark.parametrize("B,C_", SHAPES)
def test_nll_and_gradient_within_four_times_float32(cuda, accuracy_log, B, C_):
    """Kernel error against float64 <= 4 x the float32 restatement's + 1e-6: the loss per row
    over max(1, |ref|), the gradient's maximum over the matrix over max|ref|."""
    for scale, (O, Y, (r64, g64), (r32, g32)) in inputs(B, C_).items():
        assert np.isfinite(r32).all() and np.isfinite(g32).all()
        loss, rows, dO = run_nll(cuda, O, Y, C_)
        loss_p, rows_p, dO_p = run_nll(cuda, O, Y, C_, pad=5)  # padded rows: the same numbers
        assert np.array_equal(rows, rows_p) and np.array_equal(dO, dO_p) and loss == loss_p
        loss_n, rows_n, _ = run_nll(cuda, O, Y, C_, grad=False)  # dO NULL
        assert np.array_equal(rows, rows_n) and loss == loss_n
        loss_w, _, dO_w = run_nll(cuda, O, Y, C_, rows=False)    # loss_rows NULL (workspace)
        assert loss == loss_w and np.array_equal(dO, dO_w)

        def loss_err(r):
            return float((np.abs(r - r64) / np.maximum(1.0, np.abs(r64))).max())

        def grad_err(g):
            return float(np.abs(g - g64).max() / np.abs(g64).max())

        rec = {"B": B, "C": C_, "scale": scale, "loss_err_kernel": loss_err(rows),
               "loss_err_f32": loss_err(r32), "grad_err_kernel": grad_err(dO),
               "grad_err_f32": grad_err(g32)}
        print(rec)
        accuracy_log[(B, C_, scale)] = rec
        assert rec["loss_err_kernel"] <= 4 * rec["loss_err_f32"] + 1e-6, rec
        assert rec["grad_err_kernel"] <= 4 * rec["grad_err_f32"] + 1e-6, rec
        # the mean: the rows' bar (4 x 2.7e-6 + 1e-6) and the 8 roundings of its tree
        assert abs(float(loss) - r64.mean()) <= 2e-5 * max(1.0, np.abs(r64).mean())
        if C_ == 1:  # one component: pi = w = 1, the logit has no gradient
            assert not dO[:, 5].any()


@pytest.mark.parametrize("B,C_", [(7, 3), (130, 65), (1000, 100)])
def test_mean_is_reproducible_and_in_the_stated_order(cuda, B, C_):
    gen = torch.Generator().manual_seed(5)
    O = torch.randn(B, 6 * C_, generator=gen).numpy()
    Y = ((torch.rand(B, 2, generator=gen) * 2 - 1) * torch.tensor([60.0, 170.0])).numpy()
    a = run_nll(cuda, O, Y, C_)
    b = run_nll(cuda, O, Y, C_)
    assert a[0].view(np.int32) == b[0].view(np.int32)
    assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    assert a[0] == R.fixed_order_mean(a[1])


def test_upstream_scale_and_autograd(cuda):
    O, Y, (r64, _g64), _ = inputs(67, 65)[1.0]
    _, _, g1 = run_nll(cuda, O, Y, 65)
    _, _, g3 = run_nll(cuda, O, Y, 65, scale=-2.5)
    # two roundings apart; atol: the subnormal elements, where a relative bound means nothing
    assert np.allclose(g3, -2.5 * g1, rtol=1e-6, atol=1e-30)
    Od = torch.from_numpy(O).to(cuda).requires_grad_(True)
    loss = M.mdn_nll(Od, torch.from_numpy(Y).to(cuda))
    (3.0 * loss).backward()
    assert abs(float(loss.detach()) - r64.mean()) <= 1e-5 * abs(r64.mean())
    assert np.allclose(Od.grad.cpu().numpy(), 3.0 * g1, rtol=1e-6, atol=1e-30)


# -- 2. prediction -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C_", SHAPES)
def test_prediction_matches_the_float64_argmax(cuda, B, C_):
    O = inputs(B, C_)[1.0][0]
    O64 = torch.tensor(O, dtype=torch.float64)
    scores = R.pred_scores(O64, C_).numpy()
    want = scores.argmax(axis=1)
    top = np.sort(scores, axis=1)[:, ::-1]
    clear = np.ones(B, bool) if C_ == 1 else (top[:, 0] - top[:, 1]) >= 1e-4 * top[:, 0]
    assert (~clear).sum() <= 0.01 * B
    Od = torch.from_numpy(O).to(cuda)
    latlon, idx = M.mdn_predict(Od, C_, return_index=True)
    idx = idx.cpu().numpy()
    assert np.array_equal(idx[clear], want[clear])
    mus = M.unpack_params(Od, C_)[0].cpu().numpy()  # the kernel's own unpack
    assert np.array_equal(latlon.cpu().numpy().view(np.int32),
                          mus[np.arange(B), :, idx].view(np.int32))
    # a padded row stride and idx NULL give the same coordinates
    Op = torch.zeros((B, 6 * C_ + 3), dtype=torch.float32, device=cuda)
    Op[:, :6 * C_] = Od
    ll = torch.empty((B, 2), dtype=torch.float32, device=cuda)
    call("gcg_mdn_predict_f32", B, C_, _ptr(Op), 6 * C_ + 3, 0, None, _ptr(ll),
         _stream_handle(cuda))
    assert torch.equal(ll, latlon)
    lp, ip = M.mdn_predict(Od, C_, method="pi", return_index=True)
    logits = O.reshape(B, 6, C_)[:, 5]
    assert np.array_equal(ip.cpu().numpy(), logits.argmax(axis=1))
    assert np.array_equal(lp.cpu().numpy(), mus[np.arange(B), :, logits.argmax(axis=1)])


def test_unpack_matches_the_restatement(cuda):
    for scale in (1.0, 3.0):
        O = inputs(67, 100)[scale][0]
        got = [t.cpu().numpy() for t in M.unpack_params(torch.from_numpy(O).to(cuda), 100)]
        want = [t.numpy() for t in R.unpack_params(torch.tensor(O, dtype=torch.float64), 100)]
        for g, w in zip(got, want):
            assert g.shape == w.shape and g.dtype == np.float32
            assert np.abs(g - w).max() <= 4e-7 * max(1.0, np.abs(w).max())


@pytest.mark.parametrize("C_", [2, 70, 300])
def test_ties_pick_the_lower_index(cuda, C_):
    """Two identical components: their candidates score alike, bit for bit."""
    gen = torch.Generator().manual_seed(3)
    O = (0.3 * torch.randn(9, 6, C_, generator=gen))
    O[:, 5] = -3.0
    pairs = []
    for r in range(9):  # rows' twins at different places, the pair far ahead of the rest
        a = (r * 7) % C_
        b = (a + 1 + r) % C_ if (a + 1 + r) % C_ != a else (a + 1) % C_
        pairs.append((a, b))
        O[r, :, b] = O[r, :, a]
        O[r, 5, a] = O[r, 5, b] = 4.0
        O[r, 2:4, a] = O[r, 2:4, b] = -2.0  # the smallest sigmas: the highest density
    Od = O.reshape(9, 6 * C_).to(cuda)
    for method in ("mixture", "pi"):
        _, idx = M.mdn_predict(Od, C_, method=method, return_index=True)
        assert idx.cpu().tolist() == [min(p) for p in pairs], method


# -- 3. segmentation with dropout ----------------------------------------------------------------
def check_dropout_segments(cuda, X, perm, B, p, seed=(5 << 32) | 987654321, step0=3,
                           stream_id=2):
    Xd = gs.DeviceCSR.from_scipy(X, cuda)
    nb = len(perm) // B
    perm = np.asarray(perm[:nb * B], dtype=np.int32)
    nnz_sel = int(np.diff(X.indptr)[perm].sum())
    perm_d = torch.from_numpy(perm).to(cuda)
    plain = mlp.BatchSegments(Xd, perm_d, B, nnz_sel)
    stream = D.DropoutStream(seed, stream_id, cuda)
    stream.set_step(step0)
    spec = D.DropoutSpec(stream, p)
    vals_drop = torch.full((max(X.nnz, 1),), -5.0, dtype=torch.float32, device=cuda)[:X.nnz]
    seg = mlp.BatchSegments(Xd, perm_d, B, nnz_sel, spec, vals_drop)
    assert seg.first_step == step0 and stream.step == step0 + nb  # advanced by the batches
    # the structure is the plain call's (the segment arrays up to the number of segments)
    assert torch.equal(seg.batch_seg_ptr, plain.batch_seg_ptr)
    assert torch.equal(seg.ent_pos[:nnz_sel], plain.ent_pos[:nnz_sel])
    nseg = int(seg.batch_seg_ptr[-1])
    assert torch.equal(seg.seg_col[:nseg], plain.seg_col[:nseg])
    assert torch.equal(seg.seg_ptr[:nseg + 1], plain.seg_ptr[:nseg + 1])
    bsp, ptr = seg.batch_seg_ptr.cpu().numpy(), seg.seg_ptr.cpu().numpy()
    val, vd = seg.ent_val.cpu().numpy(), vals_drop.cpu().numpy()
    touched = np.zeros(X.nnz, bool)
    for b in range(nb):
        rows = perm[b * B:(b + 1) * B]
        Xb = R.masked_rows(X, rows, p, seed, step0 + b, stream_id)
        T = Xb.T.tocsr()  # stable: batch order, then storage order, explicit zeros kept
        e0 = ptr[bsp[b]]
        assert np.array_equal(val[e0:e0 + T.nnz].view(np.int32), T.data.view(np.int32)), b
        for i, r in enumerate(rows):
            s, e = X.indptr[r], X.indptr[r + 1]
            assert np.array_equal(vd[s:e].view(np.int32),
                                  Xb.data[Xb.indptr[i]:Xb.indptr[i + 1]].view(np.int32)), (b, r)
            touched[s:e] = True
        # the forward over the batch's rows with vals_drop: bitwise scipy on the masked matrix
        K = 5
        W = np.random.default_rng(b).standard_normal((X.shape[1], K)).astype(np.float32)
        Wd = torch.from_numpy(W).to(cuda)
        out = torch.empty((B, K), dtype=torch.float32, device=cuda)
        gs.spmm_rows(Xd, Wd, rows=perm_d[b * B:(b + 1) * B], vals=vals_drop, out=out)
        assert np.array_equal(out.cpu().numpy().view(np.int32), (Xb @ W).view(np.int32)), b
    assert np.all(vd[~touched] == -5.0)  # rows outside the order are not written
    return seg, plain, stream, spec, vals_drop


@pytest.mark.parametrize("B", [32, 64])
def test_dropout_segmentation_matches_the_numpy_rule(cuda, B):
    X = ragged_csr()
    order = np.random.default_rng(3).permutation(257)
    seg, plain, stream, spec, vals_drop = check_dropout_segments(cuda, X, order, B, 0.5)
    assert seg.n_batches == 257 // B
    # the next call, the stream advanced: other masks for the same rows
    Xd = gs.DeviceCSR.from_scipy(X, cuda)
    perm_d = torch.from_numpy(order[:seg.n_batches * B].astype(np.int32)).to(cuda)
    again = mlp.BatchSegments(Xd, perm_d, B, seg.nnz_sel, spec, torch.empty_like(vals_drop))
    assert again.first_step == seg.first_step + seg.n_batches
    assert not torch.equal(again.ent_val, seg.ent_val)
    assert torch.equal(again.ent_pos, seg.ent_pos)


def test_dropout_segmentation_edge_shapes(cuda):
    check_dropout_segments(cuda, ragged_csr(n=130, f=1, max_nnz=3, seed=2),
                           np.random.default_rng(5).permutation(130), 32, 0.3)
    X = ragged_csr()
    order = np.concatenate([np.arange(8), np.arange(8, 257)])  # batch 0: the 8 empty rows
    check_dropout_segments(cuda, X, order, 8, 0.5)
    seg, *_ = check_dropout_segments(cuda, X, np.arange(8), 8, 0.5)  # no entry at all
    assert seg.nnz_sel == 0 and seg.batch_seg_ptr.cpu().tolist() == [0, 0]


def test_dropout_segmentation_with_p_zero_is_the_plain_call(cuda):
    X = ragged_csr()
    order = np.random.default_rng(3).permutation(257)
    seg, plain, *_ = check_dropout_segments(cuda, X, order, 64, 0.0)
    assert torch.equal(seg.ent_val.view(torch.int32), plain.ent_val.view(torch.int32))


# -- 4. the trainer ------------------------------------------------------------------------------
N_COMP, HID, BATCH = 5, 16, 50


@pytest.fixture(scope="module")
def problem():
    """n = 600 (400 train, 200 dev), F = 120: coordinates follow the features (three places,
    one degree of scatter), so the loss has something to learn."""
    X = synthetic_features(600, 120, nnz_per_row=12, empty_frac=0.02)
    rng = np.random.default_rng(0)
    place = np.asarray(X[:, :3].argmax(axis=1)).ravel()
    centres = np.array([[40.7, -74.0], [-33.9, 151.2], [51.5, -0.1]])
    Y = (centres[place] + rng.standard_normal((600, 2))).astype(np.float32)
    init = (glorot_uniform(120, HID), np.zeros(HID, np.float32),
            glorot_uniform(HID, 6 * N_COMP, seed=3), np.zeros(6 * N_COMP, np.float32))
    orders = [np.random.default_rng(9 + e).permutation(400) for e in range(3)]
    return X[:400], Y[:400], X[400:], Y[400:], init, orders


def model(cuda, init, **kw):
    kw.setdefault("n_epochs", 3)
    return M.NNModel_lang2loc(batch_size=BATCH, hid_size=HID, ncomp=N_COMP, init_parameters=init,
                              device=cuda, **kw)


@pytest.mark.parametrize("regul", [0, 1e-4])
def test_trajectory_matches_the_float64_trainer(cuda, problem, regul):
    """8 batches per epoch, 3 epochs = 24 Adam steps, the same orders fed to both."""
    Xtr, Ytr, Xdev, Ydev, init, orders = problem
    clf = model(cuda, init, regul_coef=regul).fit(Xtr, Ytr, Xdev, Ydev, epoch_orders=orders)
    hist, params = R.mdn_train(Xtr, Ytr, Xdev, Ydev, init, orders, BATCH, N_COMP, regul)
    for key in ("train_loss", "val_loss"):
        got = np.array([h[key] for h in clf.history])
        ref = np.array([h[key] for h in hist])
        print(key, got, ref)
        assert got.shape == ref.shape == (3,)
        assert np.all(np.abs(got - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref))), (key, got, ref)
    assert hist[-1]["train_loss"] < hist[0]["train_loss"]  # it trains
    assert clf.history[-1]["val_loss"] == min(h["val_loss"] for h in clf.history)
    for name, got in zip(("W1", "b1", "W2", "b2"), clf.get_params()):
        assert np.allclose(got, params[name], rtol=1e-4, atol=1e-5), name


def test_selection_rule_restore_and_api(cuda, problem):
    Xtr, Ytr, Xdev, Ydev, init, _ = problem
    np.random.seed(3)
    # fit's six further arguments of the reference are accepted and ignored
    clf = model(cuda, init, n_epochs=6, early_stopping_max_down=1, regul_coef=1e-6)
    clf.fit(Xtr, Ytr, Xdev, Ydev, None, None, list(range(400)), None, None, {})
    vals = [h["val_loss"] for h in clf.history]
    assert [h["epoch"] for h in clf.history] == list(range(len(vals))) and 1 <= len(vals) <= 6
    best = min(vals)
    first = vals.index(best)  # strict '<' keeps the first epoch that reaches the minimum
    assert clf.best_val_loss == best
    y_dev = torch.from_numpy(Ydev).to(cuda)
    assert float(clf._evaluate(clf.Xdev, y_dev)) == best  # the best parameters are back
    if len(vals) < 6:  # early stopping: max_down + 1 epochs without a new best
        assert len(vals) - 1 - first == 2
    pred = clf.predict(Xdev)
    assert pred.shape == (200, 2) and pred.dtype == np.float32
    mus, sigmas, corxy, pis = clf.predict_params(Xdev)
    assert mus.shape == sigmas.shape == (200, 2, N_COMP) and corxy.shape == pis.shape == (200, N_COMP)
    assert np.abs(pis.sum(axis=1) - 1).max() < 1e-5
    assert all((pred[i][:, None] == mus[i]).all(axis=0).any() for i in range(200))  # a mean
    assert clf.predict(Xdev, "pi").shape == (200, 2)
    # geo_eval_latlon against a NumPy haversine of those predictions
    lat1, lon1, lat2, lon2 = (np.radians(a.astype(np.float64)) for a in
                              (Ydev[:, 0], Ydev[:, 1], pred[:, 0], pred[:, 1]))
    h = np.sin((lat2 - lat1) / 2) ** 2 + np.cos(lat1) * np.cos(lat2) * np.sin((lon2 - lon1) / 2) ** 2
    km = 2 * 6371.0088 * np.arcsin(np.sqrt(h))
    mean, median, acc = M.geo_eval_latlon(pred, Ydev)
    assert abs(mean - km.mean()) <= 1e-9 * km.mean() and abs(median - np.median(km)) <= 1e-9 * np.median(km)
    assert acc == 100 * int((km < 161).sum()) / 200.0
    with pytest.raises(ValueError, match="must be sparse"):
        clf.predict(Xdev.toarray())
    with pytest.raises(ValueError, match="fewer than one batch"):
        model(cuda, init).fit(Xtr, Ytr, Xdev[:BATCH - 1], Ydev[:BATCH - 1])
    with pytest.raises(ValueError, match="permutation"):
        model(cuda, init, n_epochs=1).fit(Xtr, Ytr, Xdev, Ydev,
                                          epoch_orders=[np.zeros(400, np.int64)])


def test_default_init_draws_seed_then_w1_then_w2(cuda, problem):
    Xtr, Ytr, Xdev, Ydev, _, _ = problem
    for drop in (False, True):
        np.random.seed(77)
        clf = model(cuda, None, n_epochs=0, drop_out=drop).fit(Xtr, Ytr, Xdev, Ydev)
        rs = np.random.RandomState(77)
        seed = int(rs.randint(1, 2147462579)) if drop else None
        a1, a2 = np.sqrt(6.0 / (120 + HID)), np.sqrt(6.0 / (HID + 6 * N_COMP))
        W1 = rs.uniform(-a1, a1, size=(120, HID)).astype(np.float32)
        W2 = rs.uniform(-a2, a2, size=(HID, 6 * N_COMP)).astype(np.float32)
        got = clf.get_params()
        assert np.array_equal(got[0], W1) and np.array_equal(got[2], W2)
        assert not got[1].any() and not got[3].any()
        assert (clf._stream.seed if drop else None) == seed


def test_epoch_runs_without_host_synchronisation(cuda, problem, monkeypatch):
    """Every batch of an epoch, across two segmentation runs, with and without dropout, under
    sync debug mode 'error'."""
    Xtr, Ytr, Xdev, Ydev, init, orders = problem
    for drop in (False, True):
        np.random.seed(1)
        clf = model(cuda, init, n_epochs=1, drop_out=drop, regul_coef=1e-6)
        clf.fit(Xtr, Ytr, Xdev, Ydev)  # builds every lazy resource
        monkeypatch.setattr(mlp, "SEGMENT_CHUNK_ENTRIES", 3 * BATCH * 12)
        clf._prepare_epoch(orders[1])
        assert len(clf._runs) >= 2
        torch.cuda.synchronize()
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss = clf._run_batches()
        finally:
            torch.cuda.set_sync_debug_mode(before)
        assert np.isfinite(float(loss))


def test_dropout_fits_are_reproducible_and_p_zero_is_no_dropout(cuda, problem):
    Xtr, Ytr, Xdev, Ydev, init, orders = problem

    def fit(**kw):
        np.random.seed(21)
        clf = model(cuda, init, **kw).fit(Xtr, Ytr, Xdev, Ydev, epoch_orders=orders)
        return [p.view(np.int32) for p in clf.get_params()], clf.history

    a, b = fit(drop_out=True, dropout_coef=0.5), fit(drop_out=True, dropout_coef=0.5)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]
    plain, zero = fit(drop_out=False), fit(drop_out=True, dropout_coef=0)
    assert all(np.array_equal(x, y) for x, y in zip(plain[0], zero[0])) and plain[1] == zero[1]
    assert not all(np.array_equal(x, y) for x, y in zip(a[0], plain[0]))  # the mask acts


def test_dropout_first_epoch_matches_the_float64_trainer_under_the_same_masks(cuda, problem):
    Xtr, Ytr, Xdev, Ydev, init, orders = problem
    np.random.seed(21)
    clf = model(cuda, init, n_epochs=1, drop_out=True, dropout_coef=0.5, regul_coef=1e-6)
    clf.fit(Xtr, Ytr, Xdev, Ydev, epoch_orders=orders)
    hist, _ = R.mdn_train(Xtr, Ytr, Xdev, Ydev, init, orders[:1], BATCH, N_COMP, 1e-6,
                          drop=(0.5, clf._stream.seed))
    got, ref = clf.history[0], hist[0]
    print(got, ref)
    assert abs(got["train_loss"] - ref["train_loss"]) <= 1e-4 * max(1.0, abs(ref["train_loss"]))
    assert abs(got["val_loss"] - ref["val_loss"]) <= 1e-4 * max(1.0, abs(ref["val_loss"]))  # dev: no mask
    assert clf._stream.step == 8  # one step per batch


# -- 5. the reference's toy problem --------------------------------------------------------------
def test_melbourne_toy_problem(cuda):
    """lang2loc.load_toy_data (lang2loc.py:530-569) at 300 samples: 300 points around Melbourne,
    Florida and 600 around Melbourne, Australia, features that do not tell them apart. Batches
    of 10 give the 1800 Adam steps at lr 1e-3 the means need to travel; after 30 epochs every
    prediction lies within 5 degrees of one of the two centres and the dev loss has fallen."""
    n = 300
    rs = np.random.RandomState(11)
    centres = np.array([[28.0836, -80.6081], [-37.8136, 144.9631]])
    fl = rs.multivariate_normal(centres[0], np.eye(2), size=n).astype(np.float32)
    au = rs.multivariate_normal(centres[1], np.eye(2), size=2 * n).astype(np.float32)
    X = sps.csr_matrix(rs.uniform(-0.1, 0.1, size=(3 * n, 2)) + np.array([1, 0])).astype(np.float32)
    Y = np.vstack((fl, au))
    idx = np.arange(3 * n)
    rs.shuffle(idx)
    X, Y = X[idx], Y[idx]
    n_tr, n_dev = 2 * n, n // 2
    rs = np.random.RandomState(5)
    init = []
    for fan_in, fan_out in ((2, 100), (100, 24)):
        a = np.sqrt(6.0 / (fan_in + fan_out))
        init += [rs.uniform(-a, a, size=(fan_in, fan_out)).astype(np.float32),
                 np.zeros(fan_out, np.float32)]
    orders = [rs.permutation(n_tr) for _ in range(30)]
    clf = M.NNModel_lang2loc(n_epochs=30, batch_size=10, regul_coef=1e-6, hid_size=100, ncomp=4,
                             early_stopping_max_down=30, init_parameters=init, device=cuda)
    clf.fit(X[:n_tr], Y[:n_tr], X[n_tr:n_tr + n_dev], Y[n_tr:n_tr + n_dev], epoch_orders=orders)
    assert len(clf.history) == 30
    assert clf.history[-1]["val_loss"] < clf.history[0]["val_loss"]
    pred = clf.predict(X[n_tr:])
    assert pred.shape == (3 * n - n_tr, 2)
    off = np.abs(pred[:, None, :] - centres[None]).max(axis=-1).min(axis=-1)
    print("largest distance to a centre, degrees:", off.max())
    assert off.max() < 5.0
