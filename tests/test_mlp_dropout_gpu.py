"""GPU tests of the dropout MLP (graphconvgeo_amd.mlp.DropoutMLP) and of the rectify / dropout
backward beyond 1024 columns (gcg_rectify_backward_wide_f32): the training trajectory against
the float64 restatement under the same masks (tests/mlp_dropout_reference.py), segmentation
runs, p = 0 against MLP, the draw order, deterministic evaluation; the wide pass bit for bit
against the NumPy rule and sparse.column_sum per slab, through the layers and in the trainer."""
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import mlp_dropout_reference as DR
import mlp_reference as R
from graphconvgeo_amd import dropout as D
from graphconvgeo_amd import layers
from graphconvgeo_amd import mlp as M
from graphconvgeo_amd import sparse as gs
from graphconvgeo_amd._native import NativeError, call
from graphconvgeo_amd.sparse import _ptr, _stream_handle
from graphconvgeo_amd.synth import glorot_uniform
from test_backward_rule_gpu import N as GRAPH_N
from test_backward_rule_gpu import graph, operands
from test_mlp_gpu import problem

pytestmark = pytest.mark.gpu

COEFS = (1e-5, 1e-5)
B = 400


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# -- 1..5. the trainer ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def data():
    """test_mlp_gpu.problem() (1300 train rows, 300 features, 48 hidden, 9 classes) and five
    epoch orders; with B = 400: 3 batches and 100 dropped rows per epoch, 15 steps."""
    Xtr, Ytr, Xdev, Ydev, init = problem()
    rng = np.random.default_rng(9)
    orders = [rng.permutation(Xtr.shape[0]) for _ in range(5)]
    return Xtr, Ytr, Xdev, Ydev, init, orders


@functools.lru_cache(maxsize=None)
def reference_without_masks():
    Xtr, Ytr, Xdev, Ydev, init, orders = data()
    return R.mlp_train(Xtr, Ytr, Xdev, Ydev, init, orders, B, COEFS)[0]


def fit(cuda, hidden_dropout, coefs=(0.5, 0.5), cls=None, **kw):
    Xtr, Ytr, Xdev, Ydev, init, orders = data()
    np.random.seed(5)  # the two streams' seeds
    extra = {} if cls is M.MLP else {"drop_out_coefs": list(coefs),
                                     "hidden_dropout": hidden_dropout}
    clf = (cls or M.DropoutMLP)(n_epochs=5, batch_size=B, regul_coefs=COEFS, init_parameters=init,
                                hidden_layer_size=48, device=cuda, **extra, **kw)
    return clf.fit(Xtr, Ytr, Xdev, Ydev, epoch_orders=orders)


_FITS = {}


def fitted(cuda, hidden_dropout):
    """The single-run fit, shared by the tests that only read it."""
    if hidden_dropout not in _FITS:
        _FITS[hidden_dropout] = fit(cuda, hidden_dropout)
    return _FITS[hidden_dropout]


def losses(history):
    return (np.array([h["train_loss"] for h in history]),
            np.array([h["val_loss"] for h in history]))


@pytest.mark.parametrize("hidden_dropout", [False, True], ids=["reference_wiring", "hidden"])
def test_trajectory_matches_float64_reference_under_the_same_masks(cuda, hidden_dropout):
    """The bounds of test_mlp_trajectory_matches_float64_reference (the same arithmetic on masked
    operands): train loss within 1e-4 * max(1, |ref|), val loss rtol 1e-4 / atol 1e-5. The
    restatement without masks must miss both by a factor 10, or the test could not see a mask."""
    Xtr, Ytr, Xdev, Ydev, init, orders = data()
    clf = fitted(cuda, hidden_dropout)
    assert clf.stream_in.stream_id == 0 and clf.stream_hid.stream_id == 1
    assert (clf._drop_hid is not None) == hidden_dropout and clf._drop_in.p == 0.5
    m_in, m_hid = DR.stream_masks(clf, 300, 48, B)
    assert m_in is not None and (m_hid is not None) == hidden_dropout
    hist, _ = DR.mlp_dropout_train(Xtr, Ytr, Xdev, Ydev, init, orders, B, COEFS, m_in, m_hid)
    (got, gv), (ref, rv) = losses(clf.history), losses(hist)
    print("train_loss", got, ref)
    print("val_loss", gv, rv)
    assert got.shape == ref.shape == (5,)
    assert np.abs(got - ref).max() < 1e-4 * max(1.0, np.abs(ref).max()), (got, ref)
    assert np.allclose(gv, rv, rtol=1e-4, atol=1e-5)
    assert [h["train_acc"] for h in clf.history] == pytest.approx(
        [h["train_acc"] for h in hist], abs=1e-6)
    assert ref[-1] < ref[0]  # it trains
    # the steps ran on: 15 batches on both streams' clocks
    assert clf.stream_in.step == 15 and clf._steps_before == 15
    plain, pv = losses(reference_without_masks())
    print("without masks", plain, pv)
    assert np.abs(got - plain).max() > 10 * 1e-4 * max(1.0, np.abs(plain).max())
    assert (np.abs(gv - pv) > 10 * (1e-5 + 1e-4 * np.abs(pv))).any()


def test_segmentation_runs_continue_the_steps(cuda, monkeypatch):
    """Every epoch cut into three runs of one batch: bitwise the single-run fit."""
    one = fitted(cuda, True)
    assert len(one._runs) == 1
    monkeypatch.setattr(M, "SEGMENT_CHUNK_ENTRIES", 400 * 20 * 3 // 2)
    cut = fit(cuda, True)
    assert len(cut._runs) >= 2
    assert cut.stream_in.seed == one.stream_in.seed and cut.stream_in.step == 15
    for pa, pb in zip(one.get_params(), cut.get_params()):
        assert np.array_equal(bits(pa), bits(pb))
    assert one.history == cut.history


def test_p_zero_is_the_plain_trainer(cuda):
    drop = fit(cuda, False, coefs=(0.5, 0.0))
    assert drop._drop_in is None and drop._drop_hid is None and drop._vals_drop is None
    plain = fit(cuda, False, cls=M.MLP)
    for pa, pb in zip(drop.get_params(), plain.get_params()):
        assert np.array_equal(bits(pa), bits(pb))
    assert drop.history == plain.history
    assert (drop.best_dev_loss, drop.best_dev_acc) == (plain.best_dev_loss, plain.best_dev_acc)


def small_fit(cuda, seed, n_epochs, **kw):
    Xtr, Ytr, Xdev, Ydev, _ = problem(n=700, n_train=500, f=120, k=16, c=5)
    np.random.seed(seed)
    clf = M.DropoutMLP(n_epochs=n_epochs, batch_size=100, hidden_layer_size=16, device=cuda, **kw)
    return clf.fit(Xtr, Ytr, Xdev, Ydev)


@pytest.mark.parametrize("hidden_dropout", [False, True])
def test_draws_in_lasagnes_construction_order(cuda, hidden_dropout):
    """seed, Glorot, seed, Glorot from numpy's global stream -- the hidden layer's seed whether
    or not its mask is on; with init_parameters only the two seeds."""
    clf = small_fit(cuda, 77, 0, hidden_dropout=hidden_dropout)
    rs = np.random.RandomState(77)
    a1, a2 = np.sqrt(3) * np.sqrt(2.0 / (120 + 16)), np.sqrt(3) * np.sqrt(2.0 / (16 + 5))
    seed_in = rs.randint(1, 2147462579)
    W1 = rs.uniform(-a1, a1, size=(120, 16)).astype(np.float32)
    seed_hid = rs.randint(1, 2147462579)
    W2 = rs.uniform(-a2, a2, size=(16, 5)).astype(np.float32)
    got = clf.get_params()
    assert (clf.stream_in.seed, clf.stream_hid.seed) == (seed_in, seed_hid)
    assert np.array_equal(got[0], W1) and np.array_equal(got[2], W2)
    assert not got[1].any() and not got[3].any()
    again = small_fit(cuda, 77, 0, hidden_dropout=hidden_dropout, init_parameters=got)
    rs = np.random.RandomState(77)
    assert (again.stream_in.seed, again.stream_hid.seed) == \
        (rs.randint(1, 2147462579), rs.randint(1, 2147462579))


def test_fit_follows_the_numpy_seed(cuda):
    runs = [small_fit(cuda, s, 2, hidden_dropout=True) for s in (21, 21, 22)]
    for pa, pb in zip(runs[0].get_params(), runs[1].get_params()):
        assert np.array_equal(bits(pa), bits(pb))
    assert runs[0].history == runs[1].history
    assert runs[0].history != runs[2].history
    assert not np.array_equal(runs[0].get_params()[0], runs[2].get_params()[0])
    # the masks alone: the same weights and orders, another seed for the streams
    Xtr, Ytr, Xdev, Ydev, init, orders = data()
    a, b = fitted(cuda, True), None
    np.random.seed(6)
    b = M.DropoutMLP(n_epochs=1, batch_size=B, regul_coefs=COEFS, init_parameters=init,
                     hidden_layer_size=48, device=cuda, hidden_dropout=True)
    b.fit(Xtr, Ytr, Xdev, Ydev, epoch_orders=orders[:1])
    assert b.stream_in.seed != a.stream_in.seed
    assert b.history[0]["train_loss"] != a.history[0]["train_loss"]


def test_evaluation_is_deterministic(cuda):
    Xtr, Ytr, Xdev, Ydev, init, orders = data()
    clf = fitted(cuda, True)
    plain = M.MLP(n_epochs=0, batch_size=B, regul_coefs=COEFS, init_parameters=clf.get_params(),
                  hidden_layer_size=48, device=cuda).fit(Xtr, Ytr, Xdev, Ydev)
    for X in (Xdev, Xtr):
        assert np.array_equal(bits(clf.predict_proba(X)), bits(plain.predict_proba(X)))
        assert np.array_equal(bits(clf.get_embedding(X)), bits(plain.get_embedding(X)))
        assert np.array_equal(clf.predict(X), plain.predict(X))
    assert clf.accuracy(Xdev, Ydev) == plain.accuracy(Xdev, Ydev) == clf.best_dev_acc
    assert clf.best_dev_loss == plain.best_dev_loss
    assert np.array_equal(bits(clf.predict_proba(Xdev)), bits(clf.predict_proba(Xdev)))


def test_epoch_runs_without_host_synchronisation(cuda, monkeypatch):
    """Both masks, across two segmentation runs, under sync debug mode 'error'."""
    Xtr, Ytr, Xdev, Ydev, init = problem(n=1500, n_train=1000, f=200, k=24, c=6)
    clf = M.DropoutMLP(n_epochs=1, batch_size=200, hidden_layer_size=24, init_parameters=init,
                       device=cuda, hidden_dropout=True)
    clf.fit(Xtr, Ytr, Xdev, Ydev)  # builds every lazy resource
    monkeypatch.setattr(M, "SEGMENT_CHUNK_ENTRIES", 3 * 200 * 20)
    clf._prepare_epoch(np.random.default_rng(2).permutation(1000))
    assert len(clf._runs) >= 2
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, acc = clf._run_batches()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert np.isfinite(float(loss)) and 0.0 <= float(acc) <= 1.0
    assert clf.stream_in.step == 10 == clf._steps_before


def test_repeated_rows_are_refused(cuda):
    Xtr, Ytr, Xdev, Ydev, init, orders = data()
    clf = M.DropoutMLP(n_epochs=1, batch_size=B, init_parameters=init, hidden_layer_size=48,
                       device=cuda)
    with pytest.raises(ValueError, match="permutation"):
        clf.fit(Xtr, Ytr, Xdev, Ydev, epoch_orders=[np.zeros(1300, np.int64)])


# -- 6. the wide pass, kernel level ----------------------------------------------------------------
SLAB = 1024


def gate_rule(t, codes):
    """g = t, t / 2, 0 for gate byte 2, 1, 0 -- exact in float32."""
    half = np.float32(0.5) * t
    return np.where(codes == 2, t, np.where(codes == 1, half, np.float32(0.0))).astype(np.float32)


def check_slab_sums(g, db, K):
    assert db.shape == (K,)
    for c0 in range(0, K, SLAB):
        c1 = min(K, c0 + SLAB)
        want = gs.column_sum(g[:, c0:c1])
        assert torch.equal(db[c0:c1].view(torch.int32), want.view(torch.int32)), (c0, c1)


@pytest.mark.parametrize("K", [1025, 1028, 2048, 2501])
@pytest.mark.parametrize("Mr", [1, 7, 513, 1030])
def test_wide_backward_is_the_rule_bit_for_bit(cuda, Mr, K):
    """M = 513 is the first with two row blocks; K = 1025 has a one-column last slab, 2048 ends on
    a slab boundary, 2501 has a ragged third slab. g against the NumPy rule, db per slab against
    sparse.column_sum of that slab of g, a second call against the first."""
    rng = np.random.default_rng(1000 * Mr + K)
    gY_host = rng.standard_normal((Mr, K)).astype(np.float32)
    codes = rng.integers(0, 3, size=(Mr, K)).astype(np.uint8)
    codes[0, :3] = (1, 2, 0)
    codes[-1, -1] = 1  # the g / 2 rule in the last slab's last column
    gY = gs.empty_dense(Mr, K, cuda)
    gY.copy_(torch.from_numpy(gY_host))
    gate = gs.empty_gate(Mr, K, cuda)
    gate.copy_(torch.from_numpy(codes))
    # the Philox words of logical rows 0 .. M + 36, every column: one evaluation for all variants
    seed, stream_id, step = 0x1234567887654321, 5, 11
    stream = D.DropoutStream(seed, stream_id, cuda)
    stream.set_step(step)
    cols = np.arange(K)
    rows_all = np.arange(Mr + 37)
    words = D.philox4x32_10((rows_all[:, None], np.arange((K + 3) // 4)[None, :], step, stream_id),
                            (seed & 0xFFFFFFFF, seed >> 32))
    word = words.reshape(Mr + 37, -1)[:, :K]  # column j: word j & 3 of the call for j >> 2
    sub = (slice(0, min(Mr, 5)), slice(K - 9, K))
    assert np.array_equal(word[37:][sub] >= np.uint32(D.dropout_threshold(0.3)),
                          stream.keep_mask(37 + rows_all[sub[0], None], cols[None, sub[1]], 0.3))

    def dropped(p, row0):
        keep = word[row0:row0 + Mr] >= np.uint32(D.dropout_threshold(p))
        assert 0 < keep.sum() < keep.size
        return np.where(keep, gY_host * np.float32(D.dropout_scale(p)), np.float32(0.0))

    # (gate, p, row0, in place, bias)
    variants = [(True, None, 0, False, True), (True, None, 0, True, False),
                (True, 0.5, 0, False, True), (True, 0.3, 37, True, True),
                (False, 0.3, 37, False, False), (False, 0.5, 0, True, True)]
    for use_gate, p, row0, in_place, bias in variants:
        t = gY_host if p is None else dropped(p, row0)
        want = gate_rule(t, codes) if use_gate else t
        for again in (False, True):
            src = gs.empty_dense(Mr, K, cuda).copy_(gY) if in_place else gY
            out = src if in_place else None
            if p is None:
                g, db = gs.relu_backward(src, gate=gate, out=out, bias_grad=bias)
            else:
                g, db = D.dropout_relu_backward(src, D.DropoutSpec(stream, p),
                                                gate=gate if use_gate else None, out=out,
                                                bias_grad=bias, row0=row0)
            tag = (use_gate, p, row0, in_place, bias, again)
            assert (g.data_ptr() == src.data_ptr()) == in_place
            assert np.array_equal(bits(g.cpu().numpy()), bits(want)), tag
            assert (db is not None) == bias
            if bias:
                check_slab_sums(g, db, K)
                if again:
                    assert torch.equal(db.view(torch.int32), first_db.view(torch.int32)), tag
                first_db = db


def test_wide_backward_stages_unpadded_inputs(cuda):
    """Rows of 1025 and 2501 floats are not 16-B aligned: a staging copy, the same bits."""
    stream = D.DropoutStream(99, 2, cuda)
    stream.set_step(3)
    spec = D.DropoutSpec(stream, 0.5)
    for Mr, K in ((7, 1025), (513, 2501)):
        gen = torch.Generator(device=cuda).manual_seed(K)
        flat = torch.randn((Mr, K), generator=gen, device=cuda)
        assert flat.stride(0) % 4 != 0
        padded = gs.empty_dense(Mr, K, cuda).copy_(flat)
        gate = gs.empty_gate(Mr, K, cuda)
        gate.copy_(torch.randint(0, 3, (Mr, K), generator=gen, device=cuda, dtype=torch.uint8))
        for run in (lambda x: gs.relu_backward(x, gate=gate),
                    lambda x: D.dropout_relu_backward(x, spec, gate=gate),
                    lambda x: D.dropout_relu_backward(x, spec)):
            (g0, db0), (g1, db1) = run(padded), run(flat)
            assert torch.equal(g0.view(torch.int32), g1.view(torch.int32))
            assert torch.equal(db0.view(torch.int32), db1.view(torch.int32))
            assert torch.equal(flat, padded)  # the inputs stay


def test_wide_backward_of_no_rows_zeroes_the_bias_gradient(cuda):
    db = torch.full((2048,), 7.0, device=cuda)
    gate = gs.empty_gate(1, 2048, cuda)
    call("gcg_rectify_backward_wide_f32", 0, 2048, None, 2048, _ptr(gate), 2048, None, 2048,
         _ptr(db), None, 0, 0, 1.0, 0, None, 0, 0, _stream_handle(cuda))
    assert not db.cpu().numpy().any()


def test_relu_backward_without_gate_keeps_its_cap(cuda):
    """Y > 0 as the mask (gcg_relu_backward_f32) stays at 1024 columns: the entry's status."""
    x = gs.empty_dense(4, 1028, cuda).fill_(1.0)
    with pytest.raises(NativeError, match="gcg_relu_backward_f32"):
        gs.relu_backward(x, x)


# -- 7. the wide pass through the layers -----------------------------------------------------------
def test_dropout_layer_on_1100_columns(cuda):
    stream = D.DropoutStream(4242, 3, cuda)
    layer = D.DropoutLayer(p=0.3, stream=stream)
    stream.advance()
    rng = np.random.default_rng(0)
    x_host = rng.standard_normal((33, 1100)).astype(np.float32)
    gy_host = rng.standard_normal((33, 1100)).astype(np.float32)
    x = torch.from_numpy(x_host).to(cuda).requires_grad_()
    y = layer(x)
    keep = stream.keep_mask(np.arange(33)[:, None], np.arange(1100)[None, :], 0.3)
    assert 0.6 < keep.mean() < 0.8
    scale = np.float32(D.dropout_scale(0.3))
    assert np.array_equal(bits(y.detach().cpu().numpy()), bits(np.where(keep, x_host * scale, 0)))
    y.backward(torch.from_numpy(gy_host).to(cuda))
    assert np.array_equal(bits(x.grad.cpu().numpy()), bits(np.where(keep, gy_host * scale, 0)))
    assert layer(x, deterministic=True) is x


@pytest.mark.parametrize("use_rows", [False, True], ids=["all_rows", "targets"])
def test_csr_matmul_output_dropout_at_1028_columns(cuda, use_rows):
    """dZ and db within test_backward_rule_gpu's 1e-5 * max(1, |ref|) of the float64 rule under
    the same mask (keyed on the output's own row and column). The bf16-gather branch rounds the
    gradient before its product, so only its db (read from the float32 gradient) is held to
    the bound; it is bitwise the float32 branch's."""
    K = 1028
    A_host = graph()
    Z_host, targets, gYs = operands(K)
    n_out = 40 if use_rows else GRAPH_N
    gY_host = gYs[n_out]
    A = gs.DeviceCSR.from_scipy(A_host, cuda)
    rows = gs.RowSelection(targets, cuda) if use_rows else None
    stream = D.DropoutStream(31337, 0, cuda)
    stream.advance()
    spec = D.DropoutSpec(stream, 0.5)
    keep = stream.keep_mask(np.arange(n_out)[:, None], np.arange(K)[None, :], 0.5)
    S = A_host.astype(np.float64)[targets] if use_rows else A_host.astype(np.float64)
    pre = S @ Z_host.astype(np.float64)  # b = 0; exact in float32: the signs are the device's
    g_ref = gY_host.astype(np.float64) * keep * 2.0 * 0.5 * (1.0 + np.sign(pre))
    db_ref, dZ_ref = g_ref.sum(axis=0), S.T @ g_ref
    assert (pre == 0).any() and keep[pre == 0].any()  # the g / 2 rule under a kept element

    def within(got, ref):
        return np.abs(got.cpu().numpy() - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())

    def run(gather_dtype):
        Z = torch.from_numpy(Z_host).to(cuda).requires_grad_()
        b = torch.zeros(K, device=cuda).requires_grad_()
        Y = layers.csr_matmul(A, Z, b, "relu", rows, dropout=spec, gather_dtype=gather_dtype)
        Y.backward(torch.from_numpy(gY_host).to(cuda))
        return Y.detach(), Z.grad, b.grad

    Y, dZ, db = run("float32")
    y_ref = np.where(keep, 2.0 * np.maximum(pre, 0.0), 0.0)
    assert np.array_equal(Y.cpu().numpy(), y_ref.astype(np.float32))
    assert within(dZ, dZ_ref) and within(db, db_ref)
    _, dZ16, db16 = run("bfloat16")
    assert torch.equal(db16, db) and within(db16, db_ref)
    assert dZ16.shape == dZ.shape and bool(torch.isfinite(dZ16).all())


# -- 8. the wide pass in the trainer ---------------------------------------------------------------
def test_trainer_with_1100_hidden_units(cuda):
    """200 rows x 50 features, B = 64 (3 steps, 8 rows dropped), both masks: the bounds of the
    trajectory test. (That the bounds can see a mask is the trajectory test's to show: over
    1100 rescaled hidden units the masks nearly average out of the loss -- the restatement
    without masks is 3.6e-4 off here, against a bound of 1.7e-4.)"""
    rng = np.random.default_rng(2)
    X = sps.random(300, 50, density=0.2, format="csr", dtype=np.float32, random_state=2)
    Y = rng.permutation(np.arange(300) % 5)
    init = (glorot_uniform(50, 1100), np.zeros(1100, np.float32), glorot_uniform(1100, 5, seed=3),
            np.zeros(5, np.float32))
    orders = [rng.permutation(200)]
    np.random.seed(8)
    clf = M.DropoutMLP(n_epochs=1, batch_size=64, regul_coefs=COEFS, init_parameters=init,
                       hidden_layer_size=1100, device=cuda, hidden_dropout=True)
    clf.fit(X[:200], Y[:200], X[200:], Y[200:], epoch_orders=orders)
    m_in, m_hid = DR.stream_masks(clf, 50, 1100, 64)
    hist, _ = DR.mlp_dropout_train(X[:200], Y[:200], X[200:], Y[200:], init, orders, 64, COEFS,
                                   m_in, m_hid)
    (got, gv), (ref, rv) = losses(clf.history), losses(hist)
    print("train_loss", got, ref, "val_loss", gv, rv)
    assert np.abs(got - ref).max() < 1e-4 * max(1.0, np.abs(ref).max()), (got, ref)
    assert np.allclose(gv, rv, rtol=1e-4, atol=1e-5)
    assert clf.stream_hid.step == 2 and clf.stream_in.step == 3  # the last batch's step; 3 done
