"""GPU tests of the mini-batch MLP trainer (graphconvgeo_amd.mlp; reference mlp.py:96-311,
tensormain.py:79-150): the epoch segmentation against scipy's X[rows].T.tocsr(), the one-pass
W1 step bit for bit against the composition of the public kernels, the training trajectory
against the float64 reference (tests/mlp_reference.py), the selection rule and the API."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import mlp_reference as R
from graphconvgeo_amd import mlp as M
from graphconvgeo_amd import sparse as gs
from graphconvgeo_amd._native import call
from graphconvgeo_amd.layers import SparseInputDenseLayer
from graphconvgeo_amd.sparse import _ptr, _stream_handle
from graphconvgeo_amd.synth import glorot_uniform, synthetic_features, synthetic_graph

pytestmark = pytest.mark.gpu


# -- 1. segmentation ---------------------------------------------------------------------------
def ragged_csr(n=257, f=97, max_nnz=12, seed=0):
    """0..max_nnz entries per row in random (unsorted) column order, duplicate (row, col)
    entries included, rows 0..7 and every 9th row empty -- kept exactly as stored."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_nnz + 1, size=n)
    lens[:8] = 0
    lens[::9] = 0
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = rng.integers(0, f, size=indptr[-1]).astype(np.int32)  # unsorted, with repeats
    for r in range(8, n, 5):  # a certain duplicate in every fifth row that has two entries
        if lens[r] >= 2:
            indices[indptr[r] + 1] = indices[indptr[r]]
    data = (rng.random(indptr[-1]) + 0.1).astype(np.float32)
    X = sps.csr_matrix((data, indices, indptr), shape=(n, f))
    assert not X.has_sorted_indices or f == 1
    return X


def check_segments(cuda, X, perm, B):
    Xd = gs.DeviceCSR.from_scipy(X, cuda)
    nb = len(perm) // B
    perm = np.asarray(perm[:nb * B], dtype=np.int32)
    nnz_sel = int(np.diff(X.indptr)[perm].sum())
    seg = M.BatchSegments(Xd, torch.from_numpy(perm).to(cuda), B, nnz_sel)
    bsp = seg.batch_seg_ptr.cpu().numpy()
    col, ptr = seg.seg_col.cpu().numpy(), seg.seg_ptr.cpu().numpy()
    pos, val = seg.ent_pos.cpu().numpy(), seg.ent_val.cpu().numpy()
    assert bsp[0] == 0 and np.all(np.diff(bsp) >= 0)
    assert ptr[bsp[nb]] == nnz_sel  # the last batch's last segment ends the entry list
    for b in range(nb):
        T = X[perm[b * B:(b + 1) * B]].T.tocsr()  # stable: batch order, then storage order
        touched = np.flatnonzero(np.diff(T.indptr))
        s0, s1 = bsp[b], bsp[b + 1]
        assert np.array_equal(col[s0:s1], touched), b
        e0 = ptr[s0]
        assert np.array_equal(ptr[s0:s1 + 1] - e0, np.append(T.indptr[touched], T.nnz)), b
        assert np.array_equal(pos[e0:e0 + T.nnz], T.indices), b
        assert np.array_equal(val[e0:e0 + T.nnz].view(np.int32), T.data.view(np.int32)), b
    return seg


def test_segmentation_matches_scipy_transpose(cuda):
    X = ragged_csr()
    order = np.random.default_rng(3).permutation(257)
    seg = check_segments(cuda, X, order, 64)  # 4 batches, one row dropped
    assert seg.n_batches == 4


@pytest.mark.parametrize("B", [1, 257])
def test_segmentation_batch_of_one_and_of_all(cuda, B):
    check_segments(cuda, ragged_csr(), np.random.default_rng(4).permutation(257), B)


def test_segmentation_single_column(cuda):
    check_segments(cuda, ragged_csr(n=130, f=1, max_nnz=3, seed=2),
                   np.random.default_rng(5).permutation(130), 32)


def test_segmentation_batches_of_empty_rows(cuda):
    X = ragged_csr()
    order = np.concatenate([np.arange(8), np.arange(8, 257)])  # batch 0: the 8 empty rows
    seg = check_segments(cuda, X, order, 8)
    bsp = seg.batch_seg_ptr.cpu().numpy()
    assert bsp[0] == bsp[1] == 0 and bsp[-1] > 0
    # and an epoch with no entry at all
    seg = check_segments(cuda, X, np.arange(8), 8)
    assert seg.nnz_sel == 0 and seg.batch_seg_ptr.cpu().tolist() == [0, 0]


def test_segment_workspace_query(cuda):
    cap, nb = C.c_int64(), C.c_size_t()
    call("gcg_minibatch_segment_sizes", 256, 64, 97, 1500, C.byref(cap), C.byref(nb))
    # the fixed arrays alone: keys in/out (4 B), payloads in/out (8 B) per entry
    assert cap.value == 4 * 97 + 1 and nb.value >= 24 * 1500


# -- 2. the W1 step, bitwise ---------------------------------------------------------------------
def hot_column_batches(F, B=512, n_batches=3, seed=0):
    """n_batches * B rows: column 5 in every row (a segment as long as the batch), 0..3 more
    entries from a set of F // 8 + 2 columns (most columns never touched), unsorted, with
    duplicates."""
    rng = np.random.default_rng(seed)
    n = n_batches * B
    few = rng.choice(F, size=F // 8 + 2, replace=False)
    lens = rng.integers(1, 5, size=n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = few[rng.integers(0, few.size, size=indptr[-1])].astype(np.int32)
    indices[indptr[:-1] + rng.integers(0, lens)] = 5
    data = rng.standard_normal(indptr[-1]).astype(np.float32)
    return sps.csr_matrix((data, indices, indptr), shape=(n, F))


def adam_a_t(t, lr=0.002, b1=0.9, b2=0.999):
    return lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)


@pytest.mark.parametrize("coefs", [(0.0, 0.0), (1e-3, 2e-3)])
@pytest.mark.parametrize("K", [1, 3, 4, 300, 301])
@pytest.mark.parametrize("F", [97, 1000])
def test_w1_step_bitwise_equals_the_composition(cuda, F, K, coefs):
    """Three consecutive steps: p, m, v bit for bit what (X[batch])^T . G (plan-less SpMM over
    scipy's transpose) + gcg_l1l2_grad_f32, then gcg_adam_step_f32 give."""
    B = 512
    X = hot_column_batches(F, B)
    Xd = gs.DeviceCSR.from_scipy(X, cuda)
    perm = np.random.default_rng(1).permutation(X.shape[0]).astype(np.int32)
    seg = M.BatchSegments(Xd, torch.from_numpy(perm).to(cuda), B, X.nnz)
    gen = torch.Generator(device=cuda).manual_seed(F * 1000 + K)
    W = torch.randn((F, K), generator=gen, device=cuda) * 0.1
    W[::7] = 0.0          # exact zeros: sgn(0) = 0
    W[3, 0] = -0.0
    m, v = torch.zeros_like(W), torch.zeros_like(W)
    Wr, mr, vr = W.clone(), m.clone(), v.clone()
    a_t = torch.zeros((), dtype=torch.float32, device=cuda)
    l1, l2 = coefs
    stream = _stream_handle(cuda)
    for t in range(3):
        if t == 1:  # a misaligned, padded G: base 4 B past a 16-B boundary
            ld = K + 5
            G = torch.empty(B * ld + 1, device=cuda)[1:].view(B, ld)[:, :K]
            assert G.data_ptr() % 16 == 4
        else:       # the trainer's layout: 16-B aligned padded rows
            G = gs.empty_dense(B, K, cuda)
        G.copy_(torch.randn((B, K), generator=gen, device=cuda))
        a_t.fill_(adam_a_t(t + 1))
        M.w1_step(W, m, v, G, seg, t, l1, l2, a_t)
        # the composition of the public kernels
        rows = perm[t * B:(t + 1) * B]
        T = gs.DeviceCSR.from_scipy(X[rows].T.tocsr(), cuda)
        assert T.max_row_nnz() >= B  # the hot column's segment is at least the whole batch
        D = torch.zeros((F, K), device=cuda)
        D.copy_(gs.spmm(T, G, mode="rowwise"))
        pen = torch.empty_like(Wr)
        call("gcg_l1l2_grad_f32", Wr.numel(), _ptr(Wr), l1, l2, None, _ptr(pen), stream)
        g = (D + pen).contiguous()
        call("gcg_adam_step_f32", Wr.numel(), _ptr(Wr), _ptr(g), _ptr(mr), _ptr(vr), _ptr(a_t),
             0.9, 0.999, 1e-8, stream)
        for got, ref, name in ((W, Wr, "p"), (m, mr, "m"), (v, vr, "v")):
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (name, t)
    assert float((W - Wr).abs().max()) == 0.0 and bool((m != 0).any())


# -- 3..7. the trainer ---------------------------------------------------------------------------
def problem(n=1800, n_train=1300, f=300, k=48, c=9, seed=0):
    """Features and labels as tests/test_mlpconv_gpu.problem: labels follow the features."""
    X = synthetic_features(n, f, nnz_per_row=20, empty_frac=0.02)
    rng = np.random.default_rng(seed)
    Y = (np.asarray(X[:, :c].argmax(axis=1)).ravel() + (rng.random(n) < 0.2)) % c
    W1, W2 = glorot_uniform(f, k), glorot_uniform(k, c, seed=3)
    init = (W1, np.zeros(k, np.float32), W2, np.zeros(c, np.float32))
    return X[:n_train], Y[:n_train], X[n_train:], Y[n_train:], init


@pytest.fixture(scope="module")
def trajectory_problem():
    Xtr, Ytr, Xdev, Ydev, init = problem()
    rng = np.random.default_rng(9)
    orders = [rng.permutation(Xtr.shape[0]) for _ in range(5)]
    return Xtr, Ytr, Xdev, Ydev, init, orders


@pytest.mark.parametrize("add_hidden", [True, False])
def test_mlp_trajectory_matches_float64_reference(cuda, trajectory_problem, add_hidden):
    """n_train = 1300, B = 400: 3 batches and 100 dropped rows per epoch, 5 epochs = 15 Adam
    steps, the same orders fed to both."""
    Xtr, Ytr, Xdev, Ydev, init, orders = trajectory_problem
    coefs = (1e-5, 1e-5)
    if not add_hidden:
        init = (glorot_uniform(300, 9, seed=5), np.zeros(9, np.float32))
    clf = M.MLP(n_epochs=5, batch_size=400, regul_coefs=coefs, init_parameters=init,
                hidden_layer_size=48, add_hidden=add_hidden, device=cuda)
    clf.fit(Xtr, Ytr, Xdev, Ydev, epoch_orders=orders)
    hist, _ = R.mlp_train(Xtr, Ytr, Xdev, Ydev, init, orders, 400, coefs, add_hidden=add_hidden)
    got = np.array([h["train_loss"] for h in clf.history])
    ref = np.array([h["train_loss"] for h in hist])
    print("train_loss", got, ref)
    assert got.shape == ref.shape == (5,)
    assert np.abs(got - ref).max() < 1e-4 * max(1.0, np.abs(ref).max()), (got, ref)
    assert ref[-1] < ref[0]  # it trains
    gv = [h["val_loss"] for h in clf.history]
    rv = [h["val_loss"] for h in hist]
    print("val_loss", gv, rv)
    assert np.allclose(gv, rv, rtol=1e-4, atol=1e-5)


def test_selection_rule_and_api(cuda):
    Xtr, Ytr, Xdev, Ydev, init = problem(n=1500, n_train=1000, f=200, k=24, c=6)
    np.random.seed(3)
    clf = M.MLP(n_epochs=8, batch_size=100, hidden_layer_size=24, regul_coefs=(1e-6, 1e-6),
                early_stopping_max_down=2, device=cuda)
    clf.fit(Xtr, Ytr, Xdev, Ydev)
    accs = [h["val_acc"] for h in clf.history]
    assert [h["epoch"] for h in clf.history] == list(range(len(accs))) and len(accs) <= 8
    best = max(accs)  # strict '>' keeps the first epoch that reaches the maximum
    assert best > 0.0
    assert clf.accuracy(Xdev, Ydev) == best == clf.best_dev_acc
    first = accs.index(best)
    assert abs(clf.best_dev_loss - clf.history[first]["val_loss"]) == 0.0
    if len(accs) < 8:  # early stopping: max_down + 1 epochs without a new best
        assert len(accs) - 1 - first == 3
    pred, proba = clf.predict(Xdev), clf.predict_proba(Xdev)
    assert pred.shape == (500,) and proba.shape == (500, 6)
    assert abs(clf.accuracy(Xdev, Ydev) - float((pred == Ydev).mean())) < 1e-6
    assert clf.score(Xdev, Ydev) == clf.accuracy(Xdev, Ydev)
    assert np.abs(proba.sum(axis=1) - 1.0).max() < 1e-5
    W1, b1, W2, b2 = clf.get_params()
    assert W1.shape == (200, 24) and b2.shape == (6,)
    layer = SparseInputDenseLayer(200, num_units=24, W=W1, b=b1, device=cuda)
    with torch.no_grad():
        want = layer(Xdev).cpu().numpy()
    emb = clf.get_embedding(Xdev)
    assert emb.shape == (500, 24) and np.array_equal(emb.view(np.int32), want.view(np.int32))
    with pytest.raises(ValueError, match="must be sparse"):
        clf.predict(Xdev.toarray())


def test_no_epoch_improves_keeps_last_parameters(cuda):
    """Labels the model cannot get right on dev (accuracy 0 every epoch): the reference would
    crash restoring None; here the last parameters stay."""
    Xtr, Ytr, Xdev, Ydev, init = problem(n=700, n_train=500, f=100, k=8, c=4)
    clf = M.MLP(n_epochs=2, batch_size=250, hidden_layer_size=8, init_parameters=init,
                device=cuda)
    clf.fit(Xtr, Ytr, Xdev[:0], Ydev[:0])  # an empty dev set: accuracy 0 / max(0, 1) = 0
    assert [h["val_acc"] for h in clf.history] == [0.0, 0.0]
    assert not np.array_equal(clf.get_params()[0], init[0])  # trained, nothing restored


def test_default_init_draws_w1_then_w2_from_the_global_stream(cuda):
    Xtr, Ytr, Xdev, Ydev, _ = problem(n=700, n_train=500, f=120, k=16, c=5)
    np.random.seed(77)
    clf = M.MLP(n_epochs=0, batch_size=100, hidden_layer_size=16, device=cuda)
    clf.fit(Xtr, Ytr, Xdev, Ydev)
    rs = np.random.RandomState(77)
    a1, a2 = np.sqrt(3) * np.sqrt(2.0 / (120 + 16)), np.sqrt(3) * np.sqrt(2.0 / (16 + 5))
    W1 = rs.uniform(-a1, a1, size=(120, 16)).astype(np.float32)
    W2 = rs.uniform(-a2, a2, size=(16, 5)).astype(np.float32)
    got = clf.get_params()
    assert np.array_equal(got[0], W1) and np.array_equal(got[2], W2)
    assert not got[1].any() and not got[3].any()


def test_fit_is_reproducible(cuda):
    Xtr, Ytr, Xdev, Ydev, _ = problem(n=1500, n_train=1000, f=200, k=24, c=6)
    runs = []
    for _ in range(2):
        np.random.seed(21)
        clf = M.MLP(n_epochs=3, batch_size=300, hidden_layer_size=24, device=cuda)
        clf.fit(Xtr, Ytr, Xdev, Ydev)
        runs.append((clf.get_params(), clf.history))
    for pa, pb in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(pa.view(np.int32), pb.view(np.int32))
    assert runs[0][1] == runs[1][1]


def test_epoch_runs_without_host_synchronisation(cuda, monkeypatch):
    """Every batch of an epoch, across two segmentation runs, under sync debug mode 'error'."""
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    Xtr, Ytr, Xdev, Ydev, init = problem(n=1500, n_train=1000, f=200, k=24, c=6)
    clf = M.MLP(n_epochs=1, batch_size=200, hidden_layer_size=24, init_parameters=init,
                device=cuda)
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


def test_main_justinputconv_call_pattern(cuda):
    """The constructor / fit / accuracy / predict calls of tensormain.py:141-149 on
    X_conv = H * X sliced as tensormain.py:116-118, with the import swapped."""
    n, n_tr, n_dev, C_ = 2500, 1500, 500, 6
    H = synthetic_graph(n, 15000)
    X = synthetic_features(n, 200, nnz_per_row=20, empty_frac=0.02)
    rng = np.random.default_rng(0)
    Y = (np.asarray(X[:, :C_].argmax(axis=1)).ravel() + (rng.random(n) < 0.2)) % C_
    X_conv = M.input_convolution(H, X)
    ref = (H @ X).tocsr()
    ref.sort_indices()
    parts = [(0, n_tr), (n_tr, n_tr + n_dev), (n_tr + n_dev, n)]
    X_train, X_dev, X_test = (X_conv.row_slice(a, b) for a, b in parts)
    for got, (a, b) in zip((X_train, X_dev, X_test), parts):
        want, g = ref[a:b], got.to_scipy()
        assert g.shape == want.shape
        assert np.array_equal(g.indptr, want.indptr) and np.array_equal(g.indices, want.indices)
        assert np.array_equal(g.data.view(np.int32), want.data.view(np.int32))
    Y_train, Y_dev, Y_test = (Y[a:b] for a, b in parts)
    regul, batch_size, hidden_size = 1e-6, 500, 24
    np.random.seed(77)
    clf = M.MLP(n_epochs=30, batch_size=batch_size, init_parameters=None, complete_prob=False,
                add_hidden=True, regul_coefs=[regul, regul], save_results=False,
                hidden_layer_size=hidden_size, drop_out=False, drop_out_coefs=[0.5, 0.5],
                early_stopping_max_down=5, loss_name='log', nonlinearity='rectify')
    clf.fit(X_train, Y_train, X_dev, Y_dev)
    acc = clf.accuracy(X_test, Y_test)
    y_pred = clf.predict(X_test)
    assert y_pred.shape == (n - n_tr - n_dev,) and abs(acc - (y_pred == Y_test).mean()) < 1e-6
    assert acc > 1.5 / C_
    assert 0.0 <= clf.accuracy(X_dev, Y_dev) <= 1.0 and clf.predict(X_dev).shape == (n_dev,)
