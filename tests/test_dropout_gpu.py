"""Dropout on the GPU against the NumPy statement of the mask rule (graphconvgeo_amd.dropout):
the three kernels bit for bit, the layer against the oracle SpMM and a float64 restatement
with the same masks, and MLPCONV(drop_out=True) eager and as a captured HIP graph."""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

from graphconvgeo_amd import dropout as D
from graphconvgeo_amd import sparse as gs
from graphconvgeo_amd.mlpconv import MLPCONV
from graphconvgeo_amd.synth import glorot_uniform, synthetic_features, synthetic_graph
from oracle import gcn_oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
SHAPES = [(1, 1, 1), (3, 5, 5), (7, 300, 304), (65, 301, 304), (65, 301, 301),
          (130, 1024, 1024), (33, 1027, 1028)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def drop_ref(x, rows, cols, p, stream, step, rescale=True):
    """keep ? fl32(x * scale) : +0.0 with the NumPy mask."""
    keep = D.keep_mask_reference(rows, cols, p, stream.seed, step, stream.stream_id)
    scale = np.float32(D.dropout_scale(p, rescale))
    with np.errstate(invalid="ignore"):
        return np.where(keep, np.asarray(x, np.float32) * scale, np.float32(0.0)), keep


def padded(M, K, ld, dev, values=None):
    buf = torch.full((M, ld), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[:, :K]
    if values is not None:
        view.copy_(torch.from_numpy(values))
    return buf, view


def padding_untouched(buf, K):
    return bool((buf[:, K:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------
# 5. gcg_dropout_f32
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,ld", SHAPES)
@pytest.mark.parametrize("p", [0.4, 0.5, 0.999])
def test_dropout_dense_bitwise(cuda, M, K, ld, p):
    rng = np.random.default_rng(M * 1000 + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    stream = D.DropoutStream(2 ** 40 + 5, 3, cuda)
    spec = D.DropoutSpec(stream, p)
    perm = rng.permutation(K).astype(np.int32) * 3 + 1  # scattered logical columns
    perm_dev = torch.from_numpy(perm).to(cuda)
    r = np.arange(M)[:, None]
    for row0, step in ((0, 0), (1000, 7)):
        stream.set_step(step)
        for cols, col_ids in ((np.arange(K)[None, :], None), (perm[None, :], perm_dev)):
            want, _ = drop_ref(x, row0 + r, cols, p, stream, step)
            xb, xv = padded(M, K, ld, cuda, x)
            yb, yv = padded(M, K, ld, cuda)
            D.dropout_dense(xv, spec, out=yv, row0=row0, col_ids=col_ids)
            assert np.array_equal(bits(yv.cpu().numpy()), bits(want)), (row0, step)
            assert padding_untouched(yb, K) and padding_untouched(xb, K)
            assert np.array_equal(xv.cpu().numpy(), x)  # out of place: the input is left alone
            D.dropout_dense(xv, spec, out=xv, row0=row0, col_ids=col_ids)  # in place
            assert np.array_equal(bits(xv.cpu().numpy()), bits(want))
            assert padding_untouched(xb, K)


def test_dropout_dense_nan_and_row_slices(cuda):
    M, K = 65, 301
    rng = np.random.default_rng(3)
    x = rng.standard_normal((M, K)).astype(np.float32)
    x[::3, ::5] = np.nan
    x[1::3, 1::7] = np.inf
    stream = D.DropoutStream(77, 1, cuda)
    stream.set_step(2)
    spec = D.DropoutSpec(stream, 0.5)
    want, keep = drop_ref(x, np.arange(M)[:, None], np.arange(K)[None, :], 0.5, stream, 2)
    _, xv = padded(M, K, 304, cuda, x)
    got = D.dropout_dense(xv, spec).cpu().numpy()
    dropped = ~keep
    assert (dropped & ~np.isfinite(x)).any() and (keep & np.isnan(x)).any()
    assert (bits(got)[dropped] == 0).all()  # +0.0, whatever lay under a dropped slot
    assert np.isnan(got[keep & np.isnan(x)]).all()
    ok = ~np.isnan(want)
    assert np.array_equal(bits(got)[ok], bits(want)[ok])
    # rows [a, b) with row0 = a are the slice of the full run (any row partition, one mask)
    a, b = 17, 49
    part = D.dropout_dense(xv[a:b], spec, row0=a).cpu().numpy()
    assert np.array_equal(bits(part)[ok[a:b]], bits(got[a:b])[ok[a:b]])
    # rescale off: kept values pass unscaled
    plain = D.dropout_dense(xv, D.DropoutSpec(stream, 0.5, rescale=False)).cpu().numpy()
    fin = keep & np.isfinite(x)
    assert np.array_equal(plain[fin], x[fin]) and (bits(plain)[dropped] == 0).all()


# ---------------------------------------------------------------------------------------
# 6. gcg_dropout_relu_backward_f32
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,ld", [s for s in SHAPES if s[1] <= 1024]
                         + [(513, 300, 304), (2049, 20, 20)])
@pytest.mark.parametrize("p", [0.4, 0.5])
def test_dropout_relu_backward_bitwise(cuda, M, K, ld, p):
    rng = np.random.default_rng(M * 7 + K)
    gy = rng.standard_normal((M, K)).astype(np.float32)
    gate = rng.integers(0, 3, size=(M, K)).astype(np.uint8)
    if M * K >= 3:
        gate.reshape(-1)[:3] = (0, 1, 2)
        assert set(np.unique(gate)) == {0, 1, 2}
    stream = D.DropoutStream(77, 1, cuda)
    row0, step = 1000, 7
    stream.set_step(step)
    spec = D.DropoutSpec(stream, p)
    t, _ = drop_ref(gy, row0 + np.arange(M)[:, None], np.arange(K)[None, :], p, stream, step)
    g_ref = np.where(gate == 2, t, np.where(gate == 1, np.float32(0.5) * t, np.float32(0.0)))
    gate_dev = gs.empty_gate(M, K, cuda)
    gate_dev.copy_(torch.from_numpy(gate))
    # K > 256 runs on dwordx4 only: unpadded rows are staged by the wrapper, as
    # sparse.relu_backward stages them, and the caller's out / alias buffers are padded ones
    ld_io = ld if (K <= 256 or ld % 4 == 0) else (K + 3) // 4 * 4
    _, gv_in = padded(M, K, ld, cuda, gy)
    gb, gv = padded(M, K, ld_io, cuda, gy)
    ob, ov = padded(M, K, ld_io, cuda)
    g, db = D.dropout_relu_backward(gv_in, spec, gate=gate_dev, out=ov, row0=row0)
    assert g is ov and padding_untouched(ob, K)
    assert np.array_equal(bits(g.cpu().numpy()), bits(g_ref))
    # the existing gate kernel on the pre-masked gradient: same g, same bias gradient bits
    _, tv = padded(M, K, ld, cuda, t)
    g2, db2 = gs.relu_backward(tv, gate=gate_dev)
    assert np.array_equal(bits(g2.cpu().numpy()), bits(g.cpu().numpy()))
    assert np.array_equal(bits(db2.cpu().numpy()), bits(db.cpu().numpy()))
    # twice: identical bits
    g3, db3 = D.dropout_relu_backward(gv, spec, gate=gate_dev, row0=row0)
    assert torch.equal(g3, g) and torch.equal(db3, db)
    # no gate: g = t, the bias gradient its column sums
    g4, db4 = D.dropout_relu_backward(gv, spec, gate=None, row0=row0)
    assert np.array_equal(bits(g4.cpu().numpy()), bits(t))
    assert np.array_equal(bits(db4.cpu().numpy()), bits(gs.column_sum(tv).cpu().numpy()))
    # g_out aliasing gY
    g5, db5 = D.dropout_relu_backward(gv, spec, gate=gate_dev, out=gv, row0=row0)
    assert g5 is gv and torch.equal(g5, g) and torch.equal(db5, db)
    assert padding_untouched(gb, K)


# ---------------------------------------------------------------------------------------
# 7. gcg_csr_dropout_f32
# ---------------------------------------------------------------------------------------
def ragged_csr():
    """300 x 40: empty first and last rows, a run of empty rows, unsorted indices, a duplicated
    entry, and one row of 5,000 stored entries (more than two 2,048-entry work slices)."""
    rng = np.random.default_rng(11)
    lens = rng.integers(1, 9, size=300)
    lens[0] = lens[-1] = 0
    lens[10:20] = 0
    lens[5] = 5000
    indptr = np.zeros(301, np.int32)
    np.cumsum(lens, out=indptr[1:])
    indices = np.concatenate([rng.permutation(40)[:n] if n <= 40 else rng.integers(0, 40, size=n)
                              for n in lens]).astype(np.int32)
    s = indptr[30]
    assert lens[30] >= 1
    if lens[30] == 1:
        s = indptr[np.argmax(lens[30:100] >= 2) + 30]
    indices[s + 1] = indices[s]  # one (i, j) stored twice
    # small integers: sums of duplicates are exact in any order (scipy adds them to compare)
    data = rng.integers(1, 9, size=indices.size).astype(np.float32) * rng.choice([-1, 1], indices.size)
    return sps.csr_matrix((data, indices, indptr), shape=(300, 40))


def test_csr_dropout_bitwise_and_transposed_twin(cuda):
    m = ragged_csr()
    assert not m.has_sorted_indices
    X = gs.DeviceCSR.from_scipy(m, cuda)
    stream = D.DropoutStream(2 ** 40 + 5, 0, cuda)
    stream.set_step(3)
    rows = np.repeat(np.arange(300), np.diff(m.indptr))
    view = X.dropout_view(stream)
    want, keep = drop_ref(m.data, rows, m.indices, 0.4, stream, 3)
    view.refresh(D.DropoutSpec(stream, 0.4))  # a scale that rounds
    assert np.array_equal(bits(view.data.cpu().numpy()), bits(want))
    assert 0.5 < keep.mean() < 0.7
    spec = D.DropoutSpec(stream, 0.5)
    want, keep = drop_ref(m.data, rows, m.indices, 0.5, stream, 3)
    assert X.dropout_view(stream) is view and view.refresh(spec) is view
    assert view.indptr is X.indptr and view.indices is X.indices and view._plans is X._plans
    assert np.array_equal(bits(view.data.cpu().numpy()), bits(want))
    assert np.array_equal(X.data.cpu().numpy(), m.data)  # the base keeps its values
    # in place through the raw entry point
    vals = X.data.clone()
    D.csr_dropout(X, vals, vals, spec)
    assert np.array_equal(bits(vals.cpu().numpy()), bits(want))
    # the transposed twin, on the structure of the existing device transpose
    T = view.transpose()
    assert T.indices is X.transpose().indices and T.transpose() is view
    tm = T.to_scipy()
    t_rows = np.repeat(np.arange(40), np.diff(tm.indptr))
    t_want, _ = drop_ref(X.transpose().data.cpu().numpy(), tm.indices, t_rows, 0.5, stream, 3)
    assert np.array_equal(bits(tm.data), bits(t_want))
    assert (view.to_scipy() != tm.T).nnz == 0
    # a later step rewrites X and the twin it already has
    stream.set_step(4)
    view.refresh(spec)
    assert (view.to_scipy() != view.transpose().to_scipy().T).nnz == 0
    assert (view.to_scipy() != sps.csr_matrix((want, m.indices, m.indptr), shape=m.shape)).nnz


def test_csr_dropout_empty(cuda):
    X = gs.DeviceCSR.from_scipy(sps.csr_matrix((5, 4), dtype=np.float32), cuda)
    stream = D.DropoutStream(1, 0, cuda)
    view = X.dropout_view(stream).refresh(D.DropoutSpec(stream, 0.5))
    assert view.nnz == 0 and view.transpose().nnz == 0


# ---------------------------------------------------------------------------------------
# 8. the layers, 9. the trainer: a float64 restatement with the same masks
# ---------------------------------------------------------------------------------------
def masks_f64(clf, X, n, k, step):
    """(scale * keep) of X's stored entries and of the hidden layer, for one step."""
    p_hid, p_in = clf.dropout_coefs
    s_in, s_hid = clf.dropout_streams
    X = sps.csr_matrix(X)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    m_in = D.keep_mask_reference(rows, X.indices, p_in, s_in.seed, step, s_in.stream_id)
    m_hid = D.keep_mask_reference(np.arange(n)[:, None], np.arange(k)[None, :], p_hid,
                                  s_hid.seed, step, s_hid.stream_id)
    return (m_in * np.float64(D.dropout_scale(p_in)), m_hid * np.float64(D.dropout_scale(p_hid)))


def step_f64(X, H, prm, idx, y, coefs, m_in, m_hid):
    """Loss and gradients of the dropout model in float64 (Theano's rules, as
    oracle.gcn_backward, with the masks as constants)."""
    c_out, c_hid = coefs
    X = sps.csr_matrix(X)
    Xd = sps.csr_matrix((X.data.astype(np.float64) * m_in, X.indices, X.indptr), shape=X.shape)
    Hd = sps.csr_matrix(H, dtype=np.float64)
    W1, b1, W2, b2 = (prm[k].astype(np.float64) for k in ("W1", "b1", "W2", "b2"))
    pre1 = Hd @ (Xd @ W1) + b1
    h = O.relu(pre1) * m_hid
    pre2 = Hd @ (h @ W2) + b2
    logits = pre2[idx]
    P = O.softmax(logits)
    loss = O.gcn_loss(P, y, W1, W2, coefs)
    acc = float((logits.argmax(axis=1) == y).mean())
    G = P.copy()
    G[np.arange(idx.size), y] -= 1.0
    G /= idx.size
    g_pre2 = np.zeros_like(pre2)
    np.add.at(g_pre2, idx, G)
    g_Z2 = Hd.T @ g_pre2
    g_W2 = h.T @ g_Z2 + c_out * 0.5 * np.sign(W2) + c_out * W2
    g_pre1 = (g_Z2 @ W2.T) * m_hid * 0.5 * (1.0 + np.sign(pre1))
    g_W1 = Xd.T @ (Hd.T @ g_pre1) + c_hid * 0.5 * np.sign(W1) + c_hid * W1
    return loss, acc, {"W1": g_W1, "b1": g_pre1.sum(axis=0), "W2": g_W2, "b2": g_pre2.sum(axis=0)}


def small_problem(n=200, f=60, k=20, c=7, seed=0):
    H = synthetic_graph(n, 6 * n)
    rng = np.random.default_rng(seed)
    X = synthetic_features(n, f, nnz_per_row=6, empty_frac=0.02).tolil()
    X[:, :5] = rng.random((n, 5)) * (rng.random((n, 5)) < 0.6)  # a dense Zipf head
    X = sps.csr_matrix(X.tocsr(), dtype=np.float32)
    X.eliminate_zeros()
    Y = rng.integers(0, c, size=n)
    Y[:c] = np.arange(c)
    n_tr = int(0.6 * n)
    train = np.random.default_rng(77).choice(n_tr, size=n_tr).astype(np.int32)
    dev_i = np.arange(n_tr, n_tr + n // 5, dtype=np.int32)
    test_i = np.arange(n_tr + n // 5, n, dtype=np.int32)
    init = (glorot_uniform(f, k), np.full(k, 0.01, np.float32), glorot_uniform(k, c, seed=3),
            np.zeros(c, np.float32))
    return H, X, Y, train, dev_i, test_i, init


@pytest.mark.parametrize("path", ["gather", "split"])
def test_layers_against_restatement(cuda, monkeypatch, path):
    n, f, k, c = 200, 60, 20, 7
    H, X, Y, train, dev_i, test_i, init = small_problem(n, f, k, c)
    coefs = (1e-5, 1e-5)
    mode = "ordered"
    if path == "split":  # X^T . g through the dense head GEMM + the tail's transposed twin
        monkeypatch.setattr(gs, "HYBRID_MIN_ROWS", 100)
        monkeypatch.setattr(gs, "HYBRID_MIN_DENSITY", 0.3)
        monkeypatch.setattr(gs, "HYBRID_MAX_COLS", 8)
        mode = "fast"
    clf = MLPCONV(n_epochs=0, hidden_layer_size=k, regul_coefs=coefs, init_parameters=init,
                  device=cuda, mode=mode, drop_out=True, dropout_coefs=[0.5, 0.4], seed=5,
                  order="reference")
    clf.fit(X, train, dev_i, test_i, Y, H)
    assert [s.seed for s in clf.dropout_streams] == \
        list(np.random.RandomState(5).randint(1, 2147462579, size=2))
    step = 4
    for s in clf.dropout_streams:
        s.set_step(step)
    m_in, m_hid = masks_f64(clf, X, n, k, step)
    W1, b1, W2, b2 = init
    h = clf._hidden(deterministic=False).detach().cpu().numpy()
    if path == "gather":  # ordered SpMMs: bitwise the oracle's, then the mask
        Xs = sps.csr_matrix(X)
        x_drop = np.where(m_in > 0, Xs.data * np.float32(D.dropout_scale(0.4)), np.float32(0))
        Xdrop = sps.csr_matrix((x_drop.astype(np.float32), Xs.indices, Xs.indptr), shape=X.shape)
        a = O.spmm_f32(H, O.spmm_f32(Xdrop, W1), bias=b1, act="relu")
        want = np.where(m_hid > 0, a * np.float32(D.dropout_scale(0.5)), np.float32(0))
        assert np.array_equal(bits(h), bits(want))
        assert (h == 0).mean() > 0.4
    y = Y[train]
    loss, acc = clf._loss_acc(clf.rows["train"], torch.as_tensor(y.astype(np.int32), device=cuda),
                              deterministic=False)
    loss.backward()
    prm = dict(zip(("W1", "b1", "W2", "b2"), init))
    loss64, _acc64, g64 = step_f64(X, H, prm, train, y, coefs, m_in, m_hid)
    assert abs(float(loss.detach()) - loss64) <= 1e-5 * max(1.0, abs(loss64))
    for p, name in zip(clf.params, ("W1", "b1", "W2", "b2")):
        err = np.abs(p.grad.cpu().numpy() - g64[name]).max()
        assert err <= 1e-5 * max(1.0, np.abs(g64[name]).max()), (name, err)
    view = clf.Xd.dropout_view(clf.l_in_drop.stream)
    if path == "split":
        cols, head, tail_t = view._dense_column_split()
        assert 0 < cols.numel() <= 8 and tail_t.nnz > 0
        # head + tail put together are the dropped X, transposed
        Xt = view.to_scipy().T.toarray()
        got = tail_t.to_scipy().toarray()
        got[cols.cpu().numpy()] += head.cpu().numpy().T
        assert np.array_equal(got, Xt)
    else:
        assert "_dense_split" not in view.__dict__ and view._t is not None
    # deterministic: bitwise the layer without dropout
    plain = MLPCONV(n_epochs=0, hidden_layer_size=k, regul_coefs=coefs, init_parameters=init,
                    device=cuda, mode=mode, order="reference").fit(X, train, dev_i, test_i, Y, H)
    with torch.no_grad():
        assert torch.equal(clf._hidden(deterministic=True), plain._hidden())
        assert torch.equal(clf.l_hid1(clf.Xd, deterministic=True), plain.l_hid1(plain.Xd))


def test_dense_dropout_layer_autograd(cuda):
    stream = D.DropoutStream(9, 2, cuda)
    layer = D.dropout(p=0.5, stream=stream)
    stream.set_step(1)
    x = torch.randn(37, 50, device=cuda, requires_grad=True)
    y = layer(x)
    y.backward(torch.ones_like(y))
    keep = stream.keep_mask(np.arange(37)[:, None], np.arange(50)[None, :], 0.5, step=1)
    assert np.array_equal(y.detach().cpu().numpy(), np.where(keep, x.detach().cpu().numpy() * 2, 0))
    assert np.array_equal(x.grad.cpu().numpy(), np.where(keep, 2.0, 0.0).astype(np.float32))
    assert layer(x, deterministic=True) is x
    with pytest.raises(ValueError, match="must be sparse"):
        D.SparseInputDropoutLayer(p=0.5, stream=stream)(x)


@pytest.mark.parametrize("order", ["reference", "propagate_first"])
def test_mlpconv_dropout_trajectory(cuda, order):
    n, f, k, c = 1500, 120, 24, 6
    H = synthetic_graph(n, 9000)
    X = synthetic_features(n, f, nnz_per_row=12, empty_frac=0.02)
    rng = np.random.default_rng(0)
    Y = (np.asarray(X[:, :c].argmax(axis=1)).ravel() + (rng.random(n) < 0.2)) % c
    n_tr = int(0.6 * n)
    train = np.random.default_rng(77).choice(n_tr, size=n_tr).astype(np.int32)
    dev_i = np.arange(n_tr, n_tr + n // 5, dtype=np.int32)
    test_i = np.arange(n_tr + n // 5, n, dtype=np.int32)
    init = (glorot_uniform(f, k), np.zeros(k, np.float32), glorot_uniform(k, c, seed=3),
            np.zeros(c, np.float32))
    coefs = (1e-5, 1e-5)
    kw = dict(n_epochs=11, hidden_layer_size=k, regul_coefs=coefs, init_parameters=init,
              device=cuda, report_k_epoch=5, order=order)

    def fit(**extra):
        return MLPCONV(**{**kw, **extra}).fit(X, train, dev_i, test_i, Y, H)

    a = fit(drop_out=True, dropout_coefs=[0.5, 0.5], seed=5)
    # the float64 restatement with the same masks (step n in epoch n)
    prm = {key: v.astype(np.float64) for key, v in zip(("W1", "b1", "W2", "b2"), init)}
    state, ref = {}, []
    for epoch in range(11):
        m_in, m_hid = masks_f64(a, X, n, k, epoch)
        loss, _acc, g = step_f64(X, H, prm, train, Y[train], coefs, m_in, m_hid)
        ref.append(loss)
        prm = O.adam_step(prm, g, state)
    got = np.array([h["train_loss"] for h in a.history])
    ref = np.array(ref)
    assert np.abs(got - ref).max() < 1e-4 * max(1.0, np.abs(ref).max()), (got, ref)
    # a captured HIP graph: a fresh mask per replay, the eager trajectory bit for bit
    b = fit(drop_out=True, dropout_coefs=[0.5, 0.5], seed=5, use_graph=True)
    assert a.history == b.history
    for pa, pb in zip(a.get_params(), b.get_params()):
        assert np.array_equal(pa, pb)
    # the seed decides the masks
    assert fit(drop_out=True, dropout_coefs=[0.5, 0.5], seed=5).history == a.history
    other = fit(drop_out=True, dropout_coefs=[0.5, 0.5], seed=6)
    assert [h["train_loss"] for h in other.history] != [h["train_loss"] for h in a.history]
    # prediction is deterministic: the drop_out=False model with the same parameters
    p1, p2 = a.predict_proba("test"), a.predict_proba("test")
    assert np.array_equal(p1, p2)
    plain = fit(n_epochs=0, init_parameters=a.get_params())
    assert np.array_equal(plain.predict_proba("test"), p1)
    assert plain.accuracy("test", Y[test_i]) == a.accuracy("test", Y[test_i])
    # dropout_coefs = [0, 0] launches nothing: the drop_out=False trajectory
    zero, off = fit(drop_out=True, dropout_coefs=[0, 0], seed=5), fit()
    assert zero.history == off.history
    for pa, pb in zip(zero.get_params(), off.get_params()):
        assert np.array_equal(pa, pb)


def test_dropout_refuses_torch_compile(cuda, monkeypatch):
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    stream = D.DropoutStream(1, 0, cuda)
    with pytest.raises(NotImplementedError, match="torch.compile"):
        D.DropoutLayer(p=0.5, stream=stream)(torch.zeros(2, 2, device=cuda))
