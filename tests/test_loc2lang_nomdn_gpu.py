"""loc2lang's no-MDN baseline on the GPU (graphconvgeo_amd.loc2lang.NNModel_loc2lang_nomdn,
reference loc2lang.py:167-171 with nomdn=True): the one-pass Adamax step of the sparse first
layer bit for bit against the composition of the public kernels, the training trajectory against
the float64 trainer restated here, the analyses on scipy and device inputs and in two chunk
sizes, and one run from coordinates through the grid to a fit.

The restated trainer (train, predict, first_layer) and its problems (nomdn_problem) are plain
NumPy and carry no GPU mark: tests/test_grid_reference.py runs them in float32 against float64.
"""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

import grid_reference as GR
import loc2lang_reference as R
from mdn_reference import batches_of

gpu = pytest.mark.gpu


# -- the trainer, restated ---------------------------------------------------------------------
def names(hid):
    return ["Wg", "bg"] + (["Wh", "bh"] if hid else []) + ["Wo", "bo"]


def first_layer(X, p):
    """rectify(X.Wg + bg): X a dense array or a scipy CSR (its product gives a dense array)."""
    return np.maximum(np.asarray(X @ p["Wg"]) + p["bg"], 0)


def forward(X, p):
    """(G, H, Z) of loc2lang.py:164-187 with nomdn=True, up to the softmax."""
    G = first_layer(X, p)
    H = np.maximum(G @ p["Wh"] + p["bh"], 0) if "Wh" in p else G
    return G, H, H @ p["Wo"] + p["bo"]


def predict(X, params, dtype=np.float64):
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    X = X.astype(dtype) if sps.issparse(X) else np.asarray(X, dtype=dtype)
    return torch.softmax(torch.from_numpy(forward(X, p)[2]), dim=1).numpy()


def train(X_train, Y_train, X_dev, Y_dev, init, orders, batch, dtype=torch.float64):
    """loc2lang_reference.train for the no-MDN network, the gradients written out: (history,
    params) with per epoch the batch losses (each before its update) and the dev loss over every
    dev row; the final parameters in `dtype`'s NumPy type. The rectify passes no gradient at 0.
    The loss with its logits gradient is loc2lang_reference.soft_xent_and_grad, the update
    loc2lang_reference.adamax_step."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    keys = names(len(init) == 6)

    def inputs(X):
        return sps.csr_matrix(X).astype(npdt) if sps.issparse(X) else np.asarray(X, dtype=npdt)

    Xt, Xd = inputs(X_train), inputs(X_dev)
    Yt = np.asarray(sps.csr_matrix(Y_train).todense(), dtype=npdt)
    Yd = np.asarray(sps.csr_matrix(Y_dev).todense(), dtype=npdt)
    params = {k: np.asarray(v, dtype=npdt) for k, v in zip(keys, init)}
    state, hist = {}, []
    for n, order in enumerate(orders):
        losses = []
        for rows in batches_of(order, batch):
            xb, p = Xt[rows], params
            G, H, Z = forward(xb, p)
            loss_rows, dZ = R.soft_xent_and_grad(Z, Yt[rows], dtype, scale=1.0 / len(rows))
            dZ = dZ.astype(npdt)
            losses.append(float(loss_rows.mean()))
            grads = {"Wo": H.T @ dZ, "bo": dZ.sum(axis=0)}
            dH = dZ @ p["Wo"].T
            if "Wh" in p:
                g = dH * (H > 0)
                grads.update(Wh=G.T @ g, bh=g.sum(axis=0))
                dH = g @ p["Wh"].T
            gG = dH * (G > 0)
            grads.update(Wg=np.asarray(xb.T @ gG), bg=gG.sum(axis=0))
            params = R.adamax_step(params, grads, state)
            params = {k: v.astype(npdt) for k, v in params.items()}
        l_val = R.soft_xent_and_grad(forward(Xd, params)[2], Yd, dtype)[0].mean()
        hist.append({"epoch": n, "batch_losses": losses, "train_loss": float(np.mean(losses)),
                     "val_loss": float(l_val)})
    return hist, params


GRID = dict(grid_size=2.0, bbox=GR.US_BBOX, radius_km=400.0)
N_UNITS = 6


def nomdn_problem(kind, hid, seed=3):
    """The sizes of loc2lang_reference.parity_problem (n = 96, dev 40, B = 32, V = 37, 8 fixed
    epoch orders) and its targets. kind "dense": its coordinates as the [n, 2] input. kind "grid":
    136 coordinates around five US cities (sigma 1.5 degrees; rows 5 and 50 far out at sea: empty
    rows) as rows over the US grid at 2 degrees, radius 400 km -- 13 x 29 = 377 columns, a good
    part of them touched by no training row. Returns (X_train, Y_train, X_dev, Y_dev, init,
    orders, B, coords)."""
    Xtr, Ytr, Xdev, Ydev, _init, orders, B = R.parity_problem(hid=hid)
    rng = np.random.default_rng(seed)
    V, C = Ytr.shape[1], N_UNITS
    coords = np.concatenate([Xtr, Xdev])
    if kind == "grid":
        cities = np.array([[40.7, -74.0], [34.1, -118.2], [41.9, -87.6], [29.8, -95.4],
                           [47.6, -122.3]])
        coords = cities[rng.integers(0, 5, size=136)] + 1.5 * rng.standard_normal((136, 2))
        coords[[5, 50]] = [[20.0, -60.0], [55.0, -140.0]]
        X = GR.grid_representation(coords, **GRID)
        Xtr, Xdev = X[:96], X[96:]
    F = Xtr.shape[1]

    def glorot(a, b):
        lim = np.sqrt(6.0 / (a + b))
        return rng.uniform(-lim, lim, size=(a, b)).astype(np.float32)

    init = [glorot(F, C), (0.1 * rng.random(C)).astype(np.float32)]
    if hid:
        init += [glorot(C, hid), np.zeros(hid, np.float32)]
    init += [glorot(hid or C, V), np.zeros(V, np.float32)]
    return Xtr, Ytr, Xdev, Ydev, init, orders, B, coords


def within_trajectory_bound(hist, params, ref_hist, ref_params, label=""):
    """Every batch loss and dev loss within 1e-4 max(1, |ref|), every final parameter within
    rtol 1e-4, atol 1e-5: tests/test_loc2lang_gpu.py's bounds for the Gaussian model."""
    got_b = np.array([h["batch_losses"] for h in hist])
    ref_b = np.array([h["batch_losses"] for h in ref_hist])
    got_v = np.array([h["val_loss"] for h in hist])
    ref_v = np.array([h["val_loss"] for h in ref_hist])
    print(label, "batch", np.abs(got_b - ref_b).max(), "dev", np.abs(got_v - ref_v).max())
    assert got_b.shape == ref_b.shape == (8, 3)
    assert np.all(np.abs(got_b - ref_b) <= 1e-4 * np.maximum(1.0, np.abs(ref_b)))
    assert np.all(np.abs(got_v - ref_v) <= 1e-4 * np.maximum(1.0, np.abs(ref_v)))
    for name, ref in ref_params.items():
        got = params[name]
        print(label, name, "deviation", np.abs(got - ref).max())
        assert got.shape == ref.shape
        assert np.allclose(got, ref, rtol=1e-4, atol=1e-5), name


# -- 1. the one-pass Adamax step, bitwise --------------------------------------------------------
ONLY_FIRST = (11, 12, 13)


def batch_rows(F, B=32, n_batches=3, seed=0):
    """(X, perm): n_batches * B rows of about 6 entries and the epoch's order. Columns 0-3 and
    every fifth are never touched, column 7 is in every second row (hit by several rows of a
    batch), columns ONLY_FIRST are in rows of the first batch alone (their m is non-zero and
    their gradient zero from the second step on); unsorted, with duplicates."""
    rng = np.random.default_rng(seed)
    n = n_batches * B
    perm = rng.permutation(n).astype(np.int32)
    allowed = np.array([c for c in range(4, F) if c % 5 and c not in ONLY_FIRST])
    lens = rng.integers(4, 9, size=n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = allowed[rng.integers(0, allowed.size, size=indptr[-1])].astype(np.int32)
    indices[indptr[:-1][::2]] = 7
    first = perm[:B]
    indices[indptr[first] + 1] = np.resize(ONLY_FIRST, B)
    data = rng.standard_normal(indptr[-1]).astype(np.float32)
    return sps.csr_matrix((data, indices, indptr), shape=(n, F)), perm


@gpu
@pytest.mark.parametrize("K", [5, 68, 300])
def test_w1_adamax_step_bitwise_equals_the_composition(cuda, K):
    """Three consecutive steps on F = 37 rows (not a multiple of the kernel's 8 per workgroup):
    p, m, u bit for bit what (X[batch])^T . G (plan-less SpMM over scipy's transpose: the
    segments' entry order, product and sum rounded separately) and gcg_adamax_step_f32 give; from
    the second step on, rows with a non-zero m and a zero gradient move too. The Adam entry on the
    same inputs stays bitwise its own composition (gcg_l1l2_grad_f32, gcg_adam_step_f32)."""
    from graphconvgeo_amd import mlp as M
    from graphconvgeo_amd import sparse as gs
    from graphconvgeo_amd._native import call
    from graphconvgeo_amd.sparse import _ptr, _stream_handle
    F, B = 37, 32
    X, perm = batch_rows(F, B)
    Xd = gs.DeviceCSR.from_scipy(X, cuda)
    seg = M.BatchSegments(Xd, torch.from_numpy(perm).to(cuda), B, X.nnz)
    gen = torch.Generator(device=cuda).manual_seed(1000 + K)
    W = torch.randn((F, K), generator=gen, device=cuda) * 0.1
    W[3, 0] = -0.0
    state = {r: [W.clone(), torch.zeros_like(W), torch.zeros_like(W)]
             for r in ("adamax", "adamax_ref", "adam", "adam_ref")}
    a_t = torch.zeros((), dtype=torch.float32, device=cuda)
    stream = _stream_handle(cuda)
    touched_before = np.zeros(F, bool)
    moved_without_gradient = 0
    for t in range(3):
        if t == 1:  # a misaligned, padded G: base 4 B past a 16-B boundary
            ld = K + 5
            G = torch.empty(B * ld + 1, device=cuda)[1:].view(B, ld)[:, :K]
            assert G.data_ptr() % 16 == 4
        else:       # the trainer's layout: 16-B aligned padded rows
            G = gs.empty_dense(B, K, cuda)
        G.copy_(torch.randn((B, K), generator=gen, device=cuda))
        rows = perm[t * B:(t + 1) * B]
        T = gs.DeviceCSR.from_scipy(X[rows].T.tocsr(), cuda)
        D = torch.zeros((F, K), device=cuda)
        D.copy_(gs.spmm(T, G, mode="rowwise"))
        touched = np.diff(X[rows].T.tocsr().indptr) > 0
        assert not touched[:4].any() and touched[7] and (~touched[4:]).any()
        only = touched[list(ONLY_FIRST)]
        assert only.all() if t == 0 else not only.any()

        a_t.fill_(2e-3 / (1 - 0.9 ** (t + 1)))
        p, m, u = state["adamax"]
        before = p.clone()
        M.w1_adamax_step(p, m, u, G, seg, t, a_t)
        pr, mr, ur = state["adamax_ref"]
        g = D.contiguous()
        call("gcg_adamax_step_f32", pr.numel(), _ptr(pr), _ptr(g), _ptr(mr), _ptr(ur), _ptr(a_t),
             0.9, 0.999, 1e-8, stream)
        for got, ref, name in ((p, pr, "p"), (m, mr, "m"), (u, ur, "u")):
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), ("adamax", name, t)
        quiet = touched_before & ~touched  # m is non-zero, this batch's gradient is zero
        moved_without_gradient += int((p != before)[torch.from_numpy(quiet).to(cuda)].sum())
        assert torch.equal(p[:4].view(torch.int32), W[:4].view(torch.int32))  # never touched
        touched_before |= touched

        a_t.fill_(0.002 * np.sqrt(1 - 0.999 ** (t + 1)) / (1 - 0.9 ** (t + 1)))
        p, m, v = state["adam"]
        M.w1_step(p, m, v, G, seg, t, 1e-3, 2e-3, a_t)
        pr, mr, vr = state["adam_ref"]
        pen = torch.empty_like(pr)
        call("gcg_l1l2_grad_f32", pr.numel(), _ptr(pr), 1e-3, 2e-3, None, _ptr(pen), stream)
        g = (D + pen).contiguous()
        call("gcg_adam_step_f32", pr.numel(), _ptr(pr), _ptr(g), _ptr(mr), _ptr(vr), _ptr(a_t),
             0.9, 0.999, 1e-8, stream)
        for got, ref, name in ((p, pr, "p"), (m, mr, "m"), (v, vr, "v")):
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), ("adam", name, t)
    assert moved_without_gradient > 0
    assert bool((state["adamax"][2] != 0).any())


# -- 2. the trainer --------------------------------------------------------------------------------
def model(cuda, hid, init, B, **kw):
    from graphconvgeo_amd import loc2lang as L
    kw.setdefault("n_epochs", 8)
    return L.NNModel_loc2lang_nomdn(batch_size=B, hid_size=hid, n_gaus_comp=N_UNITS,
                                    init_parameters=init, device=cuda, **kw)


@gpu
@pytest.mark.parametrize("hid", [8, 0])
@pytest.mark.parametrize("kind", ["dense", "grid"])
def test_trajectory_matches_the_float64_trainer(cuda, kind, hid):
    Xtr, Ytr, Xdev, Ydev, init, orders, B, _ = nomdn_problem(kind, hid)
    clf = model(cuda, hid, init, B, early_stopping_max_down=8)
    assert clf.names == names(hid) and clf.input_size is None
    ppl_test, ppl_dev = clf.fit(Xtr, Ytr, Xdev, Ydev, Xdev[:7], Ydev[:7], epoch_orders=orders)
    assert clf.input_size == Xtr.shape[1] and clf.nomdn is True
    ref_hist, ref_params = train(Xtr, Ytr, Xdev, Ydev, init, orders, B)
    hist = [{"batch_losses": b, "val_loss": h["val_loss"]}
            for b, h in zip(clf.epoch_batch_losses, clf.history)]
    assert len(clf.history) == 8
    within_trajectory_bound(hist, dict(zip(names(hid), clf.last_params)), ref_hist, ref_params,
                            f"{kind} hid={hid}")
    ref_b = np.array([h["batch_losses"] for h in ref_hist])
    assert ref_b[-1].mean() < ref_b[0].mean()  # it trains
    assert ppl_dev == np.power(2, clf.dev_loss) and ppl_test == np.power(2, clf.test_loss)
    assert clf.dev_loss == clf.best_val_loss  # the best parameters are back
    if kind == "grid":  # rows of Wg that no training row touches keep their bits
        untouched = np.diff(sps.csc_matrix(Xtr).indptr) == 0
        assert 50 < untouched.sum() < untouched.size - 50
        Wg = clf.last_params[0]
        assert np.array_equal(Wg[untouched].view(np.int32), init[0][untouched].view(np.int32))
        # and the rows that move in float64 (a touched row whose units are all off does not) move
        moved64 = np.abs(ref_params["Wg"] - init[0]).max(axis=1) > 1e-6
        assert moved64.sum() > 50 and not moved64[untouched].any()
        assert (Wg != init[0]).any(axis=1)[moved64].all()
        assert np.array_equal(clf.get_params()[0][untouched].view(np.int32),
                              init[0][untouched].view(np.int32))


@pytest.fixture(scope="module")
def fitted(cuda):
    """One grid model, hid 8, fit for two epochs; shared and left unchanged."""
    Xtr, Ytr, Xdev, Ydev, init, orders, B, coords = nomdn_problem("grid", 8)
    clf = model(cuda, 8, init, B, n_epochs=2)
    clf.fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev, epoch_orders=orders)
    return clf, Xtr, Xdev, Ytr, Ydev, init, orders, B


def analyses(clf, X):
    ptr, rows = np.array([0, 3, 10, 40]), np.arange(40)
    return {
        "predict": clf.predict(X),
        "gaus_output": clf.gaus_output(X),
        "word_entropies": clf.word_entropies(X).cpu().numpy(),
        "local_words": clf.local_words(X, 10),
        "word_probabilities": clf.word_probabilities(X, [3, 0, 36, 3]),
        "top_words": clf.top_words(X, 5),
        "region_word_scores": clf.region_word_scores(X, ptr, rows).cpu().numpy(),
    }


@gpu
def test_scipy_and_device_inputs_and_two_chunk_sizes(cuda, fitted, monkeypatch):
    """Every method that takes X gives the same result for a scipy CSR and a DeviceCSR (bitwise:
    the same launches), and, in chunks of 7 rows instead of one chunk, within float32 rounding
    (the GEMMs behind the first layer may tile 7 rows differently from 40, as
    tests/test_loc2lang_gpu.py notes) with the rankings unchanged; all of it against the float64
    restatement."""
    from graphconvgeo_amd import loc2lang as L
    from graphconvgeo_amd import sparse as gs
    clf, Xtr, Xdev, Ytr, Ydev = fitted[:5]
    params = dict(zip(names(8), clf.get_params()))
    whole = analyses(clf, Xdev)
    on_device = analyses(clf, gs.DeviceCSR.from_scipy(Xdev, cuda))
    for k in whole:
        assert np.array_equal(whole[k], on_device[k], equal_nan=True), k
    p64 = predict(Xdev, params)
    assert whole["predict"].shape == (40, 37) and np.abs(whole["predict"] - p64).max() <= 1e-5
    G64 = first_layer(Xdev.astype(np.float64), {k: v.astype(np.float64) for k, v in params.items()})
    assert whole["gaus_output"].shape == (40, N_UNITS)
    assert np.abs(whole["gaus_output"] - G64).max() <= 1e-5 and (G64 > 0).any()
    assert np.array_equal(whole["local_words"], R.local_words(p64, 10))
    assert np.abs(whole["word_probabilities"] - p64[:, [3, 0, 36, 3]]).max() <= 1e-5
    assert np.array_equal(whole["top_words"], np.argsort(-p64, axis=1, kind="stable")[:, :5])
    logp = np.log(p64)
    want = np.stack([logp[a:b].mean(axis=0) for a, b in ((0, 3), (3, 10), (10, 40))]) - logp.mean(axis=0)
    assert np.abs(whole["region_word_scores"] - want).max() <= 1e-4
    dev_loss = clf.dev_loss

    monkeypatch.setattr(L, "EVAL_CHUNK_BYTES", 4 * 40 * 8)  # 7 rows of 40 floats per chunk
    assert clf._chunk_rows() == 7
    chunked = analyses(clf, Xdev)
    for k in ("local_words", "top_words"):
        assert np.array_equal(whole[k], chunked[k]), k
    for k in ("predict", "gaus_output", "word_entropies", "word_probabilities"):
        assert np.abs(whole[k] - chunked[k]).max() <= 1e-6, k
    assert np.abs(whole["region_word_scores"] - chunked["region_word_scores"]).max() <= 1e-5
    x, Yd = clf._split(Xdev, Ydev, "dev")
    assert abs(clf._evaluate(x, Yd) - dev_loss) <= 1e-6 * dev_loss


@gpu
@pytest.mark.parametrize("kind", ["grid", "dense"])
def test_epoch_runs_without_host_synchronisation(cuda, kind):
    Xtr, Ytr, Xdev, Ydev, init, orders, B, _ = nomdn_problem(kind, 8)
    clf = model(cuda, 8, init, B, n_epochs=1)
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


@gpu
def test_parameters_round_trip_in_the_stated_order(cuda, fitted):
    from graphconvgeo_amd import loc2lang as L
    clf, Xtr, Xdev, Ytr, Ydev, init, orders, B = fitted
    fresh = model(cuda, 8, init, B, input_size=377, output_size=37)  # built in the constructor
    assert fresh.names == ["Wg", "bg", "Wh", "bh", "Wo", "bo"]
    got = fresh.get_params()
    assert [p.shape for p in got] == [(377, 6), (6,), (6, 8), (8,), (8, 37), (37,)]
    assert all(np.array_equal(a, b) for a, b in zip(got, init))
    trained = clf.get_params()
    fresh.set_params(trained)
    assert all(np.array_equal(a, b) for a, b in zip(fresh.get_params(), trained))
    assert np.array_equal(fresh.predict(Xdev), clf.predict(Xdev))
    with pytest.raises(ValueError, match="expected"):
        fresh.set_params(trained[:4])
    with pytest.raises(ValueError, match="init_parameters must be \\[Wg, bg, Wo, bo\\]"):
        model(cuda, 0, init, B, input_size=377, output_size=37)
    assert L.NNModel_loc2lang_nomdn(output_size=37, device=cuda).params is None  # no width yet


@gpu
def test_default_init_draws_in_lasagne_construction_order(cuda):
    from graphconvgeo_amd import loc2lang as L
    F, C_, V = 9, 6, 11
    for hid in (4, 0):
        np.random.seed(77)
        clf = L.NNModel_loc2lang_nomdn(input_size=F, output_size=V, hid_size=hid, n_gaus_comp=C_,
                                       device=cuda)
        rs = np.random.RandomState(77)
        want = []
        for a, b in [(F, C_)] + ([(C_, hid)] if hid else []) + [(hid or C_, V)]:
            lim = np.sqrt(6.0 / (a + b))
            want += [rs.uniform(-lim, lim, size=(a, b)).astype(np.float32), np.zeros(b, np.float32)]
        got = clf.get_params()
        assert len(got) == len(want) == (6 if hid else 4)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


@gpu
def test_refusals_on_the_device(cuda, fitted):
    clf, Xtr, Xdev, Ytr, Ydev, init, orders, B = fitted
    for bad in (Xdev[:, :300], Xdev[:, :300].toarray(), np.zeros((4, 2), np.float32)):
        with pytest.raises(ValueError, match=r"X has \d+ columns, the model 377"):
            clf.predict(bad)
    with pytest.raises(ValueError, match="permutation"):
        model(cuda, 8, init, B, n_epochs=1).fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev,
                                                epoch_orders=[np.zeros(96, np.int64)])
    with pytest.raises(ValueError, match="differ in width|columns, the model"):
        model(cuda, 8, init, B).fit(Xtr, Ytr, Xdev[:, :300], Ydev, Xdev, Ydev)
    with pytest.raises(ValueError, match="fewer than one batch"):
        model(cuda, 8, init, 97).fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev)


# -- 3. from coordinates through the grid to a fit ---------------------------------------------
CENTRES = np.array([[40.7128, -74.0060], [34.0522, -118.2437]])  # New York, Los Angeles


def outranks(probs):
    """probs [2, 20] at the two centres: every own word of a place above every word of the other."""
    return bool(probs[0, :8].min() > probs[0, 8:16].max() and
                probs[1, 8:16].min() > probs[1, :8].max())


@gpu
@pytest.mark.parametrize("hid", [0, 8])
def test_two_regions_through_the_grid(cuda, hid):
    """loc2lang_reference.two_regions_data moved to two US cities (the grid covers the US box):
    400 training and 100 dev points, sigma 0.5 degrees, V = 20 with 8 words per place; 16 units,
    B = 50, 30 epochs = 240 Adamax steps from GlorotUniform weights of a RandomState(7). The
    float64 CPU trainer on the restated grid rows runs first and is shown to learn: its dev loss
    falls 2.993 -> 2.626 (no hidden layer) / 2.992 -> 2.666 (hid 8), the own-word margins at the
    centres are 0.54 / 0.50 and 0.63 / 0.46, and every own word of a place outranks every word of
    the other place there; asserted of it: a fall of more than 0.15, margins of at least 0.3 (what
    tests/test_loc2lang_gpu.py asks of the Gaussian model) and the ranking. Of the GPU run, from
    the coordinates through grid_representation on the device to fit on the DeviceCSR: the
    dev-loss history within 1e-4 relative of float64's, the same margins and the ranking."""
    from graphconvgeo_amd import grid
    from graphconvgeo_amd import loc2lang as L
    Xtr, Ytr, Xdev, Ydev = R.two_regions_data()
    place = np.arange(500) % 2
    moved = np.concatenate([Xtr, Xdev]) - R.MELBOURNES[place] + CENTRES[place]
    rs = np.random.RandomState(7)

    def glorot(a, b):
        lim = np.sqrt(6.0 / (a + b))
        return rs.uniform(-lim, lim, size=(a, b)).astype(np.float32)

    init = [glorot(5800, 16), np.zeros(16, np.float32)]
    if hid:
        init += [glorot(16, hid), np.zeros(hid, np.float32)]
    init += [glorot(hid or 16, 20), np.zeros(20, np.float32)]
    orders = [rs.permutation(400) for _ in range(30)]
    Xref = GR.grid_representation(moved)
    hist, p64 = train(Xref[:400], Ytr, Xref[400:], Ydev, init, orders, 50)
    ref = np.array([h["val_loss"] for h in hist])
    probs64 = predict(GR.grid_representation(CENTRES), p64)
    margin64 = R.own_word_margin(probs64)
    print("float64: dev", ref[0], ref[-1], "margins", margin64)
    assert ref[0] - ref[-1] > 0.15 and margin64.min() >= 0.3 and outranks(probs64)

    X = grid.grid_representation(moved, device=cuda)
    assert X.shape == (500, 5800) and int((X.indptr[1:] == X.indptr[:-1]).sum()) == 0
    clf = L.NNModel_loc2lang_nomdn(n_epochs=30, batch_size=50, hid_size=hid, n_gaus_comp=16,
                                   early_stopping_max_down=30, init_parameters=init, device=cuda)
    clf.fit(X.row_slice(0, 400), Ytr, X.row_slice(400, 500), Ydev, X.row_slice(400, 500), Ydev,
            epoch_orders=orders)
    got = np.array([h["val_loss"] for h in clf.history])
    print("gpu: dev", got[0], got[-1], "largest deviation", np.abs(got - ref).max())
    assert got.shape == ref.shape == (30,)
    assert np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref))
    probs = clf.predict(grid.grid_representation(CENTRES, device=cuda))
    margin = R.own_word_margin(probs)
    print("gpu: margins", margin)
    assert margin.min() >= 0.3 and outranks(probs)
