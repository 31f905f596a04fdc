"""GPU tests of the location-to-language model's analyses (graphconvgeo_amd.loc2lang: row_lse,
softmax_column_stats, the model's word_entropies / local_words / word_probabilities / top_words /
region_word_scores; csrc/vocab_stats.hip; reference loc2lang.py:516-614, 693-766). The judge is
tests/loc2lang_analysis_reference.py in float64 on the same float32 logits; the bar for a kernel is
what the same restatement achieves in float32: error <= 4 x the float32 restatement's + 1e-6, the
bar tests/test_loc2lang_gpu.py uses for the loss."""
import json
import os

import numpy as np
import pytest
import torch

import loc2lang_analysis_reference as A
import loc2lang_reference as R
from graphconvgeo_amd import geo
from graphconvgeo_amd import loc2lang as L
from graphconvgeo_amd import mdn
from graphconvgeo_amd import sparse as gs
from graphconvgeo_amd._native import call
from graphconvgeo_amd.sparse import _ptr, _stream_handle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "profiles", "loc2lang_analysis", "accuracy.jsonl")
LSE_SHAPES = [(M_, N) for M_ in (1, 5, 67)
              for N in (1, 3, 255, 256, 257, 1024, 1025, 4097, 70001)]
STATS_SHAPES = [(M_, N) for M_ in (1, 2, 67, 300) for N in (1, 3, 63, 64, 65, 257, 4099)]
SPREADS = (1.0, 30.0)
NAN = float("nan")
_inputs = {}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def logits_of(M_, N, spread):
    """R.xent_inputs' logits of one case (computed once, never modified)."""
    key = (M_, N, spread)
    if key not in _inputs:
        _inputs[key] = R.xent_inputs(M_, N, spread)[0]
    return _inputs[key]


@pytest.fixture(scope="module")
def accuracy_log():
    records = {}
    yield records
    want = len(SPREADS) * (len(LSE_SHAPES) + len(STATS_SHAPES))
    if len(records) == want:  # both sweeps ran whole: rewrite the file
        os.makedirs(os.path.dirname(ACCURACY), exist_ok=True)
        with open(ACCURACY, "w") as f:
            for key in sorted(records):
                f.write(json.dumps(records[key]) + "\n")


def on_device(cuda, Z, pad=0):
    """Z on row strides N + pad, the padding holding NaN."""
    M_, N = Z.shape
    Zd = torch.full((M_, N + pad), NAN, dtype=torch.float32, device=cuda)
    Zd[:, :N] = torch.from_numpy(np.ascontiguousarray(Z))
    return Zd


def run_lse(cuda, Z, pad=0):
    """One gcg_row_lse_f64 call: lse as NumPy float64."""
    M_, N = Z.shape
    Zd = on_device(cuda, Z, pad)
    lse = torch.full((M_,), 7.0, dtype=torch.float64, device=cuda)
    call("gcg_row_lse_f64", M_, N, _ptr(Zd), N + pad, _ptr(lse), _stream_handle(cuda))
    return lse.cpu().numpy()


def run_stats(cuda, Z, lse, pad=0, splits=None, S0=None, T0=None):
    """gcg_softmax_column_stats_f64 over the rows of Z, in one call or in consecutive calls of
    `splits` rows each, onto S0 / T0 (zeros when None): (S, T) as NumPy float64."""
    M_, N = Z.shape
    Zd = on_device(cuda, Z, pad)
    ld = torch.from_numpy(np.ascontiguousarray(lse)).to(cuda)
    S = torch.zeros(N, dtype=torch.float64, device=cuda) if S0 is None else \
        torch.from_numpy(S0.copy()).to(cuda)
    T = torch.zeros(N, dtype=torch.float64, device=cuda) if T0 is None else \
        torch.from_numpy(T0.copy()).to(cuda)
    a = 0
    for m in splits or [M_]:
        call("gcg_softmax_column_stats_f64", m, N, _ptr(Zd[a:]) if a < M_ else _ptr(Zd), N + pad,
             _ptr(ld[a:]) if a < M_ else _ptr(ld), _ptr(S), _ptr(T), _stream_handle(cuda))
        a += m
    assert a == M_
    return S.cpu().numpy(), T.cpu().numpy()


# -- 1. the row log-sum-exp ----------------------------------------------------------------------
def lse_err(x, ref):
    return float((np.abs(x - ref) / np.maximum(1.0, np.abs(ref))).max())


@pytest.mark.parametrize("M_,N", LSE_SHAPES)
def test_row_lse_within_four_times_float32(cuda, accuracy_log, M_, N):
    """lse over max(1, |ref|) against float64 <= 4 x the float32 restatement's + 1e-6; a padded
    ldl with NaN in the padding gives the same bits, and so does a second call."""
    for spread in SPREADS:
        Z = logits_of(M_, N, spread)
        ref, f32 = A.row_lse(Z), A.row_lse(Z, np.float32).astype(np.float64)
        got = run_lse(cuda, Z)
        assert same_bits(got, run_lse(cuda, Z, pad=3))
        assert same_bits(got, run_lse(cuda, Z))
        rec = {"kernel": "row_lse", "M": M_, "N": N, "spread": spread,
               "lse_err_kernel": lse_err(got, ref), "lse_err_f32": lse_err(f32, ref)}
        print(rec)
        accuracy_log[("lse", M_, N, spread)] = rec
        assert rec["lse_err_kernel"] <= 4 * rec["lse_err_f32"] + 1e-6, rec
        Zd = torch.from_numpy(Z.copy()).to(cuda)
        assert same_bits(L.row_lse(Zd).cpu().numpy(), got)


def test_row_lse_rows_and_edge_rows(cuda):
    """A row's lse is bitwise that of a one-row call (N = 4097 odd: rows 1, 2, 3 start off a 16-B
    boundary, the one-row call's row is aligned); a row holding -inf entries gives the float64
    value; a row of equal entries gives z + log N (its float32 sum of N ones is exact); a NaN, a
    +inf and an all -inf row give NaN, NaN and -inf and touch no other row."""
    Z = logits_of(67, 4097, 30.0)
    got = run_lse(cuda, Z)
    for r in (0, 1, 2, 3, 40, 66):
        assert same_bits(run_lse(cuda, Z[r:r + 1]), got[r:r + 1]), r
    E = Z.copy()
    E[5, ::3] = -np.inf
    E[6, 1:] = -np.inf
    E[7, :] = np.float32(-2.75)
    E[8, 100], E[9, 4096], E[10, :] = np.nan, np.inf, -np.inf
    out = run_lse(cuda, E)
    ref, f32 = A.row_lse(E[5:7]), A.row_lse(E[5:7], np.float32).astype(np.float64)
    assert lse_err(out[5:7], ref) <= 4 * lse_err(f32, ref) + 1e-6
    assert out[6] == float(E[6, 0])
    assert abs(out[7] - (-2.75 + np.log(4097.0))) <= 1e-13 * abs(out[7])
    assert np.isnan(out[8]) and np.isnan(out[9]) and out[10] == -np.inf
    keep = np.r_[0:5, 11:67]
    assert same_bits(out[keep], got[keep])


# -- 2. the column sums --------------------------------------------------------------------------
def stats_record(S, T, Z):
    """The errors of (S, T) and of the float32 restatement against float64 on the logits Z: S over
    max|ref|, the entropies log S - T / S absolutely. The kernel's entropies must be NaN exactly
    where float64's are; the float32 restatement's error is taken over the columns where it has a
    number (it underflows to S = 0 where float64 does not), which only lowers the bar."""
    S64, T64, e64 = A.column_stats(Z)
    S32, T32, e32 = A.column_stats_f32(Z)
    with np.errstate(all="ignore"):
        ent = np.where(S == 0, np.nan, np.log(S) - T / S)
    assert np.array_equal(np.isnan(ent), np.isnan(e64))
    fin = ~np.isnan(e64)

    def ent_err(e):
        d = np.abs(e[fin] - e64[fin])
        d = d[~np.isnan(d)]  # the float32 restatement underflows to S = 0 where float64 does not
        return float(d.max()) if d.size else 0.0

    top = np.abs(S64).max()
    return {"S_err_kernel": float(np.abs(S - S64).max() / top) if top else float(np.abs(S).max()),
            "S_err_f32": float(np.abs(S32 - S64).max() / top) if top else 0.0,
            "ent_err_kernel": ent_err(ent), "ent_err_f32": ent_err(e32)}, ent


def assert_within_bar(rec):
    for name in ("S", "ent"):
        assert rec[name + "_err_kernel"] <= 4 * rec[name + "_err_f32"] + 1e-6, (name, rec)


@pytest.mark.parametrize("M_,N", STATS_SHAPES)
def test_column_stats_within_four_times_float32(cuda, accuracy_log, M_, N):
    """S over max|ref| and the entropies log S - T / S absolutely, against float64, <= 4 x the
    float32 restatement's + 1e-6 (lse from gcg_row_lse_f64, as the model takes it); at spread 30
    most p underflow in float32. NaN in the ldl padding reaches nothing; two runs agree bitwise."""
    for spread in SPREADS:
        Z = logits_of(M_, N, spread)
        lse = run_lse(cuda, Z)
        S, T = run_stats(cuda, Z, lse)
        assert np.isfinite(S).all() and np.isfinite(T).all()
        for other in (run_stats(cuda, Z, lse, pad=3), run_stats(cuda, Z, lse)):
            assert same_bits(other[0], S) and same_bits(other[1], T)
        rec, _ = stats_record(S, T, Z)
        rec = {"kernel": "softmax_column_stats", "M": M_, "N": N, "spread": spread, **rec}
        print(rec)
        accuracy_log[("stats", M_, N, spread)] = rec
        assert_within_bar(rec)


@pytest.mark.parametrize("N", [65, 4099])
def test_column_stats_row_splits_and_accumulation(cuda, N):
    """M = 67 as calls of 1, 0, 29 and 37 rows is bitwise the single call (from zero and from
    non-zero S, T alike); accumulating onto non-zero S and T adds to them; the wrapper gives the
    kernel's bits."""
    for spread in SPREADS:
        Z = logits_of(67, N, spread)
        lse = run_lse(cuda, Z)
        S, T = run_stats(cuda, Z, lse)
        Ss, Ts = run_stats(cuda, Z, lse, splits=[1, 0, 29, 37])
        assert same_bits(Ss, S) and same_bits(Ts, T)
        Ss, Ts = run_stats(cuda, Z, lse, splits=[8, 8, 8, 43], pad=1)
        assert same_bits(Ss, S) and same_bits(Ts, T)
        rng = np.random.default_rng(N)
        S0, T0 = rng.random(N) + 0.5, -rng.random(N)
        S1, T1 = run_stats(cuda, Z, lse, S0=S0, T0=T0)
        S2, T2 = run_stats(cuda, Z, lse, S0=S0, T0=T0, splits=[1, 0, 29, 37])
        assert same_bits(S2, S1) and same_bits(T2, T1)
        # the same 67 terms added in another order: 67 roundings of a running value on either
        # side and one of the comparison's own sum, each at most 2^-53 of the largest
        assert np.abs(S1 - (S0 + S)).max() <= 135 * 1.12e-16 * (S0 + S).max()
        assert np.abs(T1 - (T0 + T)).max() <= 135 * 1.12e-16 * np.abs(T0 + T).max()
        Zd = torch.from_numpy(Z.copy()).to(cuda)
        Sw = torch.zeros(N, dtype=torch.float64, device=cuda)
        Tw = torch.zeros_like(Sw)
        L.softmax_column_stats(Zd[:30], L.row_lse(Zd[:30]), Sw, Tw)
        L.softmax_column_stats(Zd[30:], L.row_lse(Zd[30:]), Sw, Tw)
        assert same_bits(Sw.cpu().numpy(), S) and same_bits(Tw.cpu().numpy(), T)


def test_column_stats_minus_infinity(cuda):
    """A -inf logit contributes 0 to both sums, and a column that is -inf in every row gives
    S = 0 and T = 0 exactly (the entropy there is NaN); the rest is within the bar."""
    for spread in SPREADS:
        Z = logits_of(67, 257, spread).copy()
        Z[3, 5] = Z[10, 200] = Z[66, 256] = -np.inf
        Z[:, 9] = Z[:, 64] = -np.inf
        lse = run_lse(cuda, Z)
        S, T = run_stats(cuda, Z, lse)
        assert S[9] == 0 and T[9] == 0 and S[64] == 0 and T[64] == 0
        assert np.isfinite(S).all() and np.isfinite(T).all()
        rec, ent = stats_record(S, T, Z)
        print(rec)
        assert_within_bar(rec)
        assert np.isnan(ent[9]) and np.isnan(ent[64]) and np.isfinite(np.delete(ent, [9, 64])).all()
        T64 = A.column_stats(Z)[1]
        assert np.abs(T - T64).max() <= (4 * np.abs(A.column_stats_f32(Z)[1] - T64).max() / np.abs(
            T64).max() + 1e-6) * np.abs(T64).max()


def test_wrappers_refuse_bad_operands(cuda):
    Z = torch.zeros((3, 4), device=cuda)
    lse = torch.zeros(3, dtype=torch.float64, device=cuda)
    S = torch.zeros(4, dtype=torch.float64, device=cuda)
    T = torch.zeros_like(S)
    L.softmax_column_stats(Z, lse, S, T)
    assert S.cpu().tolist() == [3.0] * 4 and T.cpu().tolist() == [0.0] * 4   # p = 1, a = 0
    for bad in (lambda: L.softmax_column_stats(Z, lse[:2], S, T),
                lambda: L.softmax_column_stats(Z, lse.float(), S, T),
                lambda: L.softmax_column_stats(Z, lse, S[:3], T),
                lambda: L.softmax_column_stats(Z, lse, S, T.cpu()),
                lambda: L.softmax_column_stats(Z, lse, S, S),
                lambda: L.softmax_column_stats(Z, lse, torch.zeros(8, dtype=torch.float64,
                                                                   device=cuda)[::2], T),
                lambda: L.softmax_column_stats(Z.double(), lse, S, T),
                lambda: L.row_lse(Z[0]),
                lambda: L.row_lse(Z[:, :0])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        L.softmax_column_stats(Z, lse.cpu().numpy(), S, T)
    assert L.row_lse(Z[:0]).shape == (0,)


# -- 3. the model --------------------------------------------------------------------------------
K_TOP = 20


@pytest.fixture(scope="module")
def regions(cuda):
    """two_regions_data and the four initial components of test_two_regions."""
    Xtr, Ytr, Xdev, Ydev = R.two_regions_data()
    tree = geo.KDTreeClustering(100).fit(Xtr, device=cuda)
    comp = mdn.cluster_params(Xtr, tree.clusters.cpu().numpy(), tree.num_clusters, raw=True)
    assert tree.num_clusters == 4
    n = Xdev.shape[0]
    # the dev rows alternate between the places; the third group is every row (overlapping)
    group_rows = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2), np.arange(n)])
    group_ptr = np.array([0, n // 2, n, 2 * n])
    return Xtr, Ytr, Xdev, Ydev, comp, group_ptr, group_rows


def make_model(cuda, regions, hid, n_epochs=0):
    Xtr, Ytr, Xdev, Ydev, comp = regions[:5]
    clf = L.NNModel_loc2lang(n_epochs=n_epochs, batch_size=50, hid_size=hid, n_gaus_comp=4,
                             early_stopping_max_down=60, device=cuda,
                             init_parameters=R.two_regions_init(comp, hid))
    rs = np.random.RandomState(7)
    clf.fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev, epoch_orders=[rs.permutation(400)
                                                             for _ in range(n_epochs)])
    return clf


@pytest.fixture(scope="module", params=[0, 8])
def fresh(request, cuda, regions):
    """The model at two_regions_init's parameters, and its own float32 logits on the dev rows."""
    clf = make_model(cuda, regions, request.param)
    Z = clf._logits(clf._to_coords(regions[2])).cpu().numpy()
    return clf, Z


@pytest.fixture(scope="module", params=[0, 8])
def fitted(request, cuda, regions):
    """test_two_regions' fit (60 epochs of 8 batches), meeting its margins."""
    clf = make_model(cuda, regions, request.param, n_epochs=60)
    assert R.own_word_margin(clf.predict(R.MELBOURNES)).min() >= 0.3
    return clf


def entropy_bar(Z):
    """(4 x the float32 restatement's largest entropy error + 1e-6, the float64 entropies); a word
    without an entropy (S = 0, NaN in both) has no error."""
    e64, e32 = A.column_stats(Z)[2], A.column_stats_f32(Z)[2]
    assert np.array_equal(np.isnan(e32), np.isnan(e64))
    d = np.abs(e32 - e64)[~np.isnan(e64)]
    return 4 * float(d.max() if d.size else 0.0) + 1e-6, e64


def check_entropies_and_local_words(clf, Xdev):
    Z = clf._logits(clf._to_coords(Xdev)).cpu().numpy()
    bar, e64 = entropy_bar(Z)
    ent = clf.word_entropies(Xdev)
    assert ent.dtype == torch.float64 and ent.is_cuda and tuple(ent.shape) == (20,)
    err = np.abs(ent.cpu().numpy() - e64).max()
    print("entropies: error", err, "bar", bar)
    assert err <= bar
    for k in (1, 5, 16, 20):
        words = clf.local_words(Xdev, k)
        assert words.shape == (k,) and len(set(words.tolist())) == k
        assert np.all(np.diff(e64[words]) >= -2 * bar)
        rest = np.setdiff1d(np.arange(20), words)
        assert rest.size == 0 or e64[rest].min() >= e64[words[-1]] - 2 * bar
    assert clf.local_words(Xdev).shape == (20,)   # k = 50 of 20 words: all of them
    return e64


def test_word_entropies_and_local_words(cuda, regions, fresh):
    """word_entropies against the restatement on the model's own float32 logits, within the bar;
    local_words as an ordering of the float64 entropies, no share excluded: non-decreasing at the
    returned indices up to twice the bar, and no word left out more than twice the bar below the
    k-th."""
    check_entropies_and_local_words(fresh[0], regions[2])


def test_fitted_model_entropies_and_local_words(cuda, regions, fitted):
    """The same after the fit, where the entropies are far apart: a place's own words, which the
    model now gives to half of the dev rows, are more local than the four common words."""
    e64 = check_entropies_and_local_words(fitted, regions[2])
    assert e64[:16].mean() < e64[16:].mean()


def test_word_probabilities_are_predict_columns(cuda, regions, fresh):
    clf, _ = fresh
    Xdev = regions[2]
    probs = clf.predict(Xdev)
    words = [3, 3, 19, 0, 7, 3]   # repeated and unsorted
    got = clf.word_probabilities(Xdev, words)
    assert got.shape == (100, 6) and got.dtype == np.float32
    assert np.abs(got - probs[:, words]).max() <= 1e-6
    t = clf.word_probabilities(Xdev, np.arange(20), as_tensor=True)
    assert t.is_cuda and t.dtype == torch.float32
    assert np.abs(t.cpu().numpy() - probs).max() <= 1e-6
    assert clf.word_probabilities(Xdev, []).shape == (100, 0)
    for bad in ([0, 20], [-1], [0.5]):
        with pytest.raises(ValueError, match="words"):
            clf.word_probabilities(Xdev, bad)


def test_top_words_tie_rule(cuda, regions, fresh):
    """Equal columns of Wo and bo give bitwise equal logits (asserted of the fixture): words 4, 11
    and 17 tie in every row, 2 and 9 as well, and the lower index comes first."""
    clf, _ = fresh
    Xdev = regions[2]
    saved = clf.get_params()
    try:
        params = [p.copy() for p in saved]
        for a, b in ((4, 11), (4, 17), (2, 9)):
            params[-2][:, b] = params[-2][:, a]
            params[-1][b] = params[-1][a]
        clf.set_params(params)
        Z = clf._logits(clf._to_coords(Xdev)).cpu().numpy()
        assert np.array_equal(Z[:, 4], Z[:, 11]) and np.array_equal(Z[:, 4], Z[:, 17])
        assert np.array_equal(Z[:, 2], Z[:, 9])
        for k in (1, 7, 20):
            top = clf.top_words(Xdev, k)
            assert top.shape == (100, k) and np.array_equal(top, A.top_words(Z, k))
        full = clf.top_words(Xdev, 20)
        where = np.argsort(full, axis=1)   # where[r, w]: the place of word w in row r
        assert np.all(where[:, 11] == where[:, 4] + 1) and np.all(where[:, 17] == where[:, 4] + 2)
        assert np.all(where[:, 9] == where[:, 2] + 1)
        for k in (0, 21):
            with pytest.raises(ValueError, match="k must be"):
                clf.top_words(Xdev, k)
    finally:
        clf.set_params(saved)


GOLD_PTR = np.array([0, 8, 16, 16])     # each place's own 8 words; the group of all rows has none
GOLD_WORD = np.arange(16)
FRACTIONS = (0.01, 0.1, 0.25, 0.4, 0.5)  # V = 20: k = 0, 2, 5, 8, 10


def check_scores(clf, Xdev, Z, group_ptr, group_rows):
    ref = A.region_scores(Z, group_ptr, group_rows)
    f32 = A.region_scores(Z, group_ptr, group_rows, np.float32).astype(np.float64)
    assert np.isfinite(f32).all()
    scores = clf.region_word_scores(Xdev, group_ptr, group_rows)
    assert scores.is_cuda and scores.dtype == torch.float32 and tuple(scores.shape) == (3, 20)
    top = max(1.0, np.abs(ref).max())
    err, err32 = np.abs(scores.cpu().numpy() - ref).max() / top, np.abs(f32 - ref).max() / top
    print("region scores: error", err, "float32 restatement", err32)
    assert err <= 4 * err32 + 1e-6
    r64 = A.region_recall(ref, GOLD_PTR, GOLD_WORD, FRACTIONS)
    r32 = A.region_recall(f32.astype(np.float32), GOLD_PTR, GOLD_WORD, FRACTIONS)
    # if the two restatements rank a gold word differently the fixture is wrong, not the kernel
    assert np.array_equal(r64[4], r32[4])
    got = L.region_recall(scores, GOLD_PTR, GOLD_WORD, FRACTIONS)
    assert got.ks == r64[0] == [0, 2, 5, 8, 10]
    assert np.array_equal(got.ranks, r64[4])
    assert np.array_equal(got.per_group, r64[3], equal_nan=True)
    assert got.recall == r64[1] and got.oracle == r64[2]
    assert np.isnan(got.per_group[:, 2]).all() and got.recall[0] == 0.0
    return scores.cpu().numpy(), got


def test_region_word_scores_and_recall(cuda, regions, fresh):
    """region_word_scores against the literal float64 form (np.log(softmax), group means minus
    the global mean) on the model's own logits, within the bar; groups: the two places and all
    rows (overlapping; its scores are the mean minus itself, 0). region_recall on the device
    scores gives the ranks both restatements give."""
    clf, Z = fresh
    Xdev, group_ptr, group_rows = regions[2], regions[5], regions[6]
    scores, _ = check_scores(clf, Xdev, Z, group_ptr, group_rows)
    assert np.abs(scores[2]).max() <= 1e-6
    for ptr, rows, what in (([0, 50, 50, 100], group_rows[:100], "empty"),
                            ([0, 50, 101], group_rows[:100], "monotone"),
                            ([0, 50, 100], np.r_[group_rows[:99], 100], "outside")):
        with pytest.raises(ValueError, match=what):
            clf.region_word_scores(Xdev, ptr, rows)


def test_fitted_regions_rank_their_own_words_first(cuda, regions, fitted):
    """After the fit each place's own 8 words outrank the other place's 8 in its group's scores,
    and the recall at k = 8 of 20 reflects it."""
    Xdev, group_ptr, group_rows = regions[2], regions[5], regions[6]
    Z = fitted._logits(fitted._to_coords(Xdev)).cpu().numpy()
    scores, got = check_scores(fitted, Xdev, Z, group_ptr, group_rows)
    assert scores[0, :8].min() > scores[0, 8:16].max()
    assert scores[1, 8:16].min() > scores[1, :8].max()
    assert got.ranks.max() < 12 and got.recall[4] >= got.recall[3] >= 0.5
    assert got.oracle == [0.0, 0.25, 0.625, 1.0, 1.0]


def test_chunks_do_not_change_the_analyses(cuda, regions, fresh, monkeypatch):
    """100 rows in chunks of 7: the entropies and the scores move by float32 rounding at the
    most (1e-6 relative, as test_evaluation_chunks_do_not_change_the_loss sets and explains: the
    GEMMs in front may tile a 7-row problem differently; bitwise is asked of the kernels)."""
    clf, _ = fresh
    Xdev, group_ptr, group_rows = regions[2], regions[5], regions[6]
    ent = clf.word_entropies(Xdev).cpu().numpy()
    scores = clf.region_word_scores(Xdev, group_ptr, group_rows).cpu().numpy()
    probs = clf.word_probabilities(Xdev, [1, 18])
    tops = clf.top_words(Xdev, 3)
    monkeypatch.setattr(L, "EVAL_CHUNK_BYTES", 4 * gs.row_stride(20) * 8)
    assert clf._chunk_rows() == 7
    assert np.abs(clf.word_entropies(Xdev).cpu().numpy() - ent).max() <= 1e-6 * np.abs(ent).max()
    again = clf.region_word_scores(Xdev, group_ptr, group_rows).cpu().numpy()
    assert np.abs(again - scores).max() <= 1e-6 * max(1.0, np.abs(scores).max())
    assert np.abs(clf.word_probabilities(Xdev, [1, 18]) - probs).max() <= 1e-6
    assert clf.top_words(Xdev, 3).shape == tops.shape


def test_minus_infinity_word_has_no_entropy(cuda, regions, fresh):
    """A word whose bias is -inf has probability 0 everywhere: S = 0, and word_entropies gives NaN
    there and the restatement's values elsewhere; local_words puts it last."""
    clf, _ = fresh
    Xdev = regions[2]
    saved = clf.get_params()
    try:
        params = [p.copy() for p in saved]
        params[-1][5] = -np.inf
        clf.set_params(params)
        Z = clf._logits(clf._to_coords(Xdev)).cpu().numpy()
        assert np.all(Z[:, 5] == -np.inf)
        bar, e64 = entropy_bar(Z)
        ent = clf.word_entropies(Xdev).cpu().numpy()
        assert np.isnan(ent[5]) and np.isnan(e64[5])
        keep = np.arange(20) != 5
        assert np.abs(ent[keep] - e64[keep]).max() <= bar
        assert clf.local_words(Xdev, 20)[-1] == 5
    finally:
        clf.set_params(saved)


def test_scan_runs_without_host_synchronisation(cuda, regions, fresh):
    """The scan and what the analyses do per chunk, under set_sync_debug_mode("error"), in two
    chunks; only the final copy of a result synchronises."""
    clf, _ = fresh
    x = clf._to_coords(regions[2])
    words = torch.tensor([3, 0, 3], device=cuda)
    clf.word_entropies(regions[2])   # builds every lazy resource
    S = torch.zeros(20, dtype=torch.float64, device=cuda)
    T = torch.zeros_like(S)
    probs = torch.empty((100, 3), dtype=torch.float32, device=cuda)
    tops = torch.empty((100, 4), dtype=torch.int64, device=cuda)
    lses = torch.empty(100, dtype=torch.float64, device=cuda)
    seen = []

    def per_chunk(a, b, Z, lse):
        seen.append((a, b))
        L.softmax_column_stats(Z, lse, S, T)
        probs[a:b] = torch.exp(Z[:, words].to(torch.float64) - lse[:, None])
        tops[a:b] = torch.sort(Z, dim=1, descending=True, stable=True)[1][:, :4]
        lses[a:b] = lse

    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    step = L.EVAL_CHUNK_BYTES
    L.EVAL_CHUNK_BYTES = 4 * gs.row_stride(20) * 61
    torch.cuda.set_sync_debug_mode("error")
    try:
        clf._scan(x, per_chunk)
        ent = torch.where(S == 0, torch.full_like(S, NAN), torch.log(S) - T / S)
    finally:
        torch.cuda.set_sync_debug_mode(before)
        L.EVAL_CHUNK_BYTES = step
    assert seen == [(0, 60), (60, 100)]
    assert np.abs(ent.cpu().numpy() - clf.word_entropies(regions[2]).cpu().numpy()).max() <= 1e-6
    assert np.abs(probs.cpu().numpy() - clf.predict(regions[2])[:, [3, 0, 3]]).max() <= 1e-6
    assert np.array_equal(tops.cpu().numpy(), clf.top_words(regions[2], 4))
    assert bool(torch.isfinite(lses).all())
