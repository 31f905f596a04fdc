"""CPU tests of the location-to-language model's analyses: the NumPy restatement itself
(tests/loc2lang_analysis_reference.py) against scipy / scikit-learn and against the literal form,
the two new C entries' argument checks without a GPU, the host-side validations, and
region_recall on CPU tensors against the literal restatement of loc2lang.py:580-614."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import loc2lang_analysis_reference as A
import loc2lang_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("gcg_row_lse_f64", "gcg_softmax_column_stats_f64")


# -- the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [1.0, 30.0])
def test_entropies_from_two_sums_are_scipys(spread):
    """log S - T / S from the column sums is scipy.stats.entropy of the l1-normalised columns of
    the float64 softmax; -inf logits and a column that is -inf in every row included."""
    Z = R.xent_inputs(67, 257, spread)[0].copy()
    Z[3, 5] = Z[10, 200] = -np.inf
    Z[:, 9] = -np.inf
    S, T, ent = A.column_stats(Z)
    P = A.softmax(Z)
    assert np.abs(np.exp(A.log_softmax(Z)) - P).max() <= 1e-13   # exp of |a| < 200: 200 eps
    assert np.abs(A.row_lse(Z) - np.log(np.exp(Z.astype(np.float64)).sum(axis=1))).max() <= 1e-12
    assert np.abs(S - P.sum(axis=0)).max() <= 1e-13 * S.max()
    want = A.entropies_literal(P)
    assert S[9] == 0 and T[9] == 0 and np.isnan(ent[9])
    keep = np.arange(257) != 9
    assert np.abs(ent[keep] - want[keep]).max() <= 1e-12
    S32, T32, ent32 = A.column_stats_f32(Z)
    assert np.abs(S32 - S).max() <= 1e-5 * S.max() and np.isnan(ent32[9])
    assert np.abs(ent32[keep] - ent[keep]).max() <= 1e-4


@pytest.mark.parametrize("hid", [0, 8])
def test_linear_identity_is_the_literal_group_means(hid):
    """mean_g log p - mean log p = ((mean_g h - mean h) . Wo) - (mean_g lse - mean lse), float64,
    on the two-regions model's own layers; overlapping groups."""
    Xtr, _, Xdev, _ = R.two_regions_data()
    X = Xdev[:60]
    rng = np.random.default_rng(3)
    mus = (R.MELBOURNES[np.arange(4) % 2] + rng.standard_normal((4, 2))).astype(np.float32)
    init = R.two_regions_init([mus, np.full((4, 2), 1.0, np.float32),
                               np.zeros(4, np.float32)], hid)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in zip(R.names(hid), init)}
    x = torch.tensor(X, dtype=torch.float64)
    h = R.bigaus(x, p["mus"], p["sigmas"], p["corxy"])
    if hid:
        h = torch.relu(h @ p["Wh"] + p["bh"])
    Z = R.logits_of(x, p).numpy()
    ptr = np.array([0, 30, 60, 120])
    rows = np.concatenate([np.arange(0, 60, 2), np.arange(1, 60, 2), np.arange(60)])
    lin = A.region_scores_linear(h.numpy(), p["Wo"].numpy(), p["bo"].numpy(), ptr, rows)
    e = np.exp(Z - Z.max(axis=1, keepdims=True))     # float64 logits: nothing rounded on the way
    logp = np.log(e / e.sum(axis=1, keepdims=True))
    lit = np.stack([logp[r].mean(axis=0) - logp.mean(axis=0) for r in A.groups_of(ptr, rows)])
    assert lin.shape == lit.shape == (3, 20)
    assert np.abs(lin - lit).max() <= 1e-12
    assert np.abs(lin[2]).max() <= 1e-12   # the group of all rows is the global mean


# -- the ABI ---------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_built():
    from graphconvgeo_amd import _build, _native
    header = open(os.path.join(ROOT, "include", "gcg_spmm.h")).read()
    for name in ENTRIES:
        assert name + "(" in header and name in _native.SIGNATURES
    assert any(os.path.basename(s) == "vocab_stats.hip" for s in _build.SOURCES)


def test_abi_argument_validation_without_gpu(native_lib):
    lib = native_lib
    a, b, c, d = (C.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000))
    odd4, odd8 = C.c_void_p(0x10002), C.c_void_p(0x20004)
    lse = lib.gcg_row_lse_f64
    assert lse(4, 0, a, 4, b, None) == 1                               # N = 0
    assert lse(4, (1 << 24) + 1, a, 1 << 25, b, None) == 1             # N > 2^24
    assert b"2^24" in lib.gcg_last_error() and b"gcg_row_lse_f64" in lib.gcg_last_error()
    assert lse(-1, 8, a, 8, b, None) == 1                              # negative M
    assert lse(4, 8, a, 7, b, None) == 1                               # ldl < N
    assert lse(4, 8, None, 8, b, None) == 1                            # null operands
    assert lse(4, 8, a, 8, None, None) == 1
    assert lse(4, 8, odd4, 8, b, None) == 2                            # a misaligned base
    assert lse(4, 8, a, 8, odd8, None) == 2
    assert lse(0, 8, None, 8, None, None) == 0                         # M == 0: no launch
    cs = lib.gcg_softmax_column_stats_f64
    assert cs(4, 0, a, 4, b, c, d, None) == 1
    assert cs(4, (1 << 24) + 1, a, 1 << 25, b, c, d, None) == 1
    assert b"gcg_softmax_column_stats_f64" in lib.gcg_last_error()
    assert cs(-1, 8, a, 8, b, c, d, None) == 1
    assert cs(4, 8, a, 7, b, c, d, None) == 1
    for args in ((None, 8, b, c, d), (a, 8, None, c, d), (a, 8, b, None, d), (a, 8, b, c, None)):
        assert cs(4, 8, *args, None) == 1
    for args in ((odd4, 8, b, c, d), (a, 8, odd8, c, d), (a, 8, b, odd8, d), (a, 8, b, c, odd8)):
        assert cs(4, 8, *args, None) == 2
    assert cs(0, 8, None, 8, None, None, None, None) == 0


# -- the wrappers' and the validations' errors ---------------------------------------------------
def test_wrappers_and_validations_refuse_on_the_host():
    from graphconvgeo_amd import loc2lang as L
    z = torch.zeros((3, 4))
    f64 = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(TypeError, match="torch tensor"):
        L.row_lse(np.zeros((3, 4), np.float32))
    with pytest.raises(TypeError, match="torch tensor"):
        L.softmax_column_stats(np.zeros((3, 4), np.float32), f64[:3], f64, f64.clone())
    with pytest.raises(ValueError, match="no CPU fallback"):
        L.row_lse(z)
    with pytest.raises(ValueError, match="no CPU fallback"):
        L.softmax_column_stats(z, f64[:3], f64, f64.clone())
    assert np.array_equal(L.check_words([3, 0, 3, 19], 20), [3, 0, 3, 19])
    assert L.check_words([], 20).size == 0 and L.check_words([1], 20).dtype == np.int64
    for words in ([0, 20], [-1], [[0, 1]], [0.5], 3):
        with pytest.raises(ValueError, match="words"):
            L.check_words(words, 20)
    ptr, rows = L.check_groups([0, 2, 5], [4, 0, 0, 1, 4], 5)     # overlapping: fine
    assert ptr.tolist() == [0, 2, 5] and rows.dtype == np.int64
    with pytest.raises(ValueError, match="monotone"):
        L.check_groups([0, 3, 2, 5], [0, 1, 2, 3, 4], 5)
    with pytest.raises(ValueError, match="monotone"):
        L.check_groups([1, 5], [0, 1, 2, 3, 4], 5)
    with pytest.raises(ValueError, match="monotone"):
        L.check_groups([0, 4], [0, 1, 2, 3, 4], 5)
    with pytest.raises(ValueError, match="empty"):
        L.check_groups([0, 2, 2, 5], [0, 1, 2, 3, 4], 5)
    for bad in ([0, 5, 1], [0, -1, 1]):
        with pytest.raises(ValueError, match="outside"):
            L.check_groups([0, 3], bad, 5)
    with pytest.raises(ValueError, match="integer"):
        L.check_groups([0, 2], [0.0, 1.0], 5)
    s = torch.zeros((2, 10))
    with pytest.raises(ValueError, match=r"\[G, V\]"):
        L.region_recall(torch.zeros(10), [0, 1], [0])
    with pytest.raises(ValueError, match="gold_ptr"):
        L.region_recall(s, [0, 1], [0])                # G + 1 entries
    with pytest.raises(ValueError, match="monotone"):
        L.region_recall(s, [0, 2, 1], [0])
    with pytest.raises(ValueError, match="outside"):
        L.region_recall(s, [0, 1, 2], [0, 10])
    with pytest.raises(ValueError, match="twice"):
        L.region_recall(s, [0, 2, 2], [3, 3])
    with pytest.raises(ValueError, match="fractions"):
        L.region_recall(s, [0, 1, 2], [0, 1], fractions=(1.5,))


# -- region_recall ---------------------------------------------------------------------------------
def check_recall(scores, gold_ptr, gold_word, fractions):
    from graphconvgeo_amd import loc2lang as L
    got = L.region_recall(torch.as_tensor(scores), gold_ptr, gold_word, fractions)
    ks, recall, oracle, per_group, ranks = A.region_recall(scores, gold_ptr, gold_word, fractions)
    assert got.ks == ks
    assert np.array_equal(got.ranks, ranks)
    assert np.array_equal(got.per_group, per_group, equal_nan=True)
    assert np.allclose(got.recall, recall, rtol=0, atol=1e-15, equal_nan=True)
    assert np.allclose(got.oracle, oracle, rtol=0, atol=1e-15, equal_nan=True)
    return got


def test_region_recall_is_the_literal_ranking_on_cpu_tensors():
    """Random scores (V = 200, five groups, one without gold words), float32 and float64, a
    NumPy array as well as a tensor."""
    from graphconvgeo_amd import loc2lang as L
    rng = np.random.default_rng(8)
    scores = rng.standard_normal((5, 200)).astype(np.float32)
    sizes = [7, 0, 31, 1, 12]
    gold_ptr = np.concatenate([[0], np.cumsum(sizes)])
    gold_word = np.concatenate([rng.choice(200, size=n, replace=False) for n in sizes])
    got = check_recall(scores, gold_ptr, gold_word, (0.01, 0.05, 0.1, 0.15, 0.2))
    assert got.ks == [2, 10, 20, 30, 40]
    assert np.isnan(got.per_group[:, 1]).all() and not np.isnan(got.per_group[:, 0]).any()
    assert got.oracle[0] == np.mean([2 / 7, 2 / 31, 1.0, 2 / 12])
    check_recall(scores.astype(np.float64), gold_ptr, gold_word, (0.5, 1.0))
    again = L.region_recall(scores, gold_ptr, gold_word)
    assert again.ranks.tolist() == got.ranks.tolist() and again.recall == got.recall
    # every word gold, k = V: everything is found, and the ranks are a permutation
    full = L.region_recall(scores[:1], [0, 200], np.arange(200), fractions=(1.0,))
    assert full.recall == [1.0] and sorted(full.ranks.tolist()) == list(range(200))


def test_region_recall_ties_overlap_empty_groups_and_k_zero():
    """Equal scores at a gold word and at a higher and a lower index: the higher index ranks
    before it, the lower after it (reversed stable argsort). Two groups share gold words and
    score rows; a group without gold words is skipped; int(f V) = 0 retrieves nothing."""
    #            0    1    2    3    4    5    6    7    8    9
    row = [2.0, 5.0, 2.0, 9.0, 2.0, 1.0, 5.0, 0.0, 2.0, 7.0]
    scores = np.array([row, row, row[::-1], row], np.float32)
    gold_ptr = [0, 3, 3, 5, 8]
    gold_word = [2, 4, 1, 2, 9, 4, 2, 3]       # groups 0 and 3 overlap in words 2 and 4
    got = check_recall(scores, gold_ptr, gold_word, (0.05, 0.3, 0.5, 0.7))
    assert got.ks == [0, 3, 5, 7]
    # row: 9 (3), 7 (9), 5 (6), 5 (1), then the 2s at 8, 4, 2, 0
    assert got.ranks[:3].tolist() == [6, 5, 3]
    assert got.ranks[5:].tolist() == [5, 6, 0]
    assert np.isnan(got.per_group[:, 1]).all()
    assert got.per_group[0].tolist()[0] == 0.0 and got.recall[0] == 0.0 and got.oracle[0] == 0.0
    assert got.per_group[:, 0].tolist() == [0.0, 0.0, 1 / 3, 1.0]
    assert got.per_group[:, 3].tolist() == [0.0, 1 / 3, 1 / 3, 1.0]
    # no covered group at all: NaN means, no ranks
    none = check_recall(scores[:1], [0, 0], [], (0.5,))
    assert np.isnan(none.recall[0]) and none.ranks.size == 0
