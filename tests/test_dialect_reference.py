"""CPU side of the dialect-embedding evaluation (graphconvgeo_amd.dialect, csrc/neighbours.hip):
the NumPy restatement (tests/dialect_reference.py) against the committed sklearn fixtures
(tests/golden/dialect_*.npz, written by tests/golden/make_dialect_golden.py) and, where sklearn
is installed, against a live run; the lexicon, its pairs and the recalls on a hand-written DARE
file; the ABI's argument checks and every ValueError of the Python layer. None needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import dialect_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DARE = os.path.join(GOLDEN, "dialect_dare.jsonl")
CASES = ("small", "medium", "wide")
ENTRIES = ("gcg_neighbours_tile", "gcg_minmax_l1_rows_f32_workspace_bytes",
           "gcg_minmax_l1_rows_f32", "gcg_neighbour_ranks_f32_workspace_bytes",
           "gcg_neighbour_ranks_f32", "gcg_kneighbors_f32_workspace_bytes", "gcg_kneighbors_f32")
# the vocabulary of the hand-written case: rows 0 .. 9
VOCAB = ["the", "south", "yall", "pop", "maine, new hampshire", "coke", "wicked", "midland",
         "fixin", "soda"]


def load(name):
    return np.load(os.path.join(GOLDEN, f"dialect_{name}.npz"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_sklearn_fixture(name):
    g = load(name)
    assert g["embs"].dtype == np.float32 and g["gap"] >= 1e-6
    assert np.array_equal(g["embs"][:, [0]], ref.gaussian_embeddings(*g["embs"].shape, int(g["seed"]))[:, [0]])
    scaled = ref.scale(g["embs"])
    assert np.abs(scaled - g["scaled"]).max() <= 1e-15
    v = scaled.shape[0]
    dist, idx = ref.kneighbors(g["scaled"], g["rows"], v)
    assert np.array_equal(idx, g["indices"])
    # sklearn expands |x|^2 + |y|^2 - 2 x.y: a distance of 0 comes back as sqrt(a few ulps of |x|^2)
    assert np.abs(dist - g["distances"]).max() <= 1e-6 * g["distances"].max()
    # ranks are the inverse of the ordering, and the query's own row comes first
    pair_ptr = np.arange(len(g["rows"]) + 1) * v
    pair_word = np.tile(np.arange(v), len(g["rows"]))
    ranks = ref.neighbour_ranks(g["scaled"], g["rows"], pair_ptr, pair_word).reshape(-1, v)
    for q, row in enumerate(g["rows"]):
        assert np.array_equal(g["indices"][q][ranks[q]], np.arange(v)) and ranks[q][row] == 0


def test_restatement_against_a_live_sklearn_run():
    pytest.importorskip("sklearn")
    from sklearn.neighbors import NearestNeighbors
    from sklearn.preprocessing import MinMaxScaler, normalize
    x = ref.gaussian_embeddings(250, 20, seed=5)
    x[7] = x[:, :].min(axis=0)  # a row that scales to all zeros keeps its zeros
    rows = np.array([3, 100, 249])
    sk = normalize(MinMaxScaler(feature_range=(0, 1)).fit_transform(x.astype(np.float64)), norm="l1")
    mine = ref.scale(x)
    assert np.abs(mine - sk).max() <= 1e-15 and not mine[7].any()
    assert ref.min_relative_gap(mine, rows) >= 1e-6  # no index hangs on the form of the distance
    dist, idx = NearestNeighbors(n_neighbors=250, algorithm="brute").fit(sk).kneighbors(sk[rows])
    my_dist, my_idx = ref.kneighbors(mine, rows, 250)
    assert np.array_equal(idx, my_idx)
    assert np.abs(dist - my_dist).max() <= 1e-6 * dist.max()


def test_restatement_rules():
    e = np.array([[0.0, 0.0], [3.0, 4.0], [0.0, 0.0], [3.0, 4.0], [1.0, 0.0]])
    order, d2 = ref.ordering(e, e[1])
    assert d2.tolist() == [25.0, 0.0, 25.0, 0.0, 20.0] and order.tolist() == [1, 3, 4, 0, 2]
    assert ref.ranks_of(e, e[3]).tolist() == [3, 0, 4, 1, 2]  # a duplicate of the query: by index
    assert ref.neighbour_ranks(e, [3, 0], [0, 2, 3], [1, 1, 4]).tolist() == [0, 0, 2]
    dist, idx = ref.kneighbors(e, np.array([[3.0, 4.0]]), 3)
    assert idx.tolist() == [[1, 3, 4]] and dist[0].tolist() == [0.0, 0.0, np.sqrt(20.0)]
    lo, hi = ref.rank_bounds(d2, 4, ref.gamma(2))
    assert (lo, hi) == (2, 3)
    lo, hi = ref.rank_bounds(d2, 2, ref.gamma(2))   # tied with row 0: either may come first
    assert (lo, hi) == (3, 5)
    s = ref.scale(np.array([[1.0, 5.0, 2.0], [3.0, 5.0, 2.0], [2.0, 5.0, 4.0]]))
    assert s.tolist() == [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0 / 3.0, 0.0, 2.0 / 3.0]]
    assert ref.gamma(64) == pytest.approx(66 * 2.0 ** -24, rel=1e-5)


def test_lexicon_pairs_and_recalls_by_hand():
    from graphconvgeo_amd import dialect as dl
    lex = dl.DialectLexicon.from_dare_json(DARE)
    # "South" / "Midland" / "Pop" / "Yall" / "Ayuh" are lowercased; New England files under its
    # lowercased subregions; texas is not in the vocabulary
    assert lex.words == {"south": {"yall", "fixin", "coke", "buggy"},
                         "maine, new hampshire": {"wicked", "ayuh"},
                         "texas": {"tump"}, "midland": {"pop", "gumband"}}
    p = lex.pairs(VOCAB)
    assert p.dialects == ["maine, new hampshire", "midland", "south"]
    assert p.rows.tolist() == [4, 7, 1]
    assert p.pair_ptr.tolist() == [0, 1, 2, 5] and p.pair_word.tolist() == [6, 3, 2, 5, 8]
    assert p.n_missing.tolist() == [1, 1, 1]   # ayuh, gumband, buggy: counted, never found
    ranks = np.array([1, 5, 0, 2, 7])
    rec = dl.recall_at_k(ranks, p.pair_ptr, p.n_missing, ks=[1, 3, 8])
    assert rec.ks == [1, 3, 8] and rec.totals.tolist() == [2, 2, 4]
    assert rec.micro == [12.5, 37.5, 62.5]
    assert rec.per_dialect.tolist() == [[0.0, 0.0, 25.0], [50.0, 0.0, 50.0], [50.0, 50.0, 75.0]]
    micro, per = ref.recall_at_k(ranks, p.pair_ptr, p.n_missing, [1, 3, 8])
    assert micro == rec.micro and np.array_equal(per, rec.per_dialect)
    # a lexicon from a mapping keeps its keys; a dialect without gold words is skipped (NaN)
    lex2 = dl.DialectLexicon({"south": ["yall", "nope"], "the": []})
    p2 = lex2.pairs(VOCAB)
    assert p2.dialects == ["south", "the"] and p2.pair_ptr.tolist() == [0, 1, 1]
    rec2 = dl.recall_at_k(np.array([4]), p2.pair_ptr, p2.n_missing, [5])
    assert rec2.micro == [50.0] and rec2.per_dialect[0, 0] == 50.0 and np.isnan(rec2.per_dialect[0, 1])


def test_dialect_entries_are_declared_bound_and_built():
    from graphconvgeo_amd import _build, _native
    import graphconvgeo_amd
    header = open(os.path.join(ROOT, "include", "gcg_spmm.h")).read()
    for name in ENTRIES:
        assert name + "(" in header and name in _native.SIGNATURES
    assert any(os.path.basename(s) == "neighbours.hip" for s in _build.SOURCES)
    assert "dialect" in graphconvgeo_amd.__all__


def test_dialect_abi_argument_validation_without_gpu(native_lib):
    lib = native_lib
    a, b, c, d, e, f = (C.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000))
    odd = C.c_void_p(0x10002)  # not 4-B aligned
    ws = C.c_void_p(0x100000)
    nb = C.c_size_t(7)
    tiles = [lib.gcg_neighbours_tile(i) for i in range(8)]
    assert tiles == [256, 32, 8, 2048, 32, 1024, 1024, 8192] and lib.gcg_neighbours_tile(99) == 0
    assert lib.gcg_minmax_l1_rows_f32_workspace_bytes(5000, 64, C.byref(nb)) == 0
    assert nb.value >= 2 * 5 * 64 * 4 + 2 * 64 * 8
    assert lib.gcg_minmax_l1_rows_f32_workspace_bytes(-1, 64, C.byref(nb)) == 1
    assert lib.gcg_minmax_l1_rows_f32_workspace_bytes(5, 0, C.byref(nb)) == 1
    assert lib.gcg_minmax_l1_rows_f32_workspace_bytes(5, 4, None) == 1
    mm = lib.gcg_minmax_l1_rows_f32
    assert mm(5, 4, a, 3, b, 4, c, ws, 1 << 20, None) == 1           # lde < D
    assert mm(5, 4, a, 4, b, 3, c, ws, 1 << 20, None) == 1           # ldo < D
    assert mm(5, 4, a, 4, b, 4, None, ws, 1 << 20, None) == 1        # no status_dev
    assert b"status_dev" in lib.gcg_last_error()
    assert mm(5, 4, a, 4, b, 4, odd, ws, 1 << 20, None) == 2
    assert lib.gcg_kneighbors_f32_workspace_bytes(2000, 17, 50, C.byref(nb)) == 0
    assert nb.value >= 17 * 8 * 50 * 8
    assert lib.gcg_kneighbors_f32_workspace_bytes(2000, 17, 1025, C.byref(nb)) == 1
    assert lib.gcg_kneighbors_f32_workspace_bytes(20, 17, 21, C.byref(nb)) == 1
    kn = lib.gcg_kneighbors_f32
    assert kn(2000, 4, a, 4, 3, b, 4, 0, c, d, e, ws, 1 << 30, None) == 1     # k < 1
    assert kn(2000, 4, a, 4, 3, b, 4, 1025, c, d, e, ws, 1 << 30, None) == 1  # k > 1024
    assert b"1 <= k <= min(V, 1024)" in lib.gcg_last_error()
    assert kn(20, 4, a, 4, 3, b, 4, 21, c, d, e, ws, 1 << 30, None) == 1      # k > V
    assert kn(20, 4, a, 3, 3, b, 4, 2, c, d, e, ws, 1 << 30, None) == 1       # lde < D
    assert kn(20, 4, a, 4, 3, b, 4, 2, c, d, None, ws, 1 << 30, None) == 1    # no status_dev
    assert kn(20, 4, a, 4, 3, b, 4, 2, c, d, odd, ws, 1 << 30, None) == 2
    rk = lib.gcg_neighbour_ranks_f32
    assert rk(20, 4, a, 4, -1, b, 4, 5, c, d, e, f, ws, 1 << 30, None) == 1   # Q < 0
    assert rk(20, 4, a, 4, 3, b, 2, 5, c, d, e, f, ws, 1 << 30, None) == 1    # ldq < D
    assert rk(20, 4, a, 4, 3, b, 4, -5, c, d, e, f, ws, 1 << 30, None) == 1   # P < 0
    assert rk(20, 4, a, 4, 3, b, 4, 5, c, d, e, None, ws, 1 << 30, None) == 1  # no status_dev
    assert rk(20, 4, a, 4, 3, b, 4, 5, c, d, e, odd, ws, 1 << 30, None) == 2
    assert lib.gcg_neighbour_ranks_f32_workspace_bytes(3, -1, C.byref(nb)) == 1
    assert lib.gcg_neighbour_ranks_f32_workspace_bytes(3, 5, None) == 1


def test_python_layer_refuses_bad_input_without_gpu():
    from graphconvgeo_amd import dialect as dl
    good = np.arange(20.0, dtype=np.float32).reshape(5, 4)
    bad = good.copy()
    bad[3, 1] = np.nan
    ptr, word = np.array([0, 1, 2]), np.array([0, 4])
    lex = dl.DialectLexicon({"a": ["b", "c"]})
    vocab = ["a", "b", "c", "d", "e"]
    for call in (
            lambda: dl.scale_embeddings(np.zeros(5)),                                  # shape
            lambda: dl.scale_embeddings(np.zeros((5, 0))),
            lambda: dl.scale_embeddings(bad),                                          # non-finite
            lambda: dl.scale_embeddings(np.array([["a"]])),
            lambda: dl.scale_embeddings(good, device="cpu"),
            lambda: dl.kneighbors(good, good[:2], 0),                                  # k out of range
            lambda: dl.kneighbors(good, good[:2], 6),
            lambda: dl.kneighbors(np.zeros((2000, 2), np.float32), [0], 1025),
            lambda: dl.kneighbors(good, good[:2], 2.5),
            lambda: dl.kneighbors(good, good[:2, :3], 2),                              # shape mismatch
            lambda: dl.kneighbors(good, np.zeros((2, 2, 4)), 2),
            lambda: dl.kneighbors(good, bad[2:4], 2),
            lambda: dl.kneighbors(bad, good[:2], 2),
            lambda: dl.kneighbors(good, [0, 5], 2),                                    # a row outside embs
            lambda: dl.kneighbors(good, [-1], 2),
            lambda: dl.kneighbors(good, np.array([0.5]), 2),
            lambda: dl.neighbour_ranks(good, [0, 1], ptr, np.array([0, 5])),           # a word outside [0, V)
            lambda: dl.neighbour_ranks(good, [0, 1], ptr, np.array([-1, 0])),
            lambda: dl.neighbour_ranks(good, [0, 1], np.array([0, 2, 1]), word),       # non-monotone
            lambda: dl.neighbour_ranks(good, [0, 1], np.array([1, 1, 2]), word),
            lambda: dl.neighbour_ranks(good, [0, 1], np.array([0, 1, 3]), word),
            lambda: dl.neighbour_ranks(good, [0, 1], np.array([0, 2]), word),          # Q + 1 entries
            lambda: dl.neighbour_ranks(good, [0, 1], ptr, np.array([0.0, 1.0])),
            lambda: dl.neighbour_ranks(good, good[:2, :3], ptr, word),
            lambda: dl.neighbour_ranks(bad, [0, 1], ptr, word),
            lambda: dl.recall_at_k(np.array([0, 1]), np.array([0, 1]), [0], [1]),      # ptr[-1] != P
            lambda: dl.recall_at_k(np.array([0, 1]), ptr, [0], [1]),                   # n_missing shape
            lambda: dl.recall_at_k(np.array([0, 1]), ptr, [0, -1], [1]),
            lambda: dl.recall_at_k(np.array([0, 1]), ptr, [0, 0], []),
            lambda: dl.recall_at_k(np.array([0, 1]), ptr, [0, 0], [1.5]),
            lambda: dl.recall_at_k(np.zeros(0, int), np.array([0, 0]), [0], [1]),      # no gold word
            lambda: dl.eval_embeddings(vocab[:4], good, lex),                          # vocab size
            lambda: dl.eval_embeddings(vocab, bad, lex),
            lambda: dl.eval_embeddings(vocab, good, dl.DialectLexicon({"zz": ["a"]})),  # none covered
            lambda: dl.eval_embeddings(vocab, good, lex, ks=[-1]),
            lambda: dl.tile("nope")):
        with pytest.raises(ValueError):
            call()
