"""TF-IDF without a GPU: the numpy restatement (tests/tfidf_reference.py) against the fixtures
and live sklearn, the host tokeniser against sklearn's analyzer, the vocabulary order, the
min_df / max_df boundaries, and the argument checks of the C-ABI entries (csrc/tfidf.hip)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import tfidf_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TFIDF_ENTRIES = ("gcg_tfidf_count_workspace_bytes", "gcg_tfidf_count",
                 "gcg_tfidf_select_workspace_bytes", "gcg_tfidf_select", "gcg_tfidf_idf_f64",
                 "gcg_tfidf_compact_workspace_bytes", "gcg_tfidf_compact", "gcg_tfidf_weight_f32")


@pytest.fixture(scope="module")
def small():
    z = np.load(os.path.join(GOLDEN, "tfidf_small.npz"))
    return z, json.loads(str(z["configs"])), str(z["text_train"]).split("\n"), \
        str(z["text_dev"]).split("\n")


def _fit(train, dev, cfg):
    from graphconvgeo_amd.tfidf import tokenize_corpus

    doc_ptr, tokens, terms = tokenize_corpus(train)
    fit = ref.fit_transform(doc_ptr, tokens, terms, **cfg)
    vocab = {t: i for i, t in enumerate(fit["feature_names"])}
    dptr, dtok, none = tokenize_corpus(dev, vocabulary=vocab)
    assert none is None
    kw = {k: cfg[k] for k in ("norm", "use_idf", "binary", "sublinear_tf")}
    return fit, ref.transform(dptr, dtok, fit["idf"], **kw)


@pytest.mark.parametrize("i", range(1, 6))
def test_restatement_equals_fixture(small, i):
    z, configs, train, dev = small
    cfg = configs[i - 1]
    fit, dv = _fit(train, dev, cfg)
    assert fit["feature_names"] == z[f"c{i}_feature_names"].tolist()
    assert np.array_equal(fit["df"], z[f"c{i}_df"])
    for got, part in ((fit, "train"), (dv, "dev")):
        assert np.array_equal(got["indptr"], z[f"c{i}_{part}_indptr"])
        assert np.array_equal(got["indices"], z[f"c{i}_{part}_indices"])
        assert np.array_equal(got["data"].view(np.int32), z[f"c{i}_{part}_data"].view(np.int32))
    if cfg["use_idf"]:
        assert np.array_equal(fit["idf"], z[f"c{i}_idf"])


@pytest.mark.parametrize("i", range(1, 6))
def test_restatement_equals_live_sklearn(small, i):
    text = pytest.importorskip("sklearn.feature_extraction.text")
    z, configs, train, dev = small
    cfg = configs[i - 1]
    vec = text.TfidfVectorizer(token_pattern=r"(?u)(?<![#@])\b\w\w+\b", stop_words="english",
                               dtype=np.float64, **cfg)
    X, D = vec.fit_transform(train).tocsr(), vec.transform(dev).tocsr()
    fit, dv = _fit(train, dev, cfg)
    assert fit["feature_names"] == vec.get_feature_names_out().tolist()
    for got, m in ((fit, X), (dv, D)):
        m.sum_duplicates()
        assert np.array_equal(got["indptr"], m.indptr) and np.array_equal(got["indices"], m.indices)
        assert ref.ulp_distance(got["data"], m.data.astype(np.float32)) == 0


def test_tokeniser_is_sklearns_analyzer():
    text = pytest.importorskip("sklearn.feature_extraction.text")
    from graphconvgeo_amd.tfidf import TOKEN_PATTERN, tokenize_corpus

    docs = ["The QUICK brown #fox and @Dog saw a I 42 x9 2019 été Straße naïve the THE fox_2 it's",
            "", "   ", "#only @tags", "fox fox Fox", "über-cool co-op e.g. a.b"]
    analyze = text.TfidfVectorizer(token_pattern=TOKEN_PATTERN, stop_words="english").build_analyzer()
    doc_ptr, tokens, terms = tokenize_corpus(docs)
    assert doc_ptr.dtype == np.int64 and tokens.dtype == np.int32 and doc_ptr[0] == 0
    for d, doc in enumerate(docs):
        assert [terms[t] for t in tokens[doc_ptr[d]:doc_ptr[d + 1]]] == analyze(doc)
    assert terms[:3] == ["quick", "brown", "saw"]  # first-seen order, stop words and tags gone
    # a fitted vocabulary gives final ids, -1 outside it
    vocab = {"fox": 0, "quick": 1}
    _, final, none = tokenize_corpus(docs, vocabulary=vocab)
    assert none is None and set(final.tolist()) == {-1, 0, 1}
    assert final[doc_ptr[4]:doc_ptr[5]].tolist() == [0, 0, 0]
    # an explicit stop list, and none at all
    assert tokenize_corpus(["aa bb cc"], stop_words=["bb"])[2] == ["aa", "cc"]
    assert tokenize_corpus(["the aa"], stop_words=None)[2] == ["the", "aa"]
    with pytest.raises(ValueError, match="stop list"):
        tokenize_corpus(["aa"], stop_words="klingon")


def test_vocabulary_order_is_sorted(small):
    from graphconvgeo_amd.tfidf import term_ranks, tokenize_corpus

    _, _, train, _ = small
    _, _, terms = tokenize_corpus(train)
    rank = term_ranks(terms)
    assert sorted(rank.tolist()) == list(range(len(terms)))
    by_rank = [None] * len(terms)
    for t, r in zip(terms, rank):
        by_rank[r] = t
    assert by_rank == sorted(terms) and by_rank != terms
    # code-point order: Z < a < aa < b < é
    assert term_ranks(["b", "a", "é", "Z", "aa"]).tolist() == [3, 1, 4, 0, 2]


def _corpus_with_dfs(dfs, n_docs):
    """Token arrays in which term t is in the first dfs[t] of n_docs documents."""
    docs = [[t for t, f in enumerate(dfs) if d < f] for d in range(n_docs)]
    doc_ptr = np.zeros(n_docs + 1, np.int64)
    np.cumsum([len(d) for d in docs], out=doc_ptr[1:])
    return doc_ptr, np.asarray([t for d in docs for t in d], np.int32)


def test_threshold_boundaries():
    from graphconvgeo_amd.tfidf import df_bounds

    n = 47                                    # 0.2 * 47 = 9.4: floor 9
    assert df_bounds(3, 0.2, n) == (3, 9) == ref.df_bounds(3, 0.2, n)
    assert df_bounds(0.1, 1.0, n) == (5, 47)  # 4.7: ceil 5; 1.0 is a share, not a count
    assert df_bounds(1, 1, n) == (1, 1)       # an integral max_df is a count
    assert df_bounds(0.2, 0.2, 50) == (10, 10)
    with pytest.raises(ValueError, match="max_df corresponds to < documents than min_df"):
        df_bounds(10, 0.2, 47)
    with pytest.raises(ValueError):
        df_bounds(-1, 0.2, 47)
    with pytest.raises(ValueError):
        df_bounds(1, 1.5, 47)
    dfs = [2, 3, 4, 9, 10, 47]                # min_df 3, max_df 0.2: 3, 4 and 9 stay
    terms = [f"t{i}" for i in range(len(dfs))]
    doc_ptr, tokens = _corpus_with_dfs(dfs, n)
    fit = ref.fit_transform(doc_ptr, tokens, terms, min_df=3, max_df=0.2)
    assert fit["feature_names"] == ["t1", "t2", "t3"] and fit["df"].tolist() == [3, 4, 9]
    text = pytest.importorskip("sklearn.feature_extraction.text")
    docs = [" ".join(terms[t] for t in tokens[doc_ptr[d]:doc_ptr[d + 1]]) for d in range(n)]
    vec = text.TfidfVectorizer(min_df=3, max_df=0.2).fit(docs)
    assert vec.get_feature_names_out().tolist() == ["t1", "t2", "t3"]
    with pytest.raises(ValueError, match="After pruning, no terms remain"):
        ref.fit_transform(doc_ptr, tokens, terms, min_df=11, max_df=0.9)


def test_tfidf_entries_are_declared_bound_and_built():
    from graphconvgeo_amd import _build, _native

    root = os.path.dirname(os.path.dirname(GOLDEN))
    header = open(os.path.join(root, "include", "gcg_spmm.h")).read()
    for name in TFIDF_ENTRIES:
        assert name + "(" in header and name in _native.SIGNATURES
    assert any(os.path.basename(s) == "tfidf.hip" for s in _build.SOURCES)


def test_tfidf_abi_argument_validation_without_gpu(native_lib):
    lib = native_lib
    a, b, c, d, e = (C.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))
    odd = C.c_void_p(0x10004)
    nbytes = C.c_size_t(7)

    def failed(status, fn, code=1):
        assert status == code, (fn, status)
        assert fn.encode() in lib.gcg_last_error()

    ws_bytes = lib.gcg_tfidf_count_workspace_bytes
    failed(ws_bytes(-1, 10, 5, C.byref(nbytes)), "gcg_tfidf_count_workspace_bytes")
    assert nbytes.value == 0
    failed(ws_bytes(4, -1, 5, C.byref(nbytes)), "gcg_tfidf_count_workspace_bytes")
    failed(ws_bytes(4, 10, 0, C.byref(nbytes)), "gcg_tfidf_count_workspace_bytes")
    failed(ws_bytes(4, 2**31, 5, C.byref(nbytes)), "gcg_tfidf_count_workspace_bytes")
    failed(ws_bytes(4, 10, 5, None), "gcg_tfidf_count_workspace_bytes")
    count = lib.gcg_tfidf_count
    ok = (a, b, None, c, d, e, 10, a, b, 0, c, d, 1 << 20, None)  # doc_ptr .. stream
    failed(count(-1, 5, 10, *ok), "gcg_tfidf_count")
    failed(count(4, 0, 10, *ok), "gcg_tfidf_count")
    failed(count(4, 5, -1, *ok), "gcg_tfidf_count")
    failed(count(4, 5, 10, None, *ok[1:]), "gcg_tfidf_count")                     # no doc_ptr
    failed(count(4, 5, 10, a, None, *ok[2:]), "gcg_tfidf_count")                  # no tokens
    failed(count(4, 5, 10, a, b, None, c, None, e, *ok[6:]), "gcg_tfidf_count")   # half an output
    failed(count(4, 5, 10, a, b, None, c, d, e, 10, None, *ok[8:]), "gcg_tfidf_count")  # no nnz_dev
    failed(count(4, 5, 10, a, b, None, c, d, e, -1, *ok[7:]), "gcg_tfidf_count")  # capacity
    failed(count(4, 5, 10, a, b, None, c, d, e, 10, a, b, 2, *ok[10:]), "gcg_tfidf_count")  # df_mode
    failed(count(4, 5, 10, a, b, None, c, d, e, 10, a, b, 0, None, d, 1 << 20, None),
           "gcg_tfidf_count")                                                     # no status_dev
    failed(count(4, 5, 10, a, b, None, c, d, e, 10, a, b, 0, c, None, 0, None), "gcg_tfidf_count")
    failed(count(4, 5, 10, odd, *ok[1:]), "gcg_tfidf_count", 2)                   # doc_ptr 8-B
    select = lib.gcg_tfidf_select
    failed(lib.gcg_tfidf_select_workspace_bytes(0, C.byref(nbytes)), "gcg_tfidf_select_workspace_bytes")
    failed(select(0, a, 1, 5, b, c, d, e, 1 << 20, None), "gcg_tfidf_select")
    failed(select(5, None, 1, 5, b, c, d, e, 1 << 20, None), "gcg_tfidf_select")
    failed(select(5, a, 1, 5, b, c, None, e, 1 << 20, None), "gcg_tfidf_select")
    failed(select(5, odd, 1, 5, b, c, d, e, 1 << 20, None), "gcg_tfidf_select", 2)
    idf = lib.gcg_tfidf_idf_f64
    failed(idf(-1, a, 10, b, None), "gcg_tfidf_idf_f64")
    failed(idf(5, a, -1, b, None), "gcg_tfidf_idf_f64")
    failed(idf(5, None, 10, b, None), "gcg_tfidf_idf_f64")
    failed(idf(5, a, 10, odd, None), "gcg_tfidf_idf_f64", 2)
    assert idf(0, None, 10, None, None) == 0
    compact = lib.gcg_tfidf_compact
    failed(lib.gcg_tfidf_compact_workspace_bytes(-1, C.byref(nbytes)),
           "gcg_tfidf_compact_workspace_bytes")
    failed(compact(-1, 5, 10, a, b, c, d, e, None, None, 0, a, 1 << 20, None), "gcg_tfidf_compact")
    failed(compact(4, 5, -1, a, b, c, d, e, None, None, 0, a, 1 << 20, None), "gcg_tfidf_compact")
    failed(compact(4, 5, 10, None, b, c, d, e, None, None, 0, a, 1 << 20, None), "gcg_tfidf_compact")
    failed(compact(4, 5, 10, a, b, c, d, e, a, None, 10, None, 0, None), "gcg_tfidf_compact")
    failed(compact(4, 5, 10, a, b, c, d, e, None, None, 0, None, 0, None), "gcg_tfidf_compact")
    failed(compact(4, 5, 10, a, b, c, d, e, a, b, -1, None, 0, None), "gcg_tfidf_compact")
    weight = lib.gcg_tfidf_weight_f32
    failed(weight(-1, 5, 10, a, b, c, d, 1, 0, 2, e, None), "gcg_tfidf_weight_f32")
    failed(weight(4, 0, 10, a, b, c, d, 1, 0, 2, e, None), "gcg_tfidf_weight_f32")
    failed(weight(4, 5, 10, a, b, c, d, 1, 0, 3, e, None), "gcg_tfidf_weight_f32")   # norm
    failed(weight(4, 5, 10, None, b, c, d, 1, 0, 2, e, None), "gcg_tfidf_weight_f32")
    failed(weight(4, 5, 10, a, b, c, d, 1, 0, 2, None, None), "gcg_tfidf_weight_f32")
    failed(weight(4, 5, 10, a, b, c, odd, 1, 0, 2, e, None), "gcg_tfidf_weight_f32", 2)
    assert weight(0, 5, 0, None, None, None, None, 1, 0, 2, None, None) == 0
