"""graphconvgeo_amd.tfidf on the GPU (csrc/tfidf.hip) against sklearn's own output
(tests/golden/tfidf_small.npz), the reference's DataLoader.tfidf (tfidf_dataloader.npz) and the
numpy restatement (tests/tfidf_reference.py).

Structure (indptr, indices, df_, the kept vocabulary and its order) is exact everywhere. Values:
at most 1 float32 ulp from the float64-cast fixtures -- the device's double log, sqrt and sum
order may differ from numpy's in the last double bit, which can move one float32 rounding and not
two -- and at most `ulp_f32_path` + 1 from the reference's float32 output, the bound read from
the fixture (sklearn's float32 path measured against the float64 one when it was generated)."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

import tfidf_reference as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def small():
    z = np.load(os.path.join(GOLDEN, "tfidf_small.npz"))
    return z, json.loads(str(z["configs"])), str(z["text_train"]).split("\n"), \
        str(z["text_dev"]).split("\n")


@pytest.fixture(scope="module")
def loader():
    z = np.load(os.path.join(GOLDEN, "tfidf_dataloader.npz"))
    return z, {p: str(z["text_" + p]).split("\n") for p in ("train", "dev", "test")}


def host(X):
    return X.indptr.cpu().numpy(), X.indices.cpu().numpy(), X.data.cpu().numpy()


def same_structure(X, indptr, indices):
    X.validate()
    got_ptr, got_idx, _ = host(X)
    assert got_ptr.dtype == np.int32 and got_idx.dtype == np.int32
    assert np.array_equal(got_ptr, indptr) and np.array_equal(got_idx, indices)


def bitwise(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(host(a), host(b)))


def zipf_tokens(seed, n_docs, n_terms, mean_len):
    """(doc_ptr, tokens, terms) with some empty documents and some ids out of range."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_terms + 1)
    lens = rng.poisson(mean_len, n_docs)
    lens[::17] = 0
    doc_ptr = np.zeros(n_docs + 1, np.int64)
    np.cumsum(lens, out=doc_ptr[1:])
    tokens = rng.choice(n_terms, size=int(doc_ptr[-1]), p=p / p.sum()).astype(np.int32)
    tokens[rng.random(tokens.size) < 0.02] = -1
    terms = [f"t{(i * 7919) % 10007:05d}_{i}" for i in range(n_terms)]  # sorted order != id order
    return doc_ptr, tokens, terms


def against_restatement(vec, X, want):
    same_structure(X, want["indptr"], want["indices"])
    assert vec.feature_names_ == want["feature_names"]
    assert np.array_equal(vec.df_.cpu().numpy(), want["df"])
    ulp = ref.ulp_distance(host(X)[2], want["data"])
    print("ulp against the restatement:", ulp)
    assert ulp <= 1


@pytest.mark.parametrize("i", range(1, 6))
def test_small_fixture_fit_and_transform(cuda, small, i):
    from graphconvgeo_amd.tfidf import TfidfFeatures

    z, configs, train, dev = small
    cfg = configs[i - 1]
    vec = TfidfFeatures(device=cuda, **cfg)
    X = vec.fit_transform(train)
    D = vec.transform(dev)
    names = z[f"c{i}_feature_names"].tolist()
    assert vec.feature_names_ == names
    assert vec.vocabulary_ == {t: k for k, t in enumerate(names)}
    assert np.array_equal(vec.df_.cpu().numpy(), z[f"c{i}_df"])
    assert X.shape == (len(train), len(names)) and D.shape == (len(dev), len(names))
    for got, part in ((X, "train"), (D, "dev")):
        same_structure(got, z[f"c{i}_{part}_indptr"], z[f"c{i}_{part}_indices"])
        ulp = ref.ulp_distance(host(got)[2], z[f"c{i}_{part}_data"])
        print(f"config {i} {part}: {ulp} ulp from sklearn's float64 output cast to float32")
        assert ulp <= 1
    if cfg["use_idf"]:
        # ln of the same quotient: numpy's and the device's are each within an ulp of it, the
        # quotient is >= 1 so that ulp is no larger than the result's, and the + 1 rounds once
        idf = vec.idf_.cpu().numpy()
        assert idf.dtype == np.float64
        assert np.max(np.abs(idf - z[f"c{i}_idf"]) / np.spacing(z[f"c{i}_idf"])) <= 3


def test_dataloader_fixture(cuda, loader):
    import pandas as pd

    from graphconvgeo_amd.tfidf import dataloader_features

    z, texts = loader
    frames = [pd.DataFrame({"text": texts[p]}) for p in ("train", "dev", "test")]
    X, vec = dataloader_features(*frames, device=cuda)
    assert vec.feature_names_ == z["feature_names"].tolist()
    bound = int(z["ulp_f32_path"]) + 1
    ptr = np.concatenate([z["train_indptr"], z["dev_indptr"][1:] + z["train_indptr"][-1],
                          z["test_indptr"][1:] + z["train_indptr"][-1] + z["dev_indptr"][-1]])
    same_structure(X, ptr, np.concatenate([z[p + "_indices"] for p in ("train", "dev", "test")]))
    data = host(X)[2]
    ulp64 = ref.ulp_distance(data, np.concatenate([z[p + "_data_f64cast"] for p in ("train", "dev", "test")]))
    ulp32 = ref.ulp_distance(data, np.concatenate([z[p + "_data"] for p in ("train", "dev", "test")]))
    print(f"dataloader: {ulp64} ulp from the float64 cast, {ulp32} ulp from the reference's "
          f"float32 output (bound {bound})")
    assert ulp64 <= 1
    assert ulp32 <= bound


def test_wide_keys(cuda):
    """70,000 one-token documents over 70,000 terms: document * n_terms passes 2^32."""
    from graphconvgeo_amd.tfidf import TfidfFeatures

    n = 70_000
    rng = np.random.default_rng(5)
    # a third of the terms twice, so a bound of two documents keeps something; ids not sorted
    tokens = np.concatenate([rng.permutation(n)[: n - n // 3], rng.permutation(n // 3)]).astype(np.int32)
    rng.shuffle(tokens)
    doc_ptr = np.arange(n + 1, dtype=np.int64)
    terms = [f"{(i * 7919) % n:05d}" for i in range(n)]
    assert len(set(terms)) == n
    cfg = dict(min_df=1, max_df=1.0, binary=False, sublinear_tf=True, norm="l2")
    vec = TfidfFeatures(device=cuda, **cfg)
    X = vec.fit_transform_tokens(doc_ptr, tokens, terms)
    against_restatement(vec, X, ref.fit_transform(doc_ptr, tokens, terms, **cfg))
    assert X.nnz == n and int(X.indices[-1]) == vec.vocabulary_[terms[tokens[-1]]]
    cfg["min_df"] = 2
    vec = TfidfFeatures(device=cuda, **cfg)
    X = vec.fit_transform_tokens(doc_ptr, tokens, terms)
    against_restatement(vec, X, ref.fit_transform(doc_ptr, tokens, terms, **cfg))


def test_edge_rows(cuda):
    from graphconvgeo_amd.tfidf import TfidfFeatures

    kw = dict(device=cuda, min_df=1, max_df=1.0, binary=False)
    # a corpus of one document
    vec = TfidfFeatures(**kw)
    X = vec.fit_transform_tokens([0, 4], np.asarray([2, 0, 2, 1], np.int32), ["b", "c", "a"])
    want = ref.fit_transform([0, 4], [2, 0, 2, 1], ["b", "c", "a"], min_df=1, max_df=1.0, binary=False)
    against_restatement(vec, X, want)
    assert vec.feature_names_ == ["a", "b", "c"] and host(X)[1].tolist() == [0, 1, 2]
    # one term, in some documents twice, some documents empty
    doc_ptr, tokens = np.asarray([0, 2, 2, 3, 3, 5]), np.zeros(5, np.int32)
    vec = TfidfFeatures(**kw)
    X = vec.fit_transform_tokens(doc_ptr, tokens, ["only"])
    against_restatement(vec, X, ref.fit_transform(doc_ptr, tokens, ["only"], min_df=1, max_df=1.0,
                                                  binary=False))
    assert host(X)[0].tolist() == [0, 1, 1, 2, 2, 3] and host(X)[2].tolist() == [1.0, 1.0, 1.0]
    # all tokens -1: an all-empty transform; and nothing left to fit on
    D = vec.transform_tokens(doc_ptr, np.full(5, -1, np.int32))
    D.validate()
    assert D.shape == (5, 1) and D.nnz == 0 and host(D)[0].tolist() == [0] * 6
    with pytest.raises(ValueError, match="After pruning, no terms remain"):
        TfidfFeatures(**kw).fit_transform_tokens(doc_ptr, np.full(5, -1, np.int32), ["only"])
    # a term in every document, cut by max_df
    doc_ptr, tokens, terms = zipf_tokens(3, 40, 12, 5)
    every = np.insert(tokens, doc_ptr[:-1], 11).astype(np.int32)
    doc_ptr = doc_ptr + np.arange(41)
    vec = TfidfFeatures(device=cuda, min_df=1, max_df=0.9)
    X = vec.fit_transform_tokens(doc_ptr, every, terms)
    assert terms[11] not in vec.vocabulary_
    against_restatement(vec, X, ref.fit_transform(doc_ptr, every, terms, min_df=1, max_df=0.9))
    # everything pruned, and bounds that cross
    with pytest.raises(ValueError, match="After pruning, no terms remain"):
        TfidfFeatures(device=cuda, min_df=39, max_df=0.99).fit_transform_tokens(doc_ptr, every, terms)
    with pytest.raises(ValueError, match="max_df corresponds to < documents than min_df"):
        TfidfFeatures(device=cuda, min_df=30, max_df=0.5).fit_transform_tokens(doc_ptr, every, terms)
    with pytest.raises(ValueError, match="empty vocabulary"):
        TfidfFeatures(device=cuda, min_df=1).fit_transform(["the and", "a"])
    with pytest.raises(ValueError, match="not fitted"):
        TfidfFeatures(device=cuda).transform(["aa"])


def test_chunking_df_modes_and_repeat_are_bitwise(cuda, monkeypatch):
    """The entry cap forced to 64 tokens (about 300 chunks), either way of accumulating the
    document frequencies, and a second run all give the bits of one chunk."""
    import torch

    from graphconvgeo_amd import tfidf

    doc_ptr, tokens, terms = zipf_tokens(11, 600, 500, 30)
    tokens[doc_ptr[7]:doc_ptr[8]] = tokens[doc_ptr[7]]  # one term many times
    long_doc = np.arange(200, dtype=np.int32) % 500     # a document above the cap
    tokens = np.concatenate([tokens, long_doc, long_doc[:30]])
    doc_ptr = np.concatenate([doc_ptr, doc_ptr[-1] + [200, 200, 230]])
    cfg = dict(min_df=3, max_df=0.3, binary=False, sublinear_tf=True)

    def run():
        vec = tfidf.TfidfFeatures(device=cuda, **cfg)
        X = vec.fit_transform_tokens(doc_ptr, tokens, terms)
        return vec, X, vec.transform_tokens(doc_ptr[:50], torch.as_tensor(tokens[:doc_ptr[49]] % 97).to(cuda))

    vec, X, D = run()
    against_restatement(vec, X, ref.fit_transform(doc_ptr, tokens, terms, **cfg))
    for cap, mode in ((tfidf.COUNT_CHUNK_ENTRIES, "atomic"), (64, "atomic"), (64, "ordered"),
                      (tfidf.COUNT_CHUNK_ENTRIES, "ordered")):
        monkeypatch.setattr(tfidf, "COUNT_CHUNK_ENTRIES", cap)
        monkeypatch.setattr(tfidf, "DF_MODE", mode)
        if cap == 64:
            assert len(tfidf.plan_chunks(doc_ptr, cap)) > 250
        vec2, X2, D2 = run()
        assert vec2.feature_names_ == vec.feature_names_ and torch.equal(vec2.df_, vec.df_)
        assert torch.equal(vec2.idf_, vec.idf_)
        assert bitwise(X, X2) and bitwise(D, D2), (cap, mode)


def test_count_sizing_call(cuda):
    """indptr = indices = counts = NULL: the call only moves the entry count on."""
    import ctypes as C

    import torch

    from graphconvgeo_amd import _native

    doc_ptr, tokens, _ = zipf_tokens(2, 90, 40, 12)
    want = len(ref.count_csr(doc_ptr, tokens, 40)[1])
    ptr, tok = torch.as_tensor(doc_ptr).to(cuda), torch.as_tensor(tokens).to(cuda)
    state = torch.tensor([5, 0], dtype=torch.int64, device=cuda)
    df = torch.zeros(40, dtype=torch.int64, device=cuda)
    ws, nbytes = _native.workspace("gcg_tfidf_count_workspace_bytes", cuda, 90, len(tokens), 40)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    _native.call("gcg_tfidf_count", 90, 40, len(tokens), p(ptr), p(tok), None, None, None, None, 0,
                 p(state), p(df), 0, p(state, 8), p(ws), nbytes,
                 C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))
    assert state.tolist() == [5 + want, 0] and int(df.sum()) == 0
    # and a capacity one entry short is reported, with nothing moved
    out = [torch.zeros(n, dtype=torch.int32, device=cuda) for n in (91, want, want)]
    _native.call("gcg_tfidf_count", 90, 40, len(tokens), p(ptr), p(tok), None, *(p(t) for t in out),
                 5 + want - 1, p(state), p(df), 0, p(state, 8), p(ws), nbytes,
                 C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))
    assert state.tolist() == [5 + want, 6]  # GCG_ERR_WORKSPACE in the status word
    assert int(out[1].sum()) == 0 and int(out[0].sum()) == 0


def test_vstack_equals_scipy(cuda):
    import torch

    from graphconvgeo_amd import sparse as gs

    a = sps.random(7, 13, density=0.3, random_state=1, format="csr", dtype=np.float32)
    b = sps.csr_matrix((0, 13), dtype=np.float32)                      # an empty part
    c = sps.random(9, 13, density=0.2, random_state=2, format="csr", dtype=np.float32).tolil()
    c[0, :] = 0
    c[4, :] = 0
    c[8, :] = 0                                                         # empty rows, first and last
    c = c.tocsr()
    c.eliminate_zeros()
    d = sps.csr_matrix((3, 13), dtype=np.float32)                      # rows, no entries
    parts = [a, b, c, d]
    want = sps.vstack(parts).tocsr()
    got = gs.vstack([gs.DeviceCSR.from_scipy(m, cuda) for m in parts])
    got.validate()
    assert got.shape == want.shape and got.nnz == want.nnz
    ptr, idx, data = host(got)
    assert np.array_equal(ptr, want.indptr) and np.array_equal(idx, want.indices)
    assert np.array_equal(data.view(np.int32), want.data.view(np.int32))
    assert isinstance(got.indptr, torch.Tensor) and got.indptr.dtype == torch.int32
    with pytest.raises(ValueError, match="width"):
        gs.vstack([got, gs.DeviceCSR.from_scipy(sps.csr_matrix((2, 5), dtype=np.float32), cuda)])
    with pytest.raises(ValueError):
        gs.vstack([])


def test_stacked_features_train_mlpconv_without_host_copy(cuda, loader, monkeypatch):
    import pandas as pd

    from graphconvgeo_amd import sparse as gs
    from graphconvgeo_amd.graph import normalize_edges_device
    from graphconvgeo_amd.mlpconv import MLPCONV
    from graphconvgeo_amd.tfidf import dataloader_features

    z, texts = loader
    frames = [pd.DataFrame({"text": texts[p]}) for p in ("train", "dev", "test")]
    X, _ = dataloader_features(*frames, device=cuda)
    n_tr, n_dev, n = len(texts["train"]), len(texts["dev"]), X.shape[0]
    rng = np.random.default_rng(4)
    H = normalize_edges_device(n, np.arange(n - 1), np.arange(1, n), cuda)
    Y = rng.integers(0, 4, n)
    monkeypatch.setattr(gs.DeviceCSR, "to_scipy", None)      # any host copy of X would trip
    monkeypatch.setattr(gs.DeviceCSR, "from_scipy", None)
    clf = MLPCONV(n_epochs=2, hidden_layer_size=8, device=cuda, seed=1)
    clf.fit(X, np.arange(n_tr), np.arange(n_tr, n_tr + n_dev), np.arange(n_tr + n_dev, n), Y, H)
    assert clf.Xd is X and len(clf.history) >= 1
    assert all(np.isfinite(h["train_loss"]) for h in clf.history)


def test_geolocate_pipeline_with_device_tfidf(cuda, monkeypatch, capsys):
    """The end-to-end example learns the task from features built on the device."""
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import geolocate_pipeline as gp

    monkeypatch.setattr(sys, "argv", ["geolocate_pipeline.py", "--users", "3000", "--epochs", "60",
                                      "--device-tfidf"])
    acc = gp.main()
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["tfidf"] == "device" and rec["features"] > 0
    assert acc > 0.5  # 12 regions: chance is 0.083
