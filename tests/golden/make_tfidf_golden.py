"""Generate the TF-IDF fixtures (run in the build container, never on the GPU box).

python tests/golden/make_tfidf_golden.py  ->  tests/golden/tfidf_small.npz, tfidf_dataloader.npz

tfidf_small.npz: a seeded corpus (about 300 train and 60 dev documents over about 400
Zipf-distributed terms; every 17th document empty, one of 1,500 tokens, documents whose every
term is pruned, out-of-vocabulary tokens in the dev part) and, for five configurations, sklearn's
own TfidfVectorizer(dtype=np.float64) output cast to float32, its feature names, idf_ and the dev
transform.

tfidf_dataloader.npz: the reference's own data.DataLoader.tfidf() (data.py:378-397), imported
with make_golden.py's shims, on synthetic user tables; it runs sklearn's float32 path. Beside its
output the float64-cast values and the measured largest ulp distance between the two
(`ulp_f32_path`) are stored. Only data is written; no reference source is copied.
"""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import pandas as pd
from sklearn.feature_extraction.text import TfidfVectorizer

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import import_reference_data_module  # noqa: E402
from tfidf_reference import ulp_distance  # noqa: E402

TOKEN_PATTERN = r"(?u)(?<![#@])\b\w\w+\b"
CONFIGS = [
    dict(binary=True, sublinear_tf=False, use_idf=True, norm="l2", min_df=10, max_df=0.2),
    dict(binary=True, sublinear_tf=True, use_idf=True, norm="l2", min_df=10, max_df=0.1),
    dict(binary=False, sublinear_tf=True, use_idf=True, norm="l2", min_df=2, max_df=0.5),
    dict(binary=False, sublinear_tf=False, use_idf=False, norm="l1", min_df=1, max_df=1.0),
    dict(binary=False, sublinear_tf=False, use_idf=True, norm=None, min_df=3, max_df=40),
]
EXTRAS = ["the", "and", "THE", "#tagged", "@someone", "a", "I", "x9", "42", "2019", "été", "naïve",
          "Straße", "Mixed", "CASE"]


def term_names(rng, n_terms, prefix="w"):
    """Term names whose sorted order is not their frequency order, and their Zipf law."""
    names = np.array([f"{prefix}{rng.integers(0, 10**6):06d}x{i}" for i in range(n_terms)])
    p = 1.0 / np.arange(1, n_terms + 1)
    return names, p / p.sum()


def zipf_corpus(rng, n_docs, names, p, mean_len):
    """Documents of Zipf-distributed terms with uppercase, tags, mentions, stop words, digits,
    one-letter words and non-ASCII letters mixed in."""
    docs = []
    for d in range(n_docs):
        if d % 17 == 16:
            docs.append("")
            continue
        toks = list(rng.choice(names, size=max(1, rng.poisson(mean_len)), p=p))
        for _ in range(rng.integers(0, 4)):
            toks.append(EXTRAS[rng.integers(0, len(EXTRAS))])
        if rng.random() < 0.3:
            toks = [t.upper() if rng.random() < 0.2 else t for t in toks]
        rng.shuffle(toks)
        docs.append(" ".join(toks))
    return docs


def small_corpus(seed=77):
    rng = np.random.default_rng(seed)
    names, p = term_names(rng, 400)
    train = zipf_corpus(rng, 300, names, p, 30)
    train[5] = " ".join(rng.choice(names, size=1500, p=p))      # one long document
    train[40] = "onlyhere onlyhere alsoonlyhere"                   # every term below min_df 2
    train[41] = f"{names[0]} {names[0]} {names[1]}"                 # every term above max_df 0.5
    dev = zipf_corpus(rng, 60, names, p, 30)
    dev = [" ".join(t if rng.random() < 0.9 else f"oov{rng.integers(0, 50)}" for t in doc.split())
           for doc in dev]
    dev[3] = "neverseen1 neverseen2 @mention #tag"
    return train, dev


def csr_arrays(prefix, m):
    m = m.tocsr()
    m.sum_duplicates()  # canonical: sorted, unique columns
    return {f"{prefix}_indptr": m.indptr.astype(np.int32), f"{prefix}_indices": m.indices.astype(np.int32),
            f"{prefix}_data": m.data}


def make_small():
    train, dev = small_corpus()
    out = {"text_train": np.array("\n".join(train)), "text_dev": np.array("\n".join(dev)),
           "configs": np.array(json.dumps(CONFIGS))}
    for i, cfg in enumerate(CONFIGS, 1):
        vec = TfidfVectorizer(token_pattern=TOKEN_PATTERN, stop_words="english", ngram_range=(1, 1),
                              dtype=np.float64, **cfg)
        X = vec.fit_transform(train)
        D = vec.transform(dev)
        assert X.dtype == np.float64
        pre = f"c{i}"
        tr = csr_arrays(pre + "_train", X)
        dv = csr_arrays(pre + "_dev", D)
        tr[pre + "_train_data"] = tr[pre + "_train_data"].astype(np.float32)
        dv[pre + "_dev_data"] = dv[pre + "_dev_data"].astype(np.float32)
        out.update(tr)
        out.update(dv)
        out[pre + "_feature_names"] = np.array(vec.get_feature_names_out().tolist())
        out[pre + "_idf"] = vec.idf_.astype(np.float64) if cfg["use_idf"] else np.zeros(0)
        out[pre + "_df"] = np.bincount(X.indices, minlength=X.shape[1]).astype(np.int64)
        empty = int((np.diff(X.indptr) == 0).sum())
        print(f"config {i}: {X.shape[1]} features, nnz {X.nnz}, {empty} empty rows, dev nnz {D.nnz}")
    np.savez_compressed(os.path.join(HERE, "tfidf_small.npz"), **out)


def user_tables(seed=78):
    rng = np.random.default_rng(seed)
    names, p = term_names(rng, 300, prefix="u")
    docs = zipf_corpus(rng, 320, names, p, 40)
    users = [f"user{i:04d}" for i in range(len(docs))]
    df = pd.DataFrame({"user": users, "lat": 40.0 + rng.random(len(docs)),
                       "lon": -100.0 + rng.random(len(docs)), "text": docs}).set_index("user")
    perm = rng.permutation(len(df))
    parts = [df.iloc[np.sort(perm[:220])], df.iloc[np.sort(perm[220:270])], df.iloc[np.sort(perm[270:])]]
    return [q.sort_index() for q in parts]


def make_dataloader():
    data = import_reference_data_module()
    dl = data.DataLoader(data_home="")
    dl.df_train, dl.df_dev, dl.df_test = user_tables()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # sklearn 1.7.2 warns about dtype='float32' as a string
        dl.tfidf()
    parts = {"train": dl.X_train, "dev": dl.X_dev, "test": dl.X_test}
    assert all(m.dtype == np.float32 for m in parts.values())
    # the same vectorizer in float64, cast: what the device is held to within 1 ulp
    v64 = TfidfVectorizer(token_pattern=dl.token_pattern, use_idf=dl.idf, norm=dl.norm,
                          binary=dl.btf, sublinear_tf=dl.subtf, min_df=dl.mindf, max_df=dl.maxdf,
                          ngram_range=(1, 1), stop_words=dl.stops, dtype=np.float64)
    texts = {"train": dl.df_train.text.values, "dev": dl.df_dev.text.values,
             "test": dl.df_test.text.values}
    cast = {"train": v64.fit_transform(texts["train"]), "dev": v64.transform(texts["dev"]),
            "test": v64.transform(texts["test"])}
    assert v64.get_feature_names_out().tolist() == dl.vectorizer.get_feature_names_out().tolist()
    out, ulp = {}, 0
    for name in parts:
        a, b = csr_arrays(name, parts[name]), csr_arrays(name + "64", cast[name])
        assert np.array_equal(a[name + "_indices"], b[name + "64_indices"])
        assert np.array_equal(a[name + "_indptr"], b[name + "64_indptr"])
        c = b[name + "64_data"].astype(np.float32)
        ulp = max(ulp, ulp_distance(a[name + "_data"], c))
        out.update(a)
        out[name + "_data_f64cast"] = c
        out["text_" + name] = np.array("\n".join(texts[name]))
    out["feature_names"] = np.array(dl.vectorizer.get_feature_names_out().tolist())
    out["ulp_f32_path"] = np.int64(ulp)
    np.savez_compressed(os.path.join(HERE, "tfidf_dataloader.npz"), **out)
    print(f"dataloader: {dl.X_train.shape} train, {dl.X_dev.shape[0]} dev, {dl.X_test.shape[0]} test, "
          f"ulp_f32_path = {ulp}")


if __name__ == "__main__":
    make_small()
    make_dataloader()
