"""Timings of the TF-IDF features (graphconvgeo_amd.tfidf, csrc/tfidf.hip) on one MI355X.

Synthetic corpora, seed 77: every document has 100 tokens drawn from a Zipf law over the raw
terms (term ids are a random permutation of the frequency ranks, so neither the ids nor the
sorted names follow the frequencies), DataLoader's thresholds (min_df 10, max_df 0.2, binary, idf,
l2).

  twitter-us      450k documents, 500k raw terms
  twitter-world   1.4M documents, 2M raw terms

Per size, one JSON line with
  fit_device_tokens_ms   TfidfFeatures.fit_transform_tokens from token arrays already in HBM and
                         the rank array already computed: the device half
  fit_host_tokens_ms     the same from host arrays (adds the host -> device copy of the tokens)
  rank_host_ms           term_ranks(terms): the one host sort of the vocabulary a fit also pays
  names_host_ms          feature_names_ and vocabulary_ of the kept terms, built on first use
  df_atomic_ms / df_ordered_ms   the fit with either way of accumulating document frequencies
  torch_ms               the same features from a torch composition on the device (unique over
                         64-bit keys, bincount, indexing, index_add_); checked equal
  host_s                 the same from the same arrays on the host: scipy coo -> csr with
                         sum_duplicates, numpy pruning, sklearn's TfidfTransformer (float64);
                         checked equal in structure, values within 1 float32 ulp
  tokenise_host_s        tokenize_corpus on a sample of joined documents, scaled to the corpus: what
                         the host spends before the device sees a token
--profile-once runs one fit and exits (for a kernel trace in a run of its own).

--tokenise adds a second line per size, {"op": "tokenise", ...}: the corpus as texts (the token
ids written out as their terms, 8 bytes each; --multibyte-share S renames that share of the terms
to start with a 2- or 3-byte character), tokenised by
  host_s                 tokenize_corpus on a sample of the documents, scaled to the corpus (the
                         host tokeniser is linear in the documents; the whole corpus takes minutes)
  device_s               tokenize_corpus_device on the whole corpus, wall time, median of --reps
  device_split_s         one more run with a synchronisation after each stage: prep_s (lower, join,
                         encode), upload_s, kernels_s (mark, spans, hash, sort, verify, number,
                         remap and their readbacks), terms_s (the distinct terms' strings, the stop
                         list, the action array)
  equal_on_sample        the device's (doc_ptr, tokens, terms) on the sample equal the host's
--tokenise-only skips the fits. --profile-once with --tokenise runs one warmed tokenisation.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphconvgeo_amd import tfidf  # noqa: E402

SIZES = {"twitter-us": (450_000, 100, 500_000), "twitter-world": (1_400_000, 100, 2_000_000)}
DEFAULTS = dict(min_df=10, max_df=0.2, norm="l2", use_idf=True, binary=True, sublinear_tf=False)


def corpus(n_docs, per_doc, n_terms, dev, seed=77):
    """(doc_ptr host, tokens device int32, terms): drawn on the device, seeded."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    cdf = torch.cumsum(1.0 / torch.arange(1, n_terms + 1, dtype=torch.float64, device=dev), 0)
    cdf /= cdf[-1].clone()
    ident = torch.randperm(n_terms, generator=g, device=dev).to(torch.int32)
    tokens = torch.empty(n_docs * per_doc, dtype=torch.int32, device=dev)
    step = 1 << 24
    for s in range(0, tokens.numel(), step):
        u = torch.rand(min(step, tokens.numel() - s), generator=g, device=dev, dtype=torch.float64)
        r = torch.searchsorted(cdf, u).clamp_(max=n_terms - 1)
        tokens[s:s + r.numel()] = ident[r]
    doc_ptr = np.arange(n_docs + 1, dtype=np.int64) * per_doc
    # names whose sorted order is neither the id nor the frequency order
    terms = [f"w{(i * 7919) % n_terms:07d}" for i in range(n_terms)]
    return doc_ptr, tokens, terms


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, [round(t * 1e3, 2) for t in ts]


def torch_composition(doc_ptr_dev, tokens, rank, n_docs, V, lo, hi):
    """The DataLoader-default features from torch ops on the device."""
    lens = doc_ptr_dev[1:] - doc_ptr_dev[:-1]
    doc = torch.repeat_interleave(torch.arange(n_docs, device=tokens.device), lens,
                                  output_size=tokens.numel())
    key = doc * V + rank[tokens.long()].long()
    uniq = torch.unique(key)
    rows, cols = uniq // V, uniq % V
    df = torch.bincount(cols, minlength=V)
    keep = (df >= lo) & (df <= hi)
    new_id = torch.cumsum(keep, 0) - 1
    sel = keep[cols]
    rows, cols = rows[sel], new_id[cols[sel]]
    indptr = torch.zeros(n_docs + 1, dtype=torch.int64, device=tokens.device)
    torch.cumsum(torch.bincount(rows, minlength=n_docs), 0, out=indptr[1:])
    idf = torch.log((1.0 + n_docs) / (1.0 + df[keep].double())) + 1.0
    x = idf[cols]
    sq = torch.zeros(n_docs, dtype=torch.float64, device=tokens.device).index_add_(0, rows, x * x)
    vals = (x / torch.sqrt(sq)[rows]).float()
    return indptr.int(), cols.int(), vals


def host_baseline(doc_ptr, tokens, rank, n_docs, V, lo, hi):
    import scipy.sparse as sps
    from sklearn.feature_extraction.text import TfidfTransformer

    t0 = time.perf_counter()
    rows = np.repeat(np.arange(n_docs, dtype=np.int32), np.diff(doc_ptr))
    X = sps.csr_matrix((np.ones(tokens.size, np.float64), (rows, rank[tokens])), shape=(n_docs, V))
    X.sum_duplicates()
    df = np.bincount(X.indices, minlength=V)
    X = X[:, np.flatnonzero((df >= lo) & (df <= hi))]
    X.data.fill(1.0)
    X = TfidfTransformer(norm="l2", use_idf=True).fit_transform(X)
    X.sort_indices()
    return time.perf_counter() - t0, X


def ulp(a, b):
    a = a.view(np.int32).astype(np.int64)
    b = b.view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max()) if a.size else 0


def tokenise_share(terms, tokens, per_doc, n_docs, sample=20_000):
    tok = tokens[: sample * per_doc].cpu().numpy().reshape(sample, per_doc)
    names = np.asarray(terms, dtype=object)
    docs = [" ".join(names[row]) for row in tok]
    tfidf.tokenize_corpus(docs[:10])  # the stop list's import is not tokenising
    t0 = time.perf_counter()
    tfidf.tokenize_corpus(docs)
    return (time.perf_counter() - t0) * n_docs / sample


_B36 = np.frombuffer(b"0123456789abcdefghijklmnopqrstuvwxyz", np.uint8)


def term_bytes(n_terms, multibyte_share, seed=78):
    """uint8 [n_terms, 9]: term i as 8 bytes of UTF-8 and a space. 'w' and 7 base-36 digits of
    i, or for a `multibyte_share` of the terms (drawn at random) a 2-byte letter and 6 digits or
    a 3-byte letter and 5: every term as many bytes, so the corpus is one gather."""
    ids = np.arange(n_terms, dtype=np.int64)
    digits = np.stack([_B36[(ids // 36 ** k) % 36] for k in range(6, -1, -1)], 1)
    out = np.full((n_terms, 9), ord(" "), np.uint8)
    out[:, 0] = ord("w")
    out[:, 1:8] = digits
    kind = np.zeros(n_terms, np.int8)
    multi = np.random.default_rng(seed).random(n_terms) < multibyte_share
    kind[multi] = 1 + (ids[multi] % 2)
    for k, lead in ((1, "\u00e9".encode()), (2, "\u65e5".encode())):   # e-acute, a CJK letter
        assert 36 ** (7 - k) >= n_terms
        out[kind == k, :len(lead)] = np.frombuffer(lead, np.uint8)
    return out


def text_corpus(tokens_host, per_doc, table, first=0, count=None):
    """The documents first .. first + count as str, from the token ids and term_bytes."""
    n_docs = tokens_host.size // per_doc
    count = n_docs - first if count is None else count
    docs, step = [], 1 << 16
    for d in range(first, first + count, step):
        e = min(d + step, first + count)
        rows = table[tokens_host[d * per_doc:e * per_doc]].reshape(e - d, per_doc * 9)
        docs.extend(bytes(r).decode("utf-8") for r in rows)
    return docs


def same_tokens(a, b):
    return bool(np.array_equal(a[0], b[0]) and a[2] == b[2] and
                np.array_equal(torch.as_tensor(a[1]).cpu().numpy(), torch.as_tensor(b[1]).cpu().numpy()))


def run_tokenise(name, dev, reps, multibyte_share, sample=20_000):
    n_docs, per_doc, V = SIZES[name]
    _, tokens, _ = corpus(n_docs, per_doc, V, dev)
    tokens_host = tokens.cpu().numpy()
    del tokens
    table = term_bytes(V, multibyte_share)
    docs = text_corpus(tokens_host, per_doc, table)
    rec = {"op": "tokenise", "config": name, "documents": n_docs, "tokens": int(tokens_host.size),
           "raw_terms": V, "multibyte_share": multibyte_share,
           "text_bytes": n_docs * per_doc * 9 + n_docs - 1}
    part = docs[:sample]
    tfidf.tokenize_corpus(part[:10])  # the stop list's import is not tokenising
    t0 = time.perf_counter()
    want = tfidf.tokenize_corpus(part)
    rec["host_s"] = round((time.perf_counter() - t0) * n_docs / sample, 2)
    rec["host_sample_documents"] = sample
    rec["equal_on_sample"] = same_tokens(tfidf.tokenize_corpus_device(part, device=dev), want)
    out = {}
    ms, all_ms = timed(lambda: out.__setitem__("r", tfidf.tokenize_corpus_device(docs, device=dev)),
                       reps)
    rec.update(device_s=round(ms * 1e-3, 3), device_all_s=[round(t * 1e-3, 3) for t in all_ms])
    split = {}
    allocs = torch.cuda.memory_stats(dev).get("num_device_alloc", 0)
    tfidf.tokenize_corpus_device(docs, device=dev, timings=split)
    rec["device_split_s"] = {k: round(v, 3) for k, v in split.items()}
    # allocations the caching allocator passed on to the driver during that run (they are slow)
    rec["device_split_driver_allocs"] = torch.cuda.memory_stats(dev).get("num_device_alloc", 0) - allocs
    doc_ptr, toks, terms = out["r"]
    rec.update(kept_tokens=int(doc_ptr[-1]), terms=len(terms),
               fallbacks=tfidf.tokenize_corpus_device.fallbacks)
    # the device's ids are the corpus' own terms in order of first appearance
    first_seen = np.unique(tokens_host, return_index=True)
    order = first_seen[0][np.argsort(first_seen[1], kind="stable")]
    rec["terms_equal_corpus"] = bool(
        len(terms) == order.size and
        terms == [bytes(r[:8]).decode("utf-8") for r in table[order]])
    t0 = time.perf_counter()
    vec = tfidf.TfidfFeatures(device=dev, tokenizer="device", **DEFAULTS)
    X = vec.fit_transform(docs)
    torch.cuda.synchronize()
    rec.update(fit_transform_texts_s=round(time.perf_counter() - t0, 3),
               fit_transform_tokenize_s=round(vec.tokenize_s_, 3), features=X.shape[1])
    print(json.dumps(rec), flush=True)


def run(name, dev, host: bool, reps: int):
    n_docs, per_doc, V = SIZES[name]
    doc_ptr, tokens, terms = corpus(n_docs, per_doc, V, dev)
    t0 = time.perf_counter()
    rank_host = tfidf.term_ranks(terms)
    rank_ms = (time.perf_counter() - t0) * 1e3
    tokens_host = tokens.cpu().numpy()
    out = {}

    def fit(tok):
        vec = tfidf.TfidfFeatures(device=dev, **DEFAULTS)
        out["X"], out["vec"] = vec.fit_transform_tokens(doc_ptr, tok, terms, rank=rank_host), vec

    rec = {"op": "tfidf", "config": name, "documents": n_docs, "tokens": int(tokens.numel()),
           "raw_terms": V, "rank_host_ms": round(rank_ms, 1)}
    modes = {}
    for _ in range(2):  # the two ways of accumulating df, alternating
        for mode in ("atomic", "ordered"):
            tfidf.DF_MODE = mode
            modes.setdefault(mode, []).append(timed(lambda: fit(tokens), reps)[0])
    rec.update(df_atomic_ms=[round(t, 2) for t in modes["atomic"]],
               df_ordered_ms=[round(t, 2) for t in modes["ordered"]])
    tfidf.DF_MODE = DEFAULT_DF_MODE
    ms, all_ms = timed(lambda: fit(tokens), reps)
    rec.update(df_mode=tfidf.DF_MODE, fit_device_tokens_ms=round(ms, 2), fit_device_tokens_all_ms=all_ms)
    ms, all_ms = timed(lambda: fit(tokens_host), reps)
    rec.update(fit_host_tokens_ms=round(ms, 2), fit_host_tokens_all_ms=all_ms)
    X, vec = out["X"], out["vec"]
    t0 = time.perf_counter()
    n_names = len(vec.vocabulary_)
    rec["names_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    assert n_names == X.shape[1]
    rec.update(features=X.shape[1], nnz=X.nnz,
               tokens_per_s=round(tokens.numel() / (rec["fit_device_tokens_ms"] * 1e-3), 1))
    lo, hi = tfidf.df_bounds(DEFAULTS["min_df"], DEFAULTS["max_df"], n_docs)
    rank_dev = torch.from_numpy(rank_host).to(dev)
    ptr_dev = torch.from_numpy(doc_ptr).to(dev)
    comp = lambda: out.__setitem__("T", torch_composition(ptr_dev, tokens, rank_dev, n_docs, V, lo, hi))
    ms, all_ms = timed(comp, reps)
    ptr, idx, val = out["T"]
    rec.update(torch_ms=round(ms, 2), torch_all_ms=all_ms,
               torch_equal_structure=bool(torch.equal(ptr, X.indptr) and torch.equal(idx, X.indices)),
               torch_max_ulp=ulp(val.cpu().numpy(), X.data.cpu().numpy()))
    del out["T"], ptr, idx, val
    rec["tokenise_host_s"] = round(tokenise_share(terms, tokens, per_doc, n_docs), 2)
    if host:
        host_s, Xh = host_baseline(doc_ptr, tokens_host, rank_host, n_docs, V, lo, hi)
        rec.update(host_s=round(host_s, 2),
                   host_equal_structure=bool(np.array_equal(Xh.indptr, X.indptr.cpu().numpy()) and
                                             np.array_equal(Xh.indices, X.indices.cpu().numpy())),
                   host_max_ulp=ulp(Xh.data.astype(np.float32), X.data.cpu().numpy()))
    print(json.dumps(rec), flush=True)


DEFAULT_DF_MODE = tfidf.DF_MODE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="twitter-us,twitter-world")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the scipy / sklearn baseline")
    ap.add_argument("--df-mode", default=DEFAULT_DF_MODE, choices=sorted(tfidf.DF_MODES),
                    help="--profile-once: how the traced fit accumulates document frequencies")
    ap.add_argument("--tokenise", action="store_true",
                    help="also time tokenising the corpus as texts, host against device")
    ap.add_argument("--tokenise-only", action="store_true", help="--tokenise without the fits")
    ap.add_argument("--multibyte-share", type=float, default=0.0,
                    help="--tokenise: the share of the terms that start with a 2- or 3-byte "
                         "character (the rest are ASCII)")
    ap.add_argument("--profile-once", action="store_true",
                    help="one warmed fit of the first size and nothing else (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tfidf needs the GPU: there is no host path to time")
    dev = torch.device("cuda")
    if args.profile_once and (args.tokenise or args.tokenise_only):
        n_docs, per_doc, V = SIZES[args.sizes.split(",")[0]]
        tokens_host = corpus(n_docs, per_doc, V, dev)[1].cpu().numpy()
        docs = text_corpus(tokens_host, per_doc, term_bytes(V, args.multibyte_share))
        for _ in range(2):
            tfidf.tokenize_corpus_device(docs, device=dev)
        torch.cuda.synchronize()
        return
    if args.profile_once:
        tfidf.DF_MODE = args.df_mode
        n_docs, per_doc, V = SIZES[args.sizes.split(",")[0]]
        doc_ptr, tokens, terms = corpus(n_docs, per_doc, V, dev)
        rank = tfidf.term_ranks(terms)
        for _ in range(2):
            tfidf.TfidfFeatures(device=dev, **DEFAULTS).fit_transform_tokens(doc_ptr, tokens, terms,
                                                                             rank=rank)
        torch.cuda.synchronize()
        return
    for name in args.sizes.split(","):
        if not args.tokenise_only:
            run(name, dev, not args.no_host, args.reps)
        if args.tokenise or args.tokenise_only:
            run_tokenise(name, dev, args.reps, args.multibyte_share)


if __name__ == "__main__":
    main()
