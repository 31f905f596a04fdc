"""Float64 numpy restatement of sklearn's TfidfVectorizer at ngram_range (1, 1), smooth_idf, over
token ids: what graphconvgeo_amd.tfidf computes on the device, written the way sklearn spells it
(CountVectorizer._count_vocab / _sort_features / _limit_features, TfidfTransformer.fit /
transform, sklearn.preprocessing.normalize). The only rounding to float32 is the last cast."""
import numpy as np


def count_csr(doc_ptr, tokens, n_terms):
    """Canonical count CSR (indptr, indices, counts) of the documents; ids outside [0, n_terms)
    are dropped. The keys doc * n_terms + term are Python-sized int64."""
    doc_ptr = np.asarray(doc_ptr, np.int64)
    tokens = np.asarray(tokens, np.int64)
    n_docs = len(doc_ptr) - 1
    doc = np.repeat(np.arange(n_docs, dtype=np.int64), np.diff(doc_ptr))
    ok = (tokens >= 0) & (tokens < n_terms)
    key, counts = np.unique(doc[ok] * np.int64(n_terms) + tokens[ok], return_counts=True)
    rows, indices = key // n_terms, key % n_terms
    indptr = np.zeros(n_docs + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n_docs), out=indptr[1:])
    return indptr.astype(np.int32), indices.astype(np.int32), counts.astype(np.int32)


def weight(indptr, indices, counts, idf, binary, sublinear_tf, use_idf, norm):
    """TfidfTransformer.transform on a count CSR, float64; returns float32 values."""
    x = np.ones(len(counts), np.float64) if binary else counts.astype(np.float64)
    if sublinear_tf:
        x = np.log(x) + 1.0
    if use_idf:
        x = x * idf[indices]
    if norm in ("l1", "l2"):
        for r in range(len(indptr) - 1):
            s, e = indptr[r], indptr[r + 1]
            total = 0.0
            for v in x[s:e]:  # inplace_csr_row_normalize_*: a running sum in storage order
                total += v * v if norm == "l2" else abs(v)
            if norm == "l2":
                total = np.sqrt(total)
            if total != 0.0:
                x[s:e] /= total
    return x.astype(np.float32)


def df_bounds(min_df, max_df, n_docs):
    """The integer df range CountVectorizer._limit_features keeps."""
    import numbers

    hi = max_df if isinstance(max_df, numbers.Integral) else max_df * n_docs
    lo = min_df if isinstance(min_df, numbers.Integral) else min_df * n_docs
    if hi < lo:
        raise ValueError("max_df corresponds to < documents than min_df")
    return int(np.ceil(lo)), int(np.floor(hi))


def fit_transform(doc_ptr, tokens, terms, min_df=10, max_df=0.2, norm="l2", use_idf=True,
                  binary=True, sublinear_tf=False):
    """dict(indptr, indices, data, df, idf, feature_names) from provisional ids into `terms`."""
    terms = list(terms)
    order = sorted(range(len(terms)), key=terms.__getitem__)
    rank = np.empty(len(terms), np.int64)
    rank[order] = np.arange(len(terms))
    tokens = np.asarray(tokens, np.int64)
    mapped = np.where((tokens >= 0) & (tokens < len(terms)), rank[np.clip(tokens, 0, len(terms) - 1)],
                      -1)
    indptr, indices, counts = count_csr(doc_ptr, mapped, len(terms))
    n_docs = len(doc_ptr) - 1
    df = np.bincount(indices, minlength=len(terms)).astype(np.int64)
    lo, hi = df_bounds(min_df, max_df, n_docs)
    keep = (df >= lo) & (df <= hi)
    if not keep.any():
        raise ValueError("After pruning, no terms remain. Try a lower min_df or a higher max_df.")
    new_id = np.cumsum(keep) - 1
    sel = keep[indices]
    row = np.repeat(np.arange(n_docs), np.diff(indptr))[sel]
    out_indptr = np.zeros(n_docs + 1, np.int64)
    np.cumsum(np.bincount(row, minlength=n_docs), out=out_indptr[1:])
    out_indices = new_id[indices[sel]].astype(np.int32)
    out_counts = counts[sel]
    kept_df = df[keep]
    idf = np.log((1.0 + n_docs) / (1.0 + kept_df.astype(np.float64))) + 1.0
    data = weight(out_indptr, out_indices, out_counts, idf, binary, sublinear_tf, use_idf, norm)
    names = [terms[i] for i in np.asarray(order)[keep]]
    return dict(indptr=out_indptr.astype(np.int32), indices=out_indices, data=data, df=kept_df,
                idf=idf, feature_names=names)


def transform(doc_ptr, tokens, idf, norm="l2", use_idf=True, binary=True, sublinear_tf=False):
    """dict(indptr, indices, data) from final ids (columns of the fitted vocabulary)."""
    indptr, indices, counts = count_csr(doc_ptr, tokens, len(idf))
    data = weight(indptr.astype(np.int64), indices, counts, idf, binary, sublinear_tf, use_idf, norm)
    return dict(indptr=indptr, indices=indices, data=data)


def ulp_distance(a, b):
    """Largest distance in float32 units in the last place between two float32 arrays."""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, np.int64(-2**31) - a, a)
    b = np.where(b < 0, np.int64(-2**31) - b, b)
    return int(np.abs(a - b).max()) if a.size else 0
