"""DataLoader.tfidf (reference data.py:378-397) with the arithmetic on the GPU.

The split follows mentions.py. The host does what needs strings: `tokenize_corpus` restates
sklearn's analyzer at ngram_range (1, 1) (lowercase, token_pattern.findall, stop list) and owns
the term -> id dictionary. The device does what is arithmetic over ids (csrc/tfidf.hip): counting
chunks of whole documents into a canonical count CSR, document frequencies, the min_df / max_df
pruning with its column renumbering, and the tf-idf weighting with the row norm, in float64 with
one rounding to float32 at the store.

`TfidfFeatures` is the TfidfVectorizer of data.py:387-390 (DataLoader's defaults) returning a
`DeviceCSR`; `dataloader_features` is DataLoader.tfidf followed by the vstack of
tensormain.py:215: the X that MLPCONV.fit, MLP.fit, the mixture-density models and loc2lang
take. Out of scope: n-grams above 1, max_features, strip_accents, smooth_idf=False.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
import re

import numpy as np
import torch

from . import _native
from ._native import call
from .sparse import DeviceCSR, vstack

TOKEN_PATTERN = r"(?u)(?<![#@])\b\w\w+\b"  # data.py:256

# Tokens counted per gcg_tfidf_count call: a corpus with more is cut into chunks of whole
# documents (the sizes come from the host's doc_ptr, so a chunk boundary costs no
# synchronisation). 2^25 tokens need ~1 GB of keys, runs and sort temporary.
COUNT_CHUNK_ENTRIES = 1 << 25

# How gcg_tfidf_count accumulates the document frequencies: "atomic" = one integer atomic per
# entry, "ordered" = from a term-ordered copy of the chunk's columns. Both are exact. Measured on
# one MI355X (profiles/tfidf/): the atomics cost 5.9 ms of a 9.0 ms Twitter-US fit
# (the head of a Zipf vocabulary takes one add per document on one address), the second sort and
# its run lengths 1.1 ms.
DF_MODES = {"atomic": 0, "ordered": 1}
DF_MODE = "ordered"

_NORMS = {None: 0, "none": 0, "l1": 1, "l2": 2}


def _stop_set(stop_words):
    if stop_words is None:
        return frozenset()
    if isinstance(stop_words, str):
        if stop_words != "english":
            raise ValueError(f"not a built-in stop list: {stop_words!r}")
        try:
            from sklearn.feature_extraction.text import ENGLISH_STOP_WORDS
        except ImportError as e:
            raise ValueError('stop_words="english" is scikit-learn\'s ENGLISH_STOP_WORDS and '
                             "scikit-learn does not import here: pass the stop words as an "
                             "explicit collection (or None)") from e
        return ENGLISH_STOP_WORDS
    return frozenset(stop_words)


def tokenize_corpus(texts, token_pattern=TOKEN_PATTERN, stop_words="english", lowercase=True,
                    vocabulary=None):
    """(doc_ptr, tokens, terms): document d's tokens are tokens[doc_ptr[d]:doc_ptr[d + 1]].

    sklearn's analyzer at ngram_range (1, 1): lowercase, token_pattern.findall, drop the stop
    words. Without `vocabulary` the ids are provisional, in order of first appearance, and
    `terms` lists them (CountVectorizer._count_vocab's defaultdict). With a fitted `vocabulary`
    (term -> column) the ids are final, -1 for a term outside it, and `terms` is None."""
    pattern = re.compile(token_pattern)
    stops = _stop_set(stop_words)
    fixed = vocabulary is not None
    ids = vocabulary if fixed else {}
    doc_ptr = np.zeros(len(texts) + 1, np.int64)
    tokens = []
    for d, text in enumerate(texts):
        if isinstance(text, bytes):
            text = text.decode("utf-8")
        if not isinstance(text, str):
            raise ValueError(f"document {d} is not a string: {type(text).__name__}")
        for tok in pattern.findall(text.lower() if lowercase else text):
            if tok in stops:
                continue
            tokens.append(ids.get(tok, -1) if fixed else ids.setdefault(tok, len(ids)))
        doc_ptr[d + 1] = len(tokens)
    if len(tokens) >= 2**31:
        raise ValueError("too many tokens for int32 CSR")
    return doc_ptr, np.asarray(tokens, np.int32), None if fixed else list(ids)


def term_ranks(terms) -> np.ndarray:
    """rank[i] = position of terms[i] among the sorted terms (CountVectorizer._sort_features):
    one sort of the vocabulary; the device applies it to the tokens."""
    order = np.asarray(sorted(range(len(terms)), key=terms.__getitem__), np.int64)
    rank = np.empty(len(terms), np.int32)
    rank[order] = np.arange(len(terms), dtype=np.int32)
    return rank


def df_bounds(min_df, max_df, n_docs: int):
    """(lo, hi): a term is kept iff lo <= df <= hi, as CountVectorizer._limit_features decides
    it. An integral bound is a count; a float is a share of the documents compared as a float,
    df <= max_df * n and df >= min_df * n, which for an integer df is floor and ceil."""
    for name, x in (("min_df", min_df), ("max_df", max_df)):
        if isinstance(x, bool) or not isinstance(x, numbers.Real) or x < 0 or \
                (not isinstance(x, numbers.Integral) and x > 1.0):
            raise ValueError(f"{name} must be a count or a share in [0, 1], not {x!r}")
    hi = max_df if isinstance(max_df, numbers.Integral) else max_df * n_docs
    lo = min_df if isinstance(min_df, numbers.Integral) else min_df * n_docs
    if hi < lo:
        raise ValueError("max_df corresponds to < documents than min_df")
    return int(math.ceil(lo)), int(math.floor(hi))


def plan_chunks(doc_ptr: np.ndarray, cap: int):
    """[(first document, stop document)]: greedy runs of whole documents of at most `cap`
    tokens (a longer document is a chunk of its own)."""
    n = len(doc_ptr) - 1
    chunks, d = [], 0
    while d < n:
        e = int(np.searchsorted(doc_ptr, doc_ptr[d] + cap, side="right")) - 1
        e = min(max(e, d + 1), n)
        chunks.append((d, e))
        d = e
    return chunks


def _ptr(t, offset_bytes=0):
    return None if t is None else C.c_void_p(t.data_ptr() + offset_bytes)


def _host_doc_ptr(doc_ptr) -> np.ndarray:
    if isinstance(doc_ptr, torch.Tensor):
        doc_ptr = doc_ptr.cpu().numpy()
    doc_ptr = np.ascontiguousarray(doc_ptr, np.int64)
    if doc_ptr.ndim != 1 or doc_ptr.size < 1 or doc_ptr[0] != 0 or np.any(np.diff(doc_ptr) < 0):
        raise ValueError("doc_ptr must start at 0 and not decrease")
    return doc_ptr


class TfidfFeatures:
    """TfidfVectorizer(ngram_range=(1, 1), dtype float32) of data.py:387-390 on the GPU.

    fit_transform / transform take texts and return a DeviceCSR; fit_transform_tokens /
    transform_tokens take what tokenize_corpus returns (the token array may already be a device
    tensor). After a fit: vocabulary_ (term -> column) and feature_names_ (sorted), both built
    on first use, n_features_, df_ (int64 device tensor, the kept terms' document frequencies),
    idf_ (float64 device tensor), n_docs_."""

    def __init__(self, min_df=10, max_df=0.2, norm="l2", use_idf=True, binary=True,
                 sublinear_tf=False, token_pattern=TOKEN_PATTERN, stop_words="english",
                 device="cuda"):
        if norm not in _NORMS:
            raise ValueError(f"norm must be 'l2', 'l1' or None, not {norm!r}")
        self.min_df, self.max_df, self.norm = min_df, max_df, norm
        self.use_idf, self.binary, self.sublinear_tf = bool(use_idf), bool(binary), bool(sublinear_tf)
        self.token_pattern, self.stop_words = token_pattern, stop_words
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("the features are built on the GPU: device must be a CUDA (HIP) device")
        self.n_features_ = None
        self._names = self._vocabulary = None

    @property
    def feature_names_(self):
        """The kept terms in column (sorted) order; one readback of the renumbering, once."""
        self._require_fit()
        if self._names is None:
            kept = np.flatnonzero(self._new_id.cpu().numpy() >= 0)  # sorted positions kept
            by_rank = np.empty(len(self._terms), np.int64)
            by_rank[self._rank_host] = np.arange(len(self._terms))
            self._names = [self._terms[i] for i in by_rank[kept]]
        return self._names

    @property
    def vocabulary_(self):
        """term -> column."""
        if self._vocabulary is None:
            self._vocabulary = {t: i for i, t in enumerate(self.feature_names_)}
        return self._vocabulary

    # -- texts ------------------------------------------------------------------------------
    def fit_transform(self, texts) -> DeviceCSR:
        doc_ptr, tokens, terms = tokenize_corpus(texts, self.token_pattern, self.stop_words)
        return self.fit_transform_tokens(doc_ptr, tokens, terms)

    def fit(self, texts) -> "TfidfFeatures":
        self.fit_transform(texts)
        return self

    def transform(self, texts) -> DeviceCSR:
        self._require_fit()
        doc_ptr, tokens, _ = tokenize_corpus(texts, self.token_pattern, self.stop_words,
                                             vocabulary=self.vocabulary_)
        return self.transform_tokens(doc_ptr, tokens)

    # -- token ids --------------------------------------------------------------------------
    def fit_transform_tokens(self, doc_ptr, tokens, terms, rank=None) -> DeviceCSR:
        """Fit on provisional ids (tokens[i] indexes `terms`, any order) and transform them.
        `rank` = term_ranks(terms), for a caller that has it already."""
        terms = terms if isinstance(terms, list) else list(terms)
        V = len(terms)
        if V == 0:
            raise ValueError("empty vocabulary; perhaps the documents only contain stop words")
        doc_ptr = _host_doc_ptr(doc_ptr)
        n_docs = len(doc_ptr) - 1
        lo, hi = df_bounds(self.min_df, self.max_df, n_docs)
        dev = self.device
        rank_host = term_ranks(terms) if rank is None else np.ascontiguousarray(rank, np.int32)
        if rank_host.shape != (V,):
            raise ValueError(f"rank has shape {rank_host.shape}, not one entry per term ({V})")
        rank = torch.from_numpy(rank_host).to(dev)
        df = torch.zeros(V, dtype=torch.int64, device=dev)
        indptr, indices, counts = self._count(doc_ptr, tokens, V, rank, df)
        stream = self._stream()
        new_id = torch.empty(V, dtype=torch.int32, device=dev)
        kept_df = torch.empty(V, dtype=torch.int64, device=dev)
        n_kept_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            ws, nbytes = _native.workspace("gcg_tfidf_select_workspace_bytes", dev, V)
            call("gcg_tfidf_select", V, _ptr(df), lo, hi, _ptr(new_id), _ptr(kept_df),
                 _ptr(n_kept_dev), _ptr(ws), nbytes, stream)
            n_kept = int(n_kept_dev.item())
            if n_kept == 0:
                raise ValueError("After pruning, no terms remain. Try a lower min_df or a higher "
                                 "max_df.")
            nnz = int(indices.numel())
            out_indptr = torch.empty(n_docs + 1, dtype=torch.int32, device=dev)
            ws, nbytes = _native.workspace("gcg_tfidf_compact_workspace_bytes", dev, n_docs)
            args = (n_docs, V, nnz, _ptr(indptr), _ptr(indices), _ptr(counts), _ptr(new_id),
                    _ptr(out_indptr))
            call("gcg_tfidf_compact", *args, None, None, 0, _ptr(ws), nbytes, stream)
            kept_nnz = int(out_indptr[-1].item())
            out_indices = torch.empty(max(kept_nnz, 1), dtype=torch.int32, device=dev)
            out_counts = torch.empty(max(kept_nnz, 1), dtype=torch.int32, device=dev)
            call("gcg_tfidf_compact", *args, _ptr(out_indices), _ptr(out_counts), kept_nnz, None, 0,
                 stream)
            self.df_ = kept_df[:n_kept].clone()
            self.idf_ = torch.empty(n_kept, dtype=torch.float64, device=dev)
            call("gcg_tfidf_idf_f64", n_kept, _ptr(self.df_), n_docs, _ptr(self.idf_), stream)
        # the kept names are host work over strings nobody may ask for: built on first use
        self._terms, self._rank_host, self._new_id = terms, rank_host, new_id
        self._names = self._vocabulary = None
        self.n_features_ = n_kept
        self.n_docs_ = n_docs
        return self._weight(out_indptr, out_indices[:kept_nnz], out_counts[:kept_nnz], n_docs)

    def transform_tokens(self, doc_ptr, tokens) -> DeviceCSR:
        """Transform final ids (columns of the fitted vocabulary; anything else is dropped)."""
        self._require_fit()
        doc_ptr = _host_doc_ptr(doc_ptr)
        indptr, indices, counts = self._count(doc_ptr, tokens, self.n_features_, None, None)
        return self._weight(indptr, indices, counts, len(doc_ptr) - 1)

    # -- device steps -----------------------------------------------------------------------
    def _require_fit(self):
        if self.n_features_ is None:
            raise ValueError("this TfidfFeatures is not fitted yet: call fit_transform first")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _count(self, doc_ptr: np.ndarray, tokens, V: int, rank, df):
        """The count CSR of all documents (indptr, indices, counts), chunk by chunk, with one
        readback (the entry count and the status) however many chunks there are."""
        dev = self.device
        if isinstance(tokens, torch.Tensor):
            tok = tokens.to(device=dev, dtype=torch.int32).contiguous()
        else:
            tok = torch.from_numpy(np.ascontiguousarray(tokens, np.int32)).to(dev)
        n_docs, total = len(doc_ptr) - 1, int(doc_ptr[-1])
        if tok.ndim != 1 or tok.numel() != total:
            raise ValueError(f"doc_ptr ends at {total} but there are {tok.numel()} tokens")
        if total >= 2**31 - 1 or n_docs >= 2**31 - 1:
            raise ValueError("too many tokens or documents for int32 CSR")
        chunks = plan_chunks(doc_ptr, COUNT_CHUNK_ENTRIES)
        ptr_dev = torch.from_numpy(doc_ptr).to(dev)
        indptr = torch.zeros(n_docs + 1, dtype=torch.int32, device=dev)
        indices = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        state = torch.zeros(2, dtype=torch.int64, device=dev)  # entries so far; status (int32)
        stream = self._stream()
        with torch.cuda.device(dev):
            sizes = [(e - d, int(doc_ptr[e] - doc_ptr[d])) for d, e in chunks]
            nbytes = max((_native.workspace_bytes("gcg_tfidf_count_workspace_bytes", nd, nt, V)
                          for nd, nt in sizes), default=0)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            for (d, e), (nd, nt) in zip(chunks, sizes):
                call("gcg_tfidf_count", nd, V, nt, _ptr(ptr_dev, 8 * d),
                     _ptr(tok, 4 * int(doc_ptr[d])), _ptr(rank), _ptr(indptr, 4 * d), _ptr(indices),
                     _ptr(counts), total, _ptr(state), _ptr(df), DF_MODES[DF_MODE],
                     _ptr(state, 8), _ptr(ws), nbytes, stream)
            nnz, status = state.tolist()
        if status & 0xffffffff:
            raise RuntimeError("gcg_tfidf_count: the count CSR outgrew its token-count capacity")
        return indptr, indices[:nnz].clone(), counts[:nnz].clone()

    def _weight(self, indptr, indices, counts, n_rows: int) -> DeviceCSR:
        dev = self.device
        n_cols, nnz = self.n_features_, int(indices.numel())
        vals = torch.empty(nnz, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("gcg_tfidf_weight_f32", n_rows, n_cols, nnz, _ptr(indptr), _ptr(indices),
                 _ptr(counts), _ptr(self.idf_) if self.use_idf else None, int(self.binary),
                 int(self.sublinear_tf), _NORMS[self.norm], _ptr(vals), self._stream())
        return DeviceCSR(indptr, indices, vals, (n_rows, n_cols), validate=False)


def dataloader_features(df_train, df_dev, df_test, **kw):
    """(X, vectorizer): DataLoader.tfidf (fit on train, transform dev and test) and the vstack
    of tensormain.py:215, all on the device. The frames carry a `text` column, as
    DataLoader.load_data leaves them; `kw` are TfidfFeatures' arguments."""
    vec = TfidfFeatures(**kw)
    parts = [vec.fit_transform(df_train["text"].values), vec.transform(df_dev["text"].values),
             vec.transform(df_test["text"].values)]
    return vstack(parts), vec
