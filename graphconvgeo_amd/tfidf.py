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

`tokenize_corpus_device` is `tokenize_corpus` with the per-token work on the device
(csrc/tokenize.hip). The host keeps what Python does in C loops over the whole corpus (lower,
join, encode) and what is per unique term (slicing the terms' strings out of the bytes, the stop
list or the fitted vocabulary); the device finds the tokens in the UTF-8 bytes, builds the term
dictionary in order of first appearance and applies the host's per-term action.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
import re
import time

import numpy as np
import torch

from . import _native
from ._native import call
from .sparse import DeviceCSR, vstack

TOKEN_PATTERN = r"(?u)(?<![#@])\b\w\w+\b"  # data.py:256
SKLEARN_TOKEN_PATTERN = r"(?u)\b\w\w+\b"  # CountVectorizer's default

# The patterns tokenize_corpus_device restates as a run rule -> whether a run preceded by '#' or
# '@' is dropped.
DEVICE_PATTERNS = {TOKEN_PATTERN: 1, SKLEARN_TOKEN_PATTERN: 0}
# Bytes of text one workgroup marks (GCG_TOKENIZE_TILE_BYTES, csrc/tokenize.hip).
TOKENIZE_TILE_BYTES = 4096
TOKENIZERS = ("host", "device")
_DROP = -2  # GCG_TOKENIZE_DROP
_N_CODE_POINTS = 0x110000

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


_word_table = None


def word_char_table() -> np.ndarray:
    """The regex engine's \\w for `str` patterns as a bitmap over U+0000..U+10FFFF: bit cp & 31
    of uint32 word cp >> 5. Asked of `re` itself, once (every code point as a one-character
    string, split on non-word characters), not restated."""
    global _word_table
    if _word_table is None:
        word = np.zeros(_N_CODE_POINTS, np.uint8)
        find = re.compile(r"(?u)\w").finditer
        step = 1 << 16
        for lo in range(0, _N_CODE_POINTS, step):
            # surrogates cannot be encoded and never reach the device: left 0
            text = "".join(map(chr, range(lo, lo + step)))
            word[[lo + m.start() for m in find(text)]] = 1
        table = np.packbits(word, bitorder="little").view("<u4").astype(np.uint32)
        table.setflags(write=False)
        _word_table = table
    return _word_table


_table_dev = {}


def _word_table_on(dev):
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _table_dev:
        _table_dev[key] = torch.from_numpy(word_char_table().copy()).to(dev)
    return _table_dev[key]


def _device_pattern(token_pattern) -> int:
    if token_pattern not in DEVICE_PATTERNS:
        raise ValueError(f"token_pattern {token_pattern!r} is not one the device tokeniser "
                         f"restates ({', '.join(map(repr, DEVICE_PATTERNS))}): use tokenize_corpus")
    return DEVICE_PATTERNS[token_pattern]


def _corpus_bytes(texts, lowercase):
    """(buf, doc_off): the documents, lowercased when asked, joined by one NUL each and encoded
    to UTF-8. doc_off is None when no document contains a NUL (the separators are then the only
    NULs and the device finds the documents by them), else the documents' byte offsets."""
    docs = []
    for d, text in enumerate(texts):
        if isinstance(text, bytes):
            text = text.decode("utf-8")
        if not isinstance(text, str):
            raise ValueError(f"document {d} is not a string: {type(text).__name__}")
        docs.append(text)
    joined = "\x00".join(docs)
    plain = joined.count("\x00") == len(docs) - 1
    # NUL is neither cased nor case-ignorable, so lowering the joined text lowers each document
    # as on its own, the final-sigma rule included; a document with a NUL of its own is lowered
    # by itself all the same, since its offsets are taken per document anyway
    if lowercase and plain:
        joined = joined.lower()
    try:
        if plain:
            return joined.encode("utf-8"), None
        parts = [(t.lower() if lowercase else t).encode("utf-8") for t in docs]
    except UnicodeEncodeError:
        for d, t in enumerate(docs):
            try:
                t.encode("utf-8")
            except UnicodeEncodeError as e:
                raise ValueError(f"document {d} cannot be encoded as UTF-8: {e}") from e
        raise
    doc_off = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([len(p) + 1 for p in parts], out=doc_off[1:])
    return b"\x00".join(parts), doc_off


def tokenize_corpus_device(texts, token_pattern=TOKEN_PATTERN, stop_words="english",
                           lowercase=True, vocabulary=None, device="cuda", hash_bits=64,
                           timings=None):
    """tokenize_corpus with the per-token work on the device: (doc_ptr, tokens, terms) under
    the same contract, `tokens` an int32 device tensor, `doc_ptr` the host int64 array.

    Only the patterns of DEVICE_PATTERNS. The device's term dictionary goes by a 64-bit hash of
    the token's bytes and is verified byte by byte; where two terms share a hash the corpus is
    tokenised by tokenize_corpus instead and `tokenize_corpus_device.fallbacks` counts it, so the
    result is exact either way (`hash_bits` below 64 cuts the hash: for tests). `timings`, a dict,
    receives the seconds of the stages (prep_s, upload_s, kernels_s, terms_s), each closed by a
    synchronisation it would not otherwise need."""
    lookbehind = _device_pattern(token_pattern)
    stops = _stop_set(stop_words)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the device tokeniser runs on the GPU: device must be a CUDA (HIP) device")
    if not 1 <= int(hash_bits) <= 64:
        raise ValueError("hash_bits must be in 1 .. 64")
    fixed = vocabulary is not None

    def lap(name, t0):
        if timings is None:
            return t0
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        if t0 is not None:
            timings[name] = timings.get(name, 0.0) + t1 - t0
        return t1

    t = lap(None, None)
    texts = list(texts)
    n_docs = len(texts)
    buf, doc_off = _corpus_bytes(texts, lowercase)
    n = len(buf)
    empty = (np.zeros(n_docs + 1, np.int64), torch.empty(0, dtype=torch.int32, device=dev),
             None if fixed else [])
    if n_docs == 0 or n == 0:
        return empty
    if n > 1 << 33:
        raise ValueError("the corpus has more than 2^33 bytes: tokenise it in parts")
    t = lap("prep_s", t)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    n16 = (n + 15) // 16 * 16
    tiles = -(-n // TOKENIZE_TILE_BYTES)
    with torch.cuda.device(dev):
        table = _word_table_on(dev)
        text = torch.empty(n16, dtype=torch.uint8, device=dev)
        # (a bytearray, because torch takes no read-only buffer)
        text[:n].copy_(torch.frombuffer(bytearray(buf), dtype=torch.uint8))
        off_dev = None if doc_off is None else torch.from_numpy(doc_off).to(dev)
        t = lap("upload_s", t)
        flags = torch.empty(n16, dtype=torch.uint8, device=dev)
        tile_base = torch.empty(tiles + 1, dtype=torch.int64, device=dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        ws, nbytes = _native.workspace("gcg_tokenize_mark_workspace_bytes", dev, n)
        call("gcg_tokenize_mark", n, _ptr(text), _ptr(table), lookbehind, _ptr(flags),
             _ptr(tile_base), _ptr(totals), _ptr(ws), nbytes, stream)
        n_tokens, n_nul = totals.tolist()
        if doc_off is None and n_nul != n_docs - 1:
            raise RuntimeError(f"gcg_tokenize_mark: {n_nul} separators for {n_docs} documents")
        if n_tokens >= 2**31 - 1:
            raise ValueError("too many tokens for int32 CSR")
        if n_tokens == 0:
            return empty
        raw_ptr = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        tok_term = torch.empty(n_tokens, dtype=torch.int32, device=dev)
        term_start = torch.empty(n_tokens, dtype=torch.int64, device=dev)
        term_len = torch.empty(n_tokens, dtype=torch.int32, device=dev)
        result = torch.zeros(2, dtype=torch.int64, device=dev)
        ws, nbytes = _native.workspace("gcg_tokenize_terms_workspace_bytes", dev, n_tokens,
                                       int(hash_bits))
        call("gcg_tokenize_terms", n, _ptr(text), _ptr(flags), _ptr(tile_base), n_tokens, n_docs,
             _ptr(off_dev), int(hash_bits), _ptr(raw_ptr), _ptr(tok_term), _ptr(term_start),
             _ptr(term_len), _ptr(result), _ptr(ws), nbytes, stream)
        n_terms, collision = result.tolist()
        del ws, flags, tile_base
        if collision:
            # two terms under one hash: exact by the host's tokeniser for this corpus
            tokenize_corpus_device.fallbacks += 1
            doc_ptr, tokens, terms = tokenize_corpus(texts, token_pattern, stop_words, lowercase,
                                                     vocabulary)
            return doc_ptr, torch.from_numpy(tokens).to(dev), terms
        starts = term_start[:n_terms].cpu().numpy()
        lens = term_len[:n_terms].cpu().numpy()
        t = lap("kernels_s", t)
        # per unique term, never per token: its string, then the stop list or the vocabulary
        names = [buf[s:e].decode("utf-8") for s, e in zip(starts.tolist(), (starts + lens).tolist())]
        if fixed:
            get = vocabulary.get
            keep = np.fromiter((w not in stops for w in names), bool, n_terms)
            cols = np.fromiter((get(w, -1) for w in names), np.int64, n_terms)
            if np.any(keep & ((cols < -1) | (cols >= 2**31))):
                raise ValueError("vocabulary columns must be in [0, 2^31)")
            action = np.where(keep, cols, _DROP)
            terms = None
        else:
            keep = np.fromiter((w not in stops for w in names), bool, n_terms)
            action = np.where(keep, np.cumsum(keep) - 1, _DROP)
            terms = [w for w, k in zip(names, keep.tolist()) if k]
        action_dev = torch.from_numpy(action.astype(np.int32)).to(dev)
        t = lap("terms_s", t)
        tokens = torch.empty(n_tokens, dtype=torch.int32, device=dev)
        ptr_dev = torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
        ws, nbytes = _native.workspace("gcg_tokenize_remap_workspace_bytes", dev, n_tokens)
        call("gcg_tokenize_remap", n_tokens, _ptr(tok_term), n_terms, _ptr(action_dev), n_docs,
             _ptr(raw_ptr), _ptr(tokens), _ptr(ptr_dev), _ptr(ws), nbytes, stream)
        doc_ptr = ptr_dev.cpu().numpy()
        lap("kernels_s", t)
    return doc_ptr, tokens[:int(doc_ptr[-1])], terms


tokenize_corpus_device.fallbacks = 0


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

    fit_transform / transform take texts and return a DeviceCSR (tokenizer="host" tokenises
    with tokenize_corpus, "device" with tokenize_corpus_device); fit_transform_tokens /
    transform_tokens take what tokenize_corpus returns (the token array may already be a device
    tensor). After a fit: vocabulary_ (term -> column) and feature_names_ (sorted), both built
    on first use, n_features_, df_ (int64 device tensor, the kept terms' document frequencies),
    idf_ (float64 device tensor), n_docs_."""

    def __init__(self, min_df=10, max_df=0.2, norm="l2", use_idf=True, binary=True,
                 sublinear_tf=False, token_pattern=TOKEN_PATTERN, stop_words="english",
                 device="cuda", tokenizer="host"):
        if norm not in _NORMS:
            raise ValueError(f"norm must be 'l2', 'l1' or None, not {norm!r}")
        if tokenizer not in TOKENIZERS:
            raise ValueError(f"tokenizer must be 'host' or 'device', not {tokenizer!r}")
        if tokenizer == "device":
            _device_pattern(token_pattern)
        self.tokenizer = tokenizer
        self.tokenize_s_ = 0.0
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
    def _tokenize(self, texts, vocabulary=None):
        """The chosen tokeniser; tokenize_s_ adds up the seconds spent in it (the device
        tokeniser ends on a readback, so they are whole)."""
        t0 = time.perf_counter()
        if self.tokenizer == "device":
            out = tokenize_corpus_device(texts, self.token_pattern, self.stop_words,
                                         vocabulary=vocabulary, device=self.device)
        else:
            out = tokenize_corpus(texts, self.token_pattern, self.stop_words, vocabulary=vocabulary)
        self.tokenize_s_ += time.perf_counter() - t0
        return out

    def fit_transform(self, texts) -> DeviceCSR:
        doc_ptr, tokens, terms = self._tokenize(texts)
        return self.fit_transform_tokens(doc_ptr, tokens, terms)

    def fit(self, texts) -> "TfidfFeatures":
        self.fit_transform(texts)
        return self

    def transform(self, texts) -> DeviceCSR:
        self._require_fit()
        doc_ptr, tokens, _ = self._tokenize(texts, self.vocabulary_)
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
