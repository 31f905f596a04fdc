"""The dialect-embedding evaluation on the GPU (csrc/neighbours.hip).

  scale_embeddings  eval_embeddings' preprocessing (main.py:373-377): MinMaxScaler(0, 1) on
                    every dimension, then l1-normalised rows
  neighbour_ranks   the 0-based position of every gold word in its query's ordering of all V
                    words: what recall@k needs of nearest_neighbours(k=len(vocab))
                    (main.py:108-162, 378), in one pass over the embeddings
  kneighbors        the k <= 1024 nearest words of every query, in order (sklearn's
                    NearestNeighbors(...).kneighbors on Euclidean distances)
  DialectLexicon    the DARE json-lines file (main.py:119-132) as dialect -> gold words, and
                    its (query, gold word) pairs over a vocabulary
  recall_at_k       main.py:230-281: the micro recall and the per-dialect recalls, from ranks
  eval_embeddings   main.py:364-384 in one call; dialect_eval's percent list (main.py:358-359)
                    is the same call with other `ks` and scale=False

Embeddings and queries are numpy arrays or tensors and are float32 on the device; results
stay on the device unless noted. A squared distance is the float32 sum of (q_j - e_j)^2 over
j = 0 .. D - 1 in that order (one subtraction and one fused multiply-add per term), words are
ordered by (that sum, row index) ascending, and both functions share the bits of every
distance, so kneighbors(...)[1][q, r] == w exactly when the rank of w for query q is r. The
query's own row is not removed: it has rank 0, as in the reference.

One deliberate deviation from the reference. nearest_neighbours files a dialect with
subregions under the lowercased subregion string, but recall_at_k (main.py:244-247) looks it up
without lowercasing and so reports every such dialect with an upper-case letter as "this
dialect does not exist", silently dropping it from the recall. Here the same lowercased key is
used on both sides.

Not built: nearest_neighbours2 (queries as products of term embeddings), loading word2vec or
logistic-regression embeddings, get_vocab / get_frequent_words, k > 1024 in kneighbors.
"""
from __future__ import annotations

import json
from collections import namedtuple

import numpy as np
import torch

from ._native import call, load, workspace as _workspace
from .geo import _ptr, _stream

Pairs = namedtuple("Pairs", "dialects rows pair_ptr pair_word n_missing")
Recall = namedtuple("Recall", "ks micro per_dialect totals")
DialectEval = namedtuple("DialectEval", "ks micro dialects totals per_dialect ranks")

MAX_K = 1024
_RANK_ERRORS = {1: "a non-finite embedding, query or distance",
                2: "pair_word holds an index outside [0, V)",
                3: "pair_ptr must rise from 0 to the number of pairs"}


def tile(name: str) -> int:
    """A tile size of the kernels: "row", "query", "query_small", "slot_cap", "col_chunk",
    "max_k", "minmax_rows" or "merge_slice" (gcg_neighbours_tile)."""
    names = ("row", "query", "query_small", "slot_cap", "col_chunk", "max_k", "minmax_rows",
             "merge_slice")
    if name not in names:
        raise ValueError(f"tile must be one of {names}, got {name!r}")
    return int(load().gcg_neighbours_tile(names.index(name)))


# ---------------------------------------------------------------- argument checks (no launch)

def _is_device(x) -> bool:
    return torch.is_tensor(x) and x.is_cuda


def _device(device, *operands) -> torch.device:
    if device is None:
        device = next((x.device for x in operands if _is_device(x)), "cuda")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the dialect kernels run on the GPU: device must be a CUDA (HIP) device")
    return dev


def _check_matrix(x, name):
    """`x` as a 2-D array or tensor after the checks that need no device: the shape, the dtype
    and, for host data, the finiteness (device data is checked by the kernels)."""
    a = x if torch.is_tensor(x) else np.asarray(x)
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError(f"{name} must have shape (rows, D) with D >= 1, got {tuple(a.shape)}")
    if torch.is_tensor(a):
        if not a.dtype.is_floating_point:
            raise ValueError(f"{name} must be floating point, got {a.dtype}")
        finite = True if a.is_cuda else bool(torch.isfinite(a).all())
    else:
        if a.dtype.kind not in "fiu":
            raise ValueError(f"{name} must be numeric, got {a.dtype}")
        finite = bool(np.isfinite(a).all())
    if not finite:
        raise ValueError(f"{name} holds a non-finite value")
    return a


def _to_device(a, dev) -> torch.Tensor:
    """float32 device tensor with unit column stride (a row stride is kept)."""
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    a = a.to(dev).to(torch.float32)
    if (a.shape[1] > 1 and a.stride(1) != 1) or (a.shape[0] > 1 and a.stride(0) < a.shape[1]):
        a = a.contiguous()
    return a


def _ld(a) -> int:
    return int(a.stride(0)) if a.shape[0] > 1 else int(a.shape[1])


def _upload(a: np.ndarray, dev) -> torch.Tensor:
    """A small host array to the device without a host wait."""
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)


def _check_indices(x, n, name) -> np.ndarray | torch.Tensor:
    """A 1-D integer index array into [0, n): host data as int64 NumPy, device data as is (its
    range costs one readback)."""
    if _is_device(x):
        if x.dim() != 1 or x.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name} must be a 1-D int32 or int64 array, got {x.dtype} {tuple(x.shape)}")
        if x.numel() > 0:
            lo, hi = torch.stack([x.min(), x.max()]).tolist()
            if lo < 0 or hi >= n:
                raise ValueError(f"{name} holds an index outside [0, {n})")
        return x
    a = x.numpy() if torch.is_tensor(x) else np.asarray(x)
    if a.ndim != 1 or a.dtype.kind not in "iu":
        raise ValueError(f"{name} must be a 1-D integer array, got {a.dtype} {a.shape}")
    a = a.astype(np.int64)
    if a.size > 0 and (a.min() < 0 or a.max() >= n):
        raise ValueError(f"{name} holds an index outside [0, {n})")
    return a


def _is_index_form(queries) -> bool:
    a = queries if torch.is_tensor(queries) else np.asarray(queries)
    return a.ndim == 1


def _operands(embs, queries, device):
    """(E, queries) as float32 device matrices; `queries` may be rows of `embs`."""
    e = _check_matrix(embs, "embs")
    if _is_index_form(queries):
        idx = _check_indices(queries, int(e.shape[0]), "queries")
        dev = _device(device, embs)
        e = _to_device(e, dev)
        idx = idx.to(dev).long() if torch.is_tensor(idx) else _upload(idx, dev)
        return e, e[idx].contiguous()
    q = _check_matrix(queries, "queries")
    if q.shape[1] != e.shape[1]:
        raise ValueError(f"queries have {q.shape[1]} columns, embs {e.shape[1]}")
    dev = _device(device, embs, queries)
    return _to_device(e, dev), _to_device(q, dev)


def _check_pairs(pair_ptr, pair_word, n_queries, n_words):
    """(pair_ptr, pair_word) as int32 arrays. Host data is checked here; device data by the
    kernels' status word."""
    out = []
    for x, name in ((pair_ptr, "pair_ptr"), (pair_word, "pair_word")):
        if _is_device(x):
            if x.dim() != 1 or x.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"{name} must be a 1-D int32 or int64 array")
            out.append(x)
            continue
        a = x.numpy() if torch.is_tensor(x) else np.asarray(x)
        if a.ndim != 1 or (a.size > 0 and a.dtype.kind not in "iu"):
            raise ValueError(f"{name} must be a 1-D integer array, got {a.dtype} {a.shape}")
        out.append(a.astype(np.int64))
    ptr, word = out
    if ptr.shape[0] != n_queries + 1:
        raise ValueError(f"pair_ptr must have {n_queries + 1} entries, got {ptr.shape[0]}")
    if word.shape[0] > 2 ** 31 - 2:
        raise ValueError("too many pairs")
    if not torch.is_tensor(ptr):
        if ptr[0] != 0 or ptr[-1] != word.shape[0] or np.any(np.diff(ptr) < 0):
            raise ValueError(_RANK_ERRORS[3])
    if not torch.is_tensor(word) and word.size > 0 and (word.min() < 0 or word.max() >= n_words):
        raise ValueError(f"pair_word holds an index outside [0, {n_words})")
    return ptr, word


def _int32_device(a, dev) -> torch.Tensor:
    if torch.is_tensor(a):
        return a.to(dev).to(torch.int32).contiguous()
    return _upload(a.astype(np.int32), dev)


# ---------------------------------------------------------------- the ABI calls (no readback)

def _scale(e):
    """(scaled [V, D] float32, status[1])."""
    dev, (v, d) = e.device, e.shape
    out = torch.empty((v, d), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = _workspace("gcg_minmax_l1_rows_f32_workspace_bytes", dev, v, d)
        call("gcg_minmax_l1_rows_f32", v, d, _ptr(e), _ld(e), _ptr(out), d, _ptr(status), _ptr(ws),
             nbytes, _stream(dev))
    return out, status


def _ranks(e, q, ptr, word):
    """(rank[P] int32, status[1])."""
    dev, p = e.device, word.shape[0]
    rank = torch.zeros(p, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = _workspace("gcg_neighbour_ranks_f32_workspace_bytes", dev, q.shape[0], p)
        call("gcg_neighbour_ranks_f32", e.shape[0], e.shape[1], _ptr(e), _ld(e), q.shape[0], _ptr(q),
             _ld(q), p, _ptr(ptr), _ptr(word), _ptr(rank), _ptr(status), _ptr(ws), nbytes,
             _stream(dev))
    return rank, status


# ---------------------------------------------------------------- the public functions

def scale_embeddings(embs, device=None) -> torch.Tensor:
    """MinMaxScaler(feature_range=(0, 1)) on every column, then normalize(norm='l1') on every
    row (main.py:373-377), as a new float32 device tensor. scale = 1 / (max - min), or 1 where
    max == min; x * scale + (0 - min * scale); a row whose l1 norm is 0 is left as it is. The
    affine step and the row sums run in float64 on float32 input, so every element is within a
    rounding or two of sklearn's float64 result. ValueError for a non-finite value (device data:
    one readback of the status word)."""
    e = _check_matrix(embs, "embs")
    e = _to_device(e, _device(device, embs))
    out, status = _scale(e)
    if int(status.item()) != 0:
        raise ValueError("embs holds a non-finite value")
    return out


def neighbour_ranks(embs, queries, pair_ptr, pair_word, device=None) -> torch.Tensor:
    """int32 [P] device tensor: rank[p] = the number of words v with (d2(q, v), v) <
    (d2(q, w), w) for the pair p = (query q, word w = pair_word[p]); query q owns pairs
    [pair_ptr[q], pair_ptr[q + 1]). queries: a [Q, D] matrix or a 1-D integer array of rows of
    embs. One readback, of the status word."""
    e = _check_matrix(embs, "embs")
    nq = int((queries if torch.is_tensor(queries) else np.asarray(queries)).shape[0])
    ptr, word = _check_pairs(pair_ptr, pair_word, nq, int(e.shape[0]))
    e, q = _operands(embs, queries, device)
    rank, status = _ranks(e, q, _int32_device(ptr, e.device), _int32_device(word, e.device))
    st = int(status.item())
    if st != 0:
        raise ValueError(_RANK_ERRORS[st])
    return rank


def kneighbors(embs, queries, k, device=None):
    """(distances [Q, k] float32, indices [Q, k] int32) device tensors: every query's k nearest
    rows of embs by (squared distance, row index), nearest first; distances are the square
    roots, as sklearn's kneighbors returns. 1 <= k <= min(V, 1024). One readback, of the
    status word."""
    e = _check_matrix(embs, "embs")
    if isinstance(k, bool) or int(k) != k:
        raise ValueError(f"k must be an integer, got {k!r}")
    k = int(k)
    if not 1 <= k <= min(int(e.shape[0]), MAX_K):
        raise ValueError(f"need 1 <= k <= min(V, {MAX_K}) = {min(int(e.shape[0]), MAX_K)}, got {k}")
    e, q = _operands(embs, queries, device)
    dev, nq = e.device, q.shape[0]
    d2 = torch.empty((nq, k), dtype=torch.float32, device=dev)
    index = torch.empty((nq, k), dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = _workspace("gcg_kneighbors_f32_workspace_bytes", dev, e.shape[0], nq, k)
        call("gcg_kneighbors_f32", e.shape[0], e.shape[1], _ptr(e), _ld(e), nq, _ptr(q), _ld(q), k,
             _ptr(d2), _ptr(index), _ptr(status), _ptr(ws), nbytes, _stream(dev))
    if int(status.item()) != 0:
        raise ValueError(_RANK_ERRORS[1])
    return torch.sqrt(d2), index


class DialectLexicon:
    """dialect key -> the set of its gold words (the reference's final_dialect_words)."""

    def __init__(self, words):
        self.words = {str(key): set(ws) for key, ws in dict(words).items()}

    @classmethod
    def from_dare_json(cls, path):
        """The json-lines file of main.py:119-132: one object per line with the fields
        `dialect`, `dialect subregions` and `word`. The key is the lowercased subregion string
        where there is one, else the lowercased dialect; words are lowercased."""
        words = {}
        with open(path, encoding="utf-8") as fin:
            for line in fin:
                line = line.strip()
                if not line:
                    continue
                obj = json.loads(line)
                key = (obj["dialect subregions"] or obj["dialect"]).lower()
                words.setdefault(key, set()).add(obj["word"].lower())
        return cls(words)

    def pairs(self, vocab) -> Pairs:
        """Pairs(dialects, rows, pair_ptr, pair_word, n_missing) over `vocab` (a sequence of
        words; a word's row is its first position): the dialects whose key is itself in vocab,
        sorted (main.py:139); their rows; per dialect the rows of its gold words that are in
        vocab, ascending, in CSR form; and the number of its gold words that are not. Those
        count in recall's denominator and can never be found (main.py:259-267)."""
        index = {}
        for i, w in enumerate(vocab):
            index.setdefault(w, i)
        dialects = [d for d in sorted(self.words) if d in index]
        ptr, word, missing = [0], [], []
        for d in dialects:
            found = sorted(index[w] for w in self.words[d] if w in index)
            word.extend(found)
            ptr.append(len(word))
            missing.append(len(self.words[d]) - len(found))
        return Pairs(dialects, np.array([index[d] for d in dialects], dtype=np.int32),
                     np.array(ptr, dtype=np.int32), np.array(word, dtype=np.int32),
                     np.array(missing, dtype=np.int64))


def _check_ks(ks) -> np.ndarray:
    k = np.asarray(list(ks))
    if k.ndim != 1 or k.size == 0 or k.dtype.kind not in "iu" or k.min() < 0:
        raise ValueError(f"ks must be a non-empty list of integers >= 0, got {ks!r}")
    return k.astype(np.int64)


def _totals(pair_ptr: np.ndarray, n_missing) -> np.ndarray:
    missing = np.asarray(n_missing)
    if missing.shape != (pair_ptr.shape[0] - 1,) or missing.dtype.kind not in "iu" or \
            (missing.size > 0 and missing.min() < 0):
        raise ValueError(f"n_missing must hold {pair_ptr.shape[0] - 1} integers >= 0")
    totals = np.diff(pair_ptr) + missing.astype(np.int64)
    if totals.sum() == 0:
        raise ValueError("no gold word: the recall has no denominator")
    return totals


def _hits(ranks: torch.Tensor, ptr: torch.Tensor, ks: torch.Tensor) -> torch.Tensor:
    """int64 [K, R]: per k and per dialect, the pairs with rank < k. Device ops, no readback."""
    below = (ranks.long()[None, :] < ks[:, None]).long()
    run = torch.cat([below.new_zeros((ks.shape[0], 1)), torch.cumsum(below, dim=1)], dim=1)
    return run[:, ptr[1:].long()] - run[:, ptr[:-1].long()]


def _recall(ks, hits: np.ndarray, totals: np.ndarray) -> Recall:
    micro = [100.0 * float(h) / float(totals.sum()) for h in hits.sum(axis=1)]
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.where(totals > 0, 100.0 * hits / np.maximum(totals, 1), np.nan)
    return Recall([int(k) for k in ks], micro, per, totals)


def recall_at_k(ranks, pair_ptr, n_missing, ks) -> Recall:
    """main.py:230-281 from ranks: Recall(ks, micro, per_dialect, totals). micro[i] =
    100 * #{rank < ks[i]} / total_positive, where total_positive counts every gold word of every
    covered dialect, in the vocabulary or not; per_dialect[i, r] = the recall of dialect r (the
    `info` list; NaN for a dialect without gold words, which the reference skips); totals[r] =
    its gold words. A gold word is found within k when its rank is below k: the neighbour list
    nbrs[0:k] of the reference holds the ranks 0 .. k - 1, the query's own row among them."""
    k = _check_ks(ks)
    ptr_np = pair_ptr.cpu().numpy() if torch.is_tensor(pair_ptr) else np.asarray(pair_ptr)
    n_pairs = int(ranks.shape[0])
    if ptr_np.ndim != 1 or ptr_np.size < 1 or ptr_np[0] != 0 or ptr_np[-1] != n_pairs or \
            np.any(np.diff(ptr_np) < 0):
        raise ValueError(_RANK_ERRORS[3])
    totals = _totals(ptr_np.astype(np.int64), n_missing)
    r = ranks if torch.is_tensor(ranks) else torch.as_tensor(np.asarray(ranks))
    dev = r.device
    ptr_t = torch.as_tensor(ptr_np.astype(np.int64))
    ks_t = torch.as_tensor(k)
    if r.is_cuda:
        ptr_t, ks_t = _upload(ptr_t.numpy(), dev), _upload(k, dev)
    return _recall(k, _hits(r, ptr_t, ks_t).cpu().numpy(), totals)


def eval_embeddings(vocab, embs, lexicon, ks=(10000, 20000, 30000, 40000, 50000), scale=True,
                    device=None) -> DialectEval:
    """main.py:364-384 in one call: scale the embeddings (unless scale=False), rank every
    dialect's gold words among the neighbours of the dialect's own vocabulary entry, and report
    recall@k. DialectEval(ks, micro, dialects, totals, per_dialect, ranks): micro[i] is the
    reference's "micro recall" at ks[i]; dialects, totals and per_dialect[i] are its `info`
    list; ranks (int32 device tensor, ordered as lexicon.pairs(vocab)) is what they were counted
    from. One readback: the status words and the counts together."""
    e = _check_matrix(embs, "embs")
    vocab = list(vocab)
    if len(vocab) != e.shape[0]:
        raise ValueError(f"vocab has {len(vocab)} words, embs {e.shape[0]} rows")
    k = _check_ks(ks)
    pairs = lexicon.pairs(vocab)
    if not pairs.dialects:
        raise ValueError("no dialect of the lexicon is in the vocabulary")
    totals = _totals(pairs.pair_ptr.astype(np.int64), pairs.n_missing)
    dev = _device(device, embs)
    e = _to_device(e, dev)
    st_scale = torch.zeros(1, dtype=torch.int32, device=dev)
    if scale:
        e, st_scale = _scale(e)
    ptr = _upload(pairs.pair_ptr, dev)
    q = e[_upload(pairs.rows.astype(np.int64), dev)].contiguous()
    ranks, st_rank = _ranks(e, q, ptr, _upload(pairs.pair_word, dev))
    hits = _hits(ranks, ptr, _upload(k, dev))
    back = torch.cat([st_scale.long(), st_rank.long(), hits.reshape(-1)]).cpu().numpy()
    if back[0] != 0 or back[1] == 1:
        raise ValueError("embs holds a non-finite value")
    if back[1] != 0:
        raise ValueError(_RANK_ERRORS[int(back[1])])
    rec = _recall(k, back[2:].reshape(k.shape[0], len(pairs.dialects)), totals)
    return DialectEval(rec.ks, rec.micro, pairs.dialects, totals, rec.per_dialect, ranks)
