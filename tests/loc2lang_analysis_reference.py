"""NumPy restatement of the location-to-language model's analyses (reference loc2lang.py:516-614
state_dialect_words, 693-712 the top words, 755-766 get_local_words) -- TEST HELPER, the
project's own code.

Everything starts from float32 logits. The float64 functions widen them first and are the judge;
the float32 functions do the same arithmetic in NumPy float32 (softmax, then the sums) and are the
yardstick of what the number format allows. 0 log 0 = 0 throughout (scipy.stats.entropy's
convention); a logit of -inf is a probability of exactly 0.
"""
import numpy as np


def _wide(Z, dtype):
    return np.asarray(Z, dtype=np.float32).astype(dtype)


def row_lse(Z, dtype=np.float64):
    """max + log sum exp(z - max) per row, in `dtype`."""
    Z = _wide(Z, dtype)
    with np.errstate(all="ignore"):
        m = Z.max(axis=1)
        return m + np.log(np.exp(Z - m[:, None]).sum(axis=1, dtype=dtype))


def log_softmax(Z, dtype=np.float64):
    return _wide(Z, dtype) - row_lse(Z, dtype)[:, None]


def softmax(Z, dtype=np.float64):
    """exp(z - max) / sum exp(z - max), the reference's softmax, in `dtype`."""
    Z = _wide(Z, dtype)
    with np.errstate(all="ignore"):
        e = np.exp(Z - Z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True, dtype=dtype)


def column_stats(Z):
    """float64 (S, T, entropies): S = sum_n p, T = sum_n p log p with p = exp(z - lse), and the
    entropy of the l1-normalised column log S - T / S (NaN where S == 0)."""
    a = log_softmax(Z)
    with np.errstate(all="ignore"):
        p = np.exp(a)
        S = p.sum(axis=0)
        T = np.where(p > 0, p * a, 0.0).sum(axis=0)
        return S, T, np.where(S == 0, np.nan, np.log(S) - T / S)


def column_stats_f32(Z):
    """The same in float32 from NumPy's float32 softmax: (S, T, entropies) as float64 arrays of
    float32 values."""
    p = softmax(Z, np.float32)
    with np.errstate(all="ignore"):
        S = p.sum(axis=0, dtype=np.float32)
        T = np.where(p > 0, p * np.log(p), np.float32(0)).sum(axis=0, dtype=np.float32)
        ent = np.where(S == 0, np.float32(np.nan), np.log(S) - T / S)
    assert S.dtype == T.dtype == ent.dtype == np.float32
    return S.astype(np.float64), T.astype(np.float64), ent.astype(np.float64)


def entropies_literal(P):
    """loc2lang.py:757-758 with the libraries the reference uses."""
    from scipy import stats
    from sklearn.preprocessing import normalize
    return stats.entropy(normalize(np.asarray(P, dtype=np.float64), norm="l1", axis=0))


def groups_of(group_ptr, group_rows):
    return [np.asarray(group_rows[a:b]) for a, b in zip(group_ptr[:-1], group_ptr[1:])]


def region_scores(Z, group_ptr, group_rows, dtype=np.float64):
    """loc2lang.py:569-579, literally: logprobs = np.log(softmax); per group the mean over its
    rows minus the mean over all rows. [G, V] in `dtype`."""
    with np.errstate(all="ignore"):
        logprobs = np.log(softmax(Z, dtype))
        glob = np.mean(logprobs, axis=0, dtype=dtype)
        return np.stack([np.mean(logprobs[rows, :], axis=0, dtype=dtype) - glob
                         for rows in groups_of(group_ptr, group_rows)])


def region_scores_linear(H, Wo, bo, group_ptr, group_rows):
    """The same through the identity the device path uses, float64: with z = h . Wo + bo,
    ((mean_g h - mean h) . Wo)_v - (mean_g lse - mean lse)."""
    H, Wo, bo = (np.asarray(a, dtype=np.float64) for a in (H, Wo, bo))
    Z = H @ Wo + bo
    m = Z.max(axis=1)
    lse = m + np.log(np.exp(Z - m[:, None]).sum(axis=1))
    out = []
    for rows in groups_of(group_ptr, group_rows):
        out.append((H[rows].mean(axis=0) - H.mean(axis=0)) @ Wo - (lse[rows].mean() - lse.mean()))
    return np.stack(out)


def ranking(score_row):
    """loc2lang.py:580-582: list(reversed(argsort)), the sort stable."""
    return np.argsort(score_row, kind="stable")[::-1]


def region_recall(scores, gold_ptr, gold_word, fractions=(0.01, 0.05, 0.1, 0.15, 0.2)):
    """loc2lang.py:587-614, literally, with sets: (ks, mean recall per k, mean oracle recall per k,
    per-group recalls [len(ks), G] with NaN for the groups skipped, the gold words' ranks)."""
    scores = np.asarray(scores)
    G, V = scores.shape
    ks = [int(f * V) for f in fractions]
    per_group = np.full((len(ks), G), np.nan)
    oracle = np.full((len(ks), G), np.nan)
    ranks = []
    for g in range(G):
        gold = set(int(w) for w in gold_word[gold_ptr[g]:gold_ptr[g + 1]])
        retrieved = [int(v) for v in ranking(scores[g])]
        where = {v: i for i, v in enumerate(retrieved)}
        ranks += [where[int(w)] for w in gold_word[gold_ptr[g]:gold_ptr[g + 1]]]
        if not gold:  # not a covered dialect
            continue
        oracle_retrieved = list(set(retrieved) & gold)
        for i, k in enumerate(ks):
            per_group[i, g] = float(len(set(retrieved[0:k]) & gold)) / len(gold)
            oracle[i, g] = float(len(set(oracle_retrieved[0:k]) & gold)) / len(gold)
    covered = np.diff(np.asarray(gold_ptr)) > 0
    with np.errstate(all="ignore"):  # no covered dialect: the mean of nothing, NaN
        recall = [float(np.mean(per_group[i, covered])) if covered.any() else float("nan")
                  for i in range(len(ks))]
        best = [float(np.mean(oracle[i, covered])) if covered.any() else float("nan")
                for i in range(len(ks))]
    return ks, recall, best, per_group, np.asarray(ranks, dtype=np.int64)


def top_words(Z, k):
    """Per row the k largest logits' columns, descending, ties to the lower index."""
    Z = np.asarray(Z)
    return np.stack([np.argsort(-row.astype(np.float64), kind="stable")[:k] for row in Z])
