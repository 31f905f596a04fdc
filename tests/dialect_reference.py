"""Float64 NumPy restatement of the dialect-embedding evaluation (graphconvgeo_amd.dialect,
csrc/neighbours.hip): eval_embeddings' scaling, the squared distances in difference form with
the full (d2, index) ordering, and recall_at_k with the gold words outside the vocabulary in
its denominator. The tests' reference; checked against sklearn by tests/golden/
make_dialect_golden.py and tests/test_dialect_reference.py."""
import numpy as np


def scale(embs):
    """MinMaxScaler(feature_range=(0, 1)) then normalize(norm='l1'), sklearn's arithmetic:
    scale = 1 / (max - min) (1 for a constant column), x * scale + (0 - min * scale); a row
    whose l1 norm is 0 is left as it is."""
    x = np.asarray(embs, dtype=np.float64)
    lo, hi = x.min(axis=0), x.max(axis=0)
    rng = hi - lo
    s = 1.0 / np.where(rng == 0.0, 1.0, rng)
    y = x * s + (0.0 - lo * s)
    norms = np.abs(y).sum(axis=1)
    return y / np.where(norms == 0.0, 1.0, norms)[:, None]


def dist2(embs, query):
    """sum_j (q_j - e_j)^2 for every row of embs, float64."""
    d = np.asarray(query, dtype=np.float64)[None, :] - np.asarray(embs, dtype=np.float64)
    return (d * d).sum(axis=1)


def ordering(embs, query):
    """(order, d2): the rows of embs by (d2, row index) ascending."""
    d2 = dist2(embs, query)
    return np.lexsort((np.arange(d2.shape[0]), d2)), d2


def ranks_of(embs, query):
    """rank[v] = the position of row v in ordering(embs, query)."""
    order, _ = ordering(embs, query)
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    return rank


def _queries(embs, queries):
    q = np.asarray(queries)
    return np.asarray(embs)[q] if q.ndim == 1 else q


def neighbour_ranks(embs, queries, pair_ptr, pair_word):
    qs = _queries(embs, queries)
    out = np.zeros(len(pair_word), dtype=np.int64)
    for q in range(qs.shape[0]):
        a, b = pair_ptr[q], pair_ptr[q + 1]
        if b > a:
            out[a:b] = ranks_of(embs, qs[q])[np.asarray(pair_word[a:b])]
    return out


def kneighbors(embs, queries, k):
    """(distances, indices) of the k first rows of every query's ordering."""
    qs = _queries(embs, queries)
    dist, idx = [], []
    for q in qs:
        order, d2 = ordering(embs, q)
        idx.append(order[:k])
        dist.append(np.sqrt(d2[order[:k]]))
    return np.array(dist), np.array(idx)


def gamma(d):
    """The relative bound on a float32 d2 of D terms against float64: D non-negative terms, a
    subtraction and a fused multiply-add each."""
    u = (d + 2) * 2.0 ** -24
    return u / (1.0 - u)


def rank_bounds(d2, w, g):
    """(lo, hi) for word w in a query's float64 distances d2: lo counts the rows that are
    below w whatever the float32 rounding, hi those that can be at or below it (w itself is one
    of them), so a correct float32 rank lies in [lo, hi - 1]."""
    lo = int(np.sum(d2 * (1.0 + g) < d2[w] * (1.0 - g)))
    hi = int(np.sum(d2 * (1.0 - g) <= d2[w] * (1.0 + g)))
    return lo, hi


def recall_at_k(ranks, pair_ptr, n_missing, ks):
    """(micro, per_dialect): main.py:230-281 from ranks. A dialect's total is its gold words in
    the vocabulary plus n_missing (never found); a dialect with none is skipped (NaN)."""
    ranks = np.asarray(ranks)
    totals = np.diff(pair_ptr) + np.asarray(n_missing)
    micro, per = [], []
    for k in ks:
        has = np.array([int(np.sum(ranks[pair_ptr[r]:pair_ptr[r + 1]] < k))
                        for r in range(len(totals))])
        micro.append(100.0 * float(has.sum()) / float(totals.sum()))
        per.append([100.0 * float(h) / t if t > 0 else float("nan") for h, t in zip(has, totals)])
    return micro, np.array(per)


def min_relative_gap(embs, queries):
    """The smallest relative gap between neighbouring distances of any query's ordering: above
    it no summation order or expansion can change the order."""
    gap = np.inf
    for q in _queries(embs, queries):
        order, d2 = ordering(embs, q)
        s = d2[order]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.diff(s) / s[1:]
        gap = min(gap, float(np.min(rel[np.isfinite(rel)], initial=np.inf)))
    return gap


def gaussian_embeddings(v, d, seed):
    """Rows of float32 Gaussians with per-column offsets and widths, so the scaling has work."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(v, d)) * rng.uniform(0.5, 3.0, size=d) + rng.uniform(-2.0, 2.0, size=d)
    return x.astype(np.float32)


def integer_embeddings(v, d, seed, span=8):
    """Small integers in [-span, span] as float32: every d2 is exact in float32 for D <= 2048.
    Rows 1 and v // 2 repeat row 0, so there are ties even at large D."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-span, span + 1, size=(v, d)).astype(np.float32)
    if v > 1:
        x[1] = x[0]
        x[v // 2] = x[0]
    return x
