"""GPU side of the dialect-embedding evaluation (graphconvgeo_amd.dialect, csrc/neighbours.hip)
against the float64 restatement (tests/dialect_reference.py): exact (d2, index) orderings on
small-integer data at every tile boundary, derived rank bands on real-valued data, the scaling
against the sklearn fixtures, reproducibility, the readback count and the planted end-to-end
problem."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import dialect_reference as ref
from graphconvgeo_amd import dialect as dl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ROW_T, Q_T, Q_TS, SLOTS, COLS, MAX_K, MM_ROWS, MERGE = 256, 32, 8, 2048, 32, 1024, 1024, 8192

# (V, D, Q): the issue's sizes, then every exported tile size T as T - 1, T, T + 1
EXACT_SHAPES = [(1, 1, 1), (2, 3, 2), (63, 4, 17), (64, 63, 1), (65, 64, 2), (257, 65, 17),
                (2000, 300, 17), (64, 1, 2), (257, 3, 1), (63, 300, 2),
                (ROW_T - 1, COLS, Q_TS - 1), (ROW_T, COLS - 1, Q_TS), (ROW_T + 1, COLS + 1, Q_TS + 1),
                (300, 5, Q_T - 1), (300, 6, Q_T), (300, 7, Q_T + 1),
                (MAX_K - 1, 2, 2), (MAX_K, 3, 1), (MAX_K + 1, 4, 2), (2 * ROW_T, 2048, 1)]


def test_tiles_are_the_ones_the_shapes_sit_on(native_lib):
    got = [dl.tile(n) for n in ("row", "query", "query_small", "slot_cap", "col_chunk", "max_k",
                                "minmax_rows", "merge_slice")]
    assert got == [ROW_T, Q_T, Q_TS, SLOTS, COLS, MAX_K, MM_ROWS, MERGE]


def exact_problem(v, d, q, seed):
    """Integer embeddings with duplicated rows; queries are rows of them (a query equal to a
    row) and fresh integer vectors; pair lists: all V words, none, one, the same word twice,
    then a few random ones."""
    rng = np.random.default_rng(seed)
    e = ref.integer_embeddings(v, d, seed)
    queries = rng.integers(-8, 9, size=(q, d)).astype(np.float32)
    for i in range(0, q, 2):
        queries[i] = e[rng.integers(0, v)]
    lists = []
    for i in range(q):
        kind = i % 5
        if kind == 0:
            lists.append(np.arange(v))
        elif kind == 1:
            lists.append(np.zeros(0, dtype=np.int64))
        elif kind == 2:
            lists.append(rng.integers(0, v, 1))
        elif kind == 3:
            w = rng.integers(0, v)
            lists.append(np.array([w, w]))
        else:
            lists.append(rng.integers(0, v, 7))
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return e, queries, ptr, np.concatenate(lists).astype(np.int32)


@pytest.mark.parametrize("v,d,q", EXACT_SHAPES)
def test_exact_data_gives_the_float64_ordering(cuda, v, d, q):
    e, queries, ptr, word = exact_problem(v, d, q, seed=v + 31 * d + q)
    want = ref.neighbour_ranks(e, queries, ptr, word)
    ed, qd = torch.as_tensor(e, device=cuda), torch.as_tensor(queries, device=cuda)
    got = dl.neighbour_ranks(ed, qd, ptr, word).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if v > 1:
        assert len(np.unique(ref.dist2(e, queries[0]))) < v  # there are ties to break
    first = got[:v]  # query 0 lists all V words: a permutation
    assert np.array_equal(np.sort(first), np.arange(v))
    for k in sorted({1, min(2, v), min(v, MAX_K)}):
        dist, idx = dl.kneighbors(ed, qd, k)
        want_dist, want_idx = ref.kneighbors(e, queries, k)
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), want_idx)
        # d2 is exact; the square root on top of it is within an ulp of float32
        assert np.all(np.abs(dist.cpu().numpy() - want_dist) <= 2.0 ** -23 * want_dist)
        if k == v:  # the rank vector is the inverse of the index row
            assert np.array_equal(idx[0].cpu().numpy()[first], np.arange(v))


@pytest.mark.parametrize("v,k,q", [(MERGE, ROW_T, 2), (MERGE + 1, ROW_T, 9), (40000, MAX_K, 3),
                                   (MERGE // 50 * ROW_T + 1, 50, 2)])
def test_kneighbors_across_the_merge_slice(cuda, v, k, q):
    """ceil(V / 256) * min(k, 256) candidates per query: at most one merge slice (one level),
    one more, and several slices; three columns of small integers, so ties cross the slices."""
    e = ref.integer_embeddings(v, 3, seed=v + k, span=8)
    rows = np.random.default_rng(k).choice(v, q, replace=False)
    dist, idx = dl.kneighbors(e, rows, k)
    want_dist, want_idx = ref.kneighbors(e, rows, k)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.all(np.abs(dist.cpu().numpy() - want_dist) <= 2.0 ** -23 * want_dist)


@pytest.mark.parametrize("n_pairs", [SLOTS - 1, SLOTS, SLOTS + 1])
def test_pair_count_across_the_lds_slot_capacity(cuda, n_pairs):
    v, d = 2100, 5
    e = ref.integer_embeddings(v, d, seed=n_pairs, span=3)
    word = np.random.default_rng(n_pairs).permutation(v)[:n_pairs].astype(np.int32)
    ptr = np.array([0, n_pairs, n_pairs], dtype=np.int32)
    got = dl.neighbour_ranks(e, np.array([5, 9]), ptr, word).cpu().numpy()
    assert np.array_equal(got, ref.neighbour_ranks(e, [5, 9], ptr, word))


def test_index_queries_strided_rows_and_a_large_tile_of_pairs(cuda):
    """Queries as rows of embs; embeddings as a view with a row stride that forbids 16-B loads
    and NaN in the padding; two queries that each list every word (more pairs in one query tile
    than the LDS slots hold, so the counts go to HBM)."""
    v, d = 2000, 6
    e = ref.integer_embeddings(v, d, seed=3, span=2)
    padded = torch.full((v, d + 3), float("nan"), device=cuda)
    padded[:, :d] = torch.as_tensor(e)
    view = padded[:, :d]
    rows = np.array([7, 1999, 0], dtype=np.int64)
    ptr = np.array([0, v, 2 * v, 2 * v + 1], dtype=np.int32)
    word = np.concatenate([np.arange(v), np.arange(v)[::-1], [4]]).astype(np.int32)
    want = ref.neighbour_ranks(e, rows, ptr, word)
    for queries in (rows, torch.as_tensor(rows, device=cuda), torch.as_tensor(rows.astype(np.int32))):
        assert np.array_equal(dl.neighbour_ranks(view, queries, ptr, word).cpu().numpy(), want)
    dist, idx = dl.kneighbors(view, rows, 9)
    assert np.array_equal(idx.cpu().numpy(), ref.kneighbors(e, rows, 9)[1])
    assert torch.isnan(padded[:, d:]).all()
    # device-resident pair arrays: the status word reports what the host check cannot see
    bad_word = torch.as_tensor(word, device=cuda).clone()
    bad_word[5] = v
    with pytest.raises(ValueError, match="outside"):
        dl.neighbour_ranks(view, rows, ptr, bad_word)
    bad_ptr = torch.as_tensor(np.array([0, 2 * v, v, 2 * v + 1], dtype=np.int32), device=cuda)
    with pytest.raises(ValueError, match="pair_ptr"):
        dl.neighbour_ranks(view, rows, bad_ptr, torch.as_tensor(word, device=cuda))
    with pytest.raises(ValueError, match="non-finite"):
        dl.neighbour_ranks(padded[:, :d + 1], padded[:3, :d + 1], ptr, word)
    with pytest.raises(ValueError, match="non-finite"):
        dl.kneighbors(padded[:, :d + 1], padded[:3, :d + 1], 2)


# ---------------------------------------------------------------- real-valued data

REAL_V, REAL_D, REAL_Q, REAL_GOLD, REAL_SEED = 2000, 64, 6, 100, 11


@pytest.fixture(scope="module")
def real(cuda):
    """Gaussian rows through scale_embeddings (the float32 device result is the data of both
    sides), Q queries that are rows, ~100 gold words each, and the float64 distances."""
    x = ref.gaussian_embeddings(REAL_V, REAL_D, REAL_SEED)
    scaled = dl.scale_embeddings(torch.as_tensor(x, device=cuda))
    e64 = scaled.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(REAL_SEED)
    rows = rng.choice(REAL_V, REAL_Q, replace=False)
    word = np.concatenate([np.sort(rng.choice(REAL_V, REAL_GOLD, replace=False))
                           for _ in range(REAL_Q)]).astype(np.int32)
    ptr = (np.arange(REAL_Q + 1) * REAL_GOLD).astype(np.int32)
    d64 = np.stack([ref.dist2(e64, e64[r]) for r in rows])
    return {"x": x, "scaled": scaled, "e64": e64, "rows": rows, "ptr": ptr, "word": word, "d64": d64}


def test_real_data_ranks_lie_in_the_derived_band(real):
    g = ref.gamma(REAL_D)
    bounds = np.array([ref.rank_bounds(real["d64"][p // REAL_GOLD], w, g)
                       for p, w in enumerate(real["word"])])
    lo, hi = bounds[:, 0], bounds[:, 1]
    tight = float(np.mean(hi - 1 == lo))
    print(f"gamma {g:.3g}: {100 * tight:.1f} % of {len(lo)} pairs have one admissible rank")
    assert tight >= 0.8  # on the CPU, before the GPU result: the band is not vacuous
    got = dl.neighbour_ranks(real["scaled"], real["rows"], real["ptr"], real["word"]).cpu().numpy()
    print(f"ranks off the float64 rank: {int(np.sum(got != ref.neighbour_ranks(real['e64'], real['rows'], real['ptr'], real['word'])))}")
    assert np.all(lo <= got) and np.all(got <= hi - 1)


def test_real_data_kneighbors(real):
    g, k = ref.gamma(REAL_D), 50
    dist, idx = dl.kneighbors(real["scaled"], real["rows"], k)
    dist, idx = dist.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    assert np.all(np.diff(dist, axis=1) >= 0)
    for q in range(REAL_Q):
        d64 = real["d64"][q]
        assert len(set(idx[q].tolist())) == k and idx[q, 0] == real["rows"][q] and dist[q, 0] == 0
        assert np.all(np.abs(dist[q] - np.sqrt(d64[idx[q]])) <= g * np.sqrt(d64[idx[q]]))
        order = np.lexsort((np.arange(REAL_V), d64))
        kth = d64[order[k - 1]]
        for v in set(idx[q].tolist()) ^ set(order[:k].tolist()):  # only words in the k-th's band
            assert d64[v] * (1 - g) <= kth * (1 + g) and d64[v] * (1 + g) >= kth * (1 - g)


# ---------------------------------------------------------------- scale_embeddings

def scale_close(got, want, d):
    """Every element within (D + 4) 2^-24 relative of the float64 value."""
    got = got.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    print(f"scale: worst relative error {np.max(err / np.maximum(np.abs(want), 1e-300)):.3g}, "
          f"bound {(d + 4) * 2.0 ** -24:.3g}")
    return bool(np.all(err <= (d + 4) * 2.0 ** -24 * np.abs(want)))


@pytest.mark.parametrize("name", ["small", "medium", "wide"])
def test_scale_embeddings_against_the_sklearn_fixture(cuda, name):
    z = np.load(os.path.join(GOLDEN, f"dialect_{name}.npz"))
    got = dl.scale_embeddings(z["embs"])
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == z["embs"].shape
    assert scale_close(got, z["scaled"], z["embs"].shape[1])
    assert scale_close(got, ref.scale(z["embs"]), z["embs"].shape[1])


@pytest.mark.parametrize("v", [1, 2, MM_ROWS - 1, MM_ROWS, MM_ROWS + 1, 2 * MM_ROWS + 3])
def test_scale_embeddings_edge_cases(cuda, v):
    d = 67
    x = ref.gaussian_embeddings(v, d, seed=v)
    x[:, 5] = -2.25                  # a constant column: scale 1, all zeros
    if v > 2:
        x[v // 2] = x.min(axis=0)    # every element the column's minimum: an all-zero row
        x[-1, 3] = x[:, 3].max() + 1  # the maximum in the last row block
    want = ref.scale(x)
    padded = torch.full((v, d + 5), float("nan"), device=cuda)
    padded[:, :d] = torch.as_tensor(x)
    got = dl.scale_embeddings(padded[:, :d])     # a row stride, NaN in the padding
    assert scale_close(got, want, d)
    assert not got[:, 5].any() and torch.isnan(padded[:, d:]).all()
    if v > 2:
        assert not got[v // 2].any() and not want[v // 2].any()
        assert np.allclose(got.sum(dim=1).cpu().numpy()[np.arange(v) != v // 2], 1.0, atol=1e-5)
    else:
        assert v == 2 or not got.any()           # V = 1: every column is constant
    assert torch.equal(got, dl.scale_embeddings(x))
    bad = padded.clone()
    bad[v - 1, d - 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        dl.scale_embeddings(bad[:, :d])


# ---------------------------------------------------------------- determinism

def test_bitwise_reproducible_and_row_consistent(real, cuda):
    e, rows = real["scaled"], real["rows"]
    batch = torch.as_tensor(np.resize(rows, 17), device=cuda)
    ptr = (np.arange(18) * 3).astype(np.int32)
    word = np.random.default_rng(2).integers(0, REAL_V, 51).astype(np.int32)
    first = (dl.neighbour_ranks(e, batch, ptr, word), *dl.kneighbors(e, batch, 33),
             dl.scale_embeddings(real["x"]))
    again = (dl.neighbour_ranks(e, batch, ptr, word), *dl.kneighbors(e, batch, 33),
             dl.scale_embeddings(real["x"]))
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        third = (dl.neighbour_ranks(e, batch, ptr, word), *dl.kneighbors(e, batch, 33),
                 dl.scale_embeddings(real["x"]))
    side.synchronize()
    for a, b, c in zip(first, again, third):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(first[3], real["scaled"])
    # a query alone (the 8-query tile) gives the row it has in the batch of 17 (the 32-query tile)
    for i in (0, 5, 16):
        alone_rank = dl.neighbour_ranks(e, batch[i:i + 1], np.array([0, 3], dtype=np.int32),
                                        word[3 * i:3 * i + 3])
        alone_dist, alone_idx = dl.kneighbors(e, batch[i:i + 1], 33)
        assert torch.equal(alone_rank, first[0][3 * i:3 * i + 3])
        assert torch.equal(alone_dist[0], first[1][i]) and torch.equal(alone_idx[0], first[2][i])
    # the two entries share their distances: index[q, r] == w exactly when rank(q, w) == r
    allptr = np.array([0, REAL_V], dtype=np.int32)
    rank = dl.neighbour_ranks(e, batch[:1], allptr, np.arange(REAL_V, dtype=np.int32)).cpu().numpy()
    _, idx = dl.kneighbors(e, batch[:1], MAX_K)
    assert np.array_equal(rank[idx[0].cpu().numpy()], np.arange(MAX_K))


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def planted(cuda):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import dialect_pipeline as dp
    X, region, vocab, gold = dp.synthetic_problem(n_users=3000, regions=6, planted=40, vocab_size=3000)
    clf, embs, _ = dp.word_embeddings(X, region, vocab)
    return {"X": X, "vocab": vocab, "lexicon": dl.DialectLexicon(gold), "clf": clf, "embs": embs}


def test_get_embedding_as_tensor_equals_the_numpy_form(planted):
    eye = planted["X"][:50]
    as_numpy = planted["clf"].get_embedding(eye)
    as_tensor = planted["clf"].get_embedding(eye, as_tensor=True)
    assert isinstance(as_numpy, np.ndarray) and as_tensor.is_cuda and as_tensor.dtype == torch.float32
    assert np.array_equal(as_tensor.cpu().numpy(), as_numpy)
    assert np.array_equal(planted["clf"].get_embedding(eye, False), as_numpy)


def test_eval_embeddings_on_the_planted_problem(planted, cuda):
    vocab, lex, embs = planted["vocab"], planted["lexicon"], planted["embs"]
    ks = (10, 40, 80, 200, 1000)
    res = dl.eval_embeddings(vocab, embs, lex, ks=ks)
    p = lex.pairs(vocab)
    assert res.dialects == [f"region{r}" for r in range(6)] and res.totals.tolist() == [40] * 6
    # the restatement on the same (device-scaled) embeddings
    scaled = dl.scale_embeddings(embs).cpu().numpy()
    want_ranks = ref.neighbour_ranks(scaled, p.rows, p.pair_ptr, p.pair_word)
    micro, per = ref.recall_at_k(want_ranks, p.pair_ptr, p.n_missing, ks)
    print(f"micro recall at {ks}: {res.micro}; ranks off float64: "
          f"{int(np.sum(res.ranks.cpu().numpy() != want_ranks))}")
    assert res.micro == micro and np.array_equal(res.per_dialect, per)
    # dialect_eval's call: other ks, no scaling; and the host form of the same embeddings
    raw = dl.eval_embeddings(vocab, embs.cpu().numpy(), lex, ks=[40], scale=False)
    want_raw = ref.neighbour_ranks(embs.cpu().numpy(), p.rows, p.pair_ptr, p.pair_word)
    assert raw.micro == ref.recall_at_k(want_raw, p.pair_ptr, p.n_missing, [40])[0]
    # trained embeddings find the planted words; shuffled rows do not
    perm = torch.as_tensor(np.random.default_rng(0).permutation(len(vocab)), device=cuda)
    shuffled = dl.eval_embeddings(vocab, embs[perm], lex, ks=[40])
    print(f"recall at 40: trained {res.micro[1]:.2f}, shuffled rows {shuffled.micro[0]:.2f}")
    assert res.micro[1] > shuffled.micro[0] and res.micro[1] > 5 * 100.0 * 40 / len(vocab)
    # a gold word outside the vocabulary counts in the denominator
    more = dl.DialectLexicon({k: set(v) | {"nowhere"} for k, v in lex.words.items()})
    res2 = dl.eval_embeddings(vocab, embs, more, ks=ks)
    assert res2.totals.tolist() == [41] * 6 and torch.equal(res2.ranks, res.ranks)
    assert res2.micro == pytest.approx([m * 240 / 246 for m in micro], rel=1e-12)


def test_eval_embeddings_reads_back_once(planted, cuda):
    vocab, lex, embs = planted["vocab"], planted["lexicon"], planted["embs"]
    want = dl.eval_embeddings(vocab, embs, lex, ks=(40, 80))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = dl.eval_embeddings(vocab, embs, lex, ks=(40, 80))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message).lower()]
    print(f"eval_embeddings: {len(syncs)} torch-visible synchronisations")
    assert len(syncs) <= 1
    assert got.micro == want.micro and torch.equal(got.ranks, want.ranks)


def test_dialect_pipeline_example(cuda):
    """The example as a user runs it: its own process, under a time limit; it asserts its own
    claim (a non-zero exit otherwise)."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dialect_pipeline.py"),
                          "--users", "2000", "--vocab", "2000", "--epochs", "6"],
                         capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stderr[-2000:]
    out = run.stdout.strip().splitlines()
    rec = json.loads(out[-1])
    assert len(out) == 1 + rec["dialects"] == 7 and rec["vocab"] == 2000
    assert rec["micro_recall"][0] > 5 * rec["chance_recall"][0]
