"""The size contract of every entry that works in a caller's workspace and runs hipcub, and of
the dense entries that keep bf16 planes or split-K partials in one: claiming
one byte less than the entry reports is GCG_ERR_WORKSPACE, names the entry in gcg_last_error() and
leaves the outputs alone; claiming exactly what it reports works. The buffer behind the claim always
has the full size, so nothing can be written out of bounds. Tiny inputs, references in numpy."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GCG_OK, GCG_ERR_WORKSPACE = 0, 6
SENTINEL = 0x5A


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def out(shape, dtype, cuda):
    """An output buffer filled with the sentinel byte."""
    t = torch.empty(shape, dtype=dtype, device=cuda)
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def untouched(t):
    return bool((t.view(torch.uint8) == SENTINEL).all().item())


def run_contract(lib, cuda, name, need, call, outputs):
    """`call(ws, claimed_bytes)` -> status. Short claim first, then the exact one."""
    assert need > 0, f"{name}: this shape needs no workspace, so it cannot check the contract"
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    assert ws.data_ptr() % 256 == 0
    st = call(ws, need - 1)
    msg = lib.gcg_last_error().decode()
    torch.cuda.synchronize(cuda)
    assert st == GCG_ERR_WORKSPACE, (name, st, msg)
    assert name in msg, (name, msg)
    for i, t in enumerate(outputs):
        assert untouched(t), f"{name}: output {i} written by the refused call"
    st = call(ws, need)
    torch.cuda.synchronize(cuda)
    assert st == GCG_OK, (name, st, lib.gcg_last_error().decode())


def reported(lib, name, *sizes):
    b = C.c_size_t(0)
    assert getattr(lib, name)(*sizes, C.byref(b)) == GCG_OK, lib.gcg_last_error()
    return b.value


# ---- csr_ops / graph_build: entries that report through workspace_needed ------------------------

def test_index_csr(native_lib, cuda):
    lib = native_lib
    idx = np.array([3, 0, 5, 3, 3, 1, 0, 5, 2, 3], np.int32)
    n_rows = 6
    need = C.c_size_t(0)
    assert lib.gcg_index_csr(len(idx), None, n_rows, None, None, None, 0, C.byref(need), None) == GCG_OK
    idx_d = dev(idx, cuda)
    seg_ptr, pos = out(n_rows + 1, torch.int32, cuda), out(len(idx), torch.int32, cuda)
    run_contract(lib, cuda, "gcg_index_csr", need.value,
                 lambda ws, b: lib.gcg_index_csr(len(idx), ptr(idx_d), n_rows, ptr(seg_ptr), ptr(pos),
                                                 ptr(ws), b, None, None), [seg_ptr, pos])
    order = np.argsort(idx, kind="stable")
    np.testing.assert_array_equal(pos.cpu().numpy(), order)
    np.testing.assert_array_equal(seg_ptr.cpu().numpy(),
                                  np.searchsorted(idx[order], np.arange(n_rows + 1)))


def test_csr_transpose(native_lib, cuda):
    lib = native_lib
    indptr = np.array([0, 2, 2, 5, 6, 6, 8], np.int32)          # 6 x 5, 8 entries, empty rows
    indices = np.array([1, 4, 0, 1, 3, 4, 0, 2], np.int32)
    vals = np.arange(1, 9, dtype=np.float32)
    n_rows, n_cols, nnz = 6, 5, 8
    need = C.c_size_t(0)
    assert lib.gcg_csr_transpose_f32(n_rows, n_cols, nnz, None, None, None, None, None, None, None, 0,
                                     C.byref(need), None) == GCG_OK
    a, b_, c = dev(indptr, cuda), dev(indices, cuda), dev(vals, cuda)
    o_ptr, o_idx, o_val = (out(n_cols + 1, torch.int32, cuda), out(nnz, torch.int32, cuda),
                           out(nnz, torch.float32, cuda))
    run_contract(lib, cuda, "gcg_csr_transpose_f32", need.value,
                 lambda ws, b: lib.gcg_csr_transpose_f32(n_rows, n_cols, nnz, ptr(a), ptr(b_), ptr(c),
                                                         ptr(o_ptr), ptr(o_idx), ptr(o_val), ptr(ws),
                                                         b, None, None), [o_ptr, o_idx, o_val])
    row_of = np.repeat(np.arange(n_rows), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    np.testing.assert_array_equal(o_ptr.cpu().numpy(), np.searchsorted(indices[order], np.arange(n_cols + 1)))
    np.testing.assert_array_equal(o_idx.cpu().numpy(), row_of[order])
    np.testing.assert_array_equal(o_val.cpu().numpy(), vals[order])


def test_normalize_adjacency(native_lib, cuda):
    lib = native_lib
    n = 6
    u = np.array([0, 1, 2, 3, 4, 0, 1, 3], np.int32)   # 8 edges, (1, 2) twice, node 5 isolated
    v = np.array([1, 2, 3, 4, 0, 2, 2, 0], np.int32)
    m = 2 * len(u) + n
    need = C.c_size_t(0)
    assert lib.gcg_normalize_adjacency_f32(n, len(u), None, None, 1, None, None, None, None, None, 0,
                                           C.byref(need), None, None) == GCG_OK
    u_d, v_d = dev(u, cuda), dev(v, cuda)
    indptr, indices, vals = (out(n + 1, torch.int32, cuda), out(m, torch.int32, cuda),
                             out(m, torch.float32, cuda))
    nnz, status = out(1, torch.int64, cuda), out(1, torch.int32, cuda)
    run_contract(lib, cuda, "gcg_normalize_adjacency_f32", need.value,
                 lambda ws, b: lib.gcg_normalize_adjacency_f32(
                     n, len(u), ptr(u_d), ptr(v_d), 1, ptr(indptr), ptr(indices), ptr(vals), ptr(nnz),
                     ptr(ws), b, None, ptr(status), None), [indptr, indices, vals, nnz, status])
    A = np.eye(n, dtype=bool)
    A[u, v] = A[v, u] = True
    d = A.sum(1).astype(np.float64)
    dinv = 1.0 / np.sqrt(d)
    rows, cols = np.nonzero(A)
    k = int(nnz.item())
    assert status.item() == 0 and k == len(rows)
    np.testing.assert_array_equal(indptr.cpu().numpy(), np.searchsorted(rows, np.arange(n + 1)))
    np.testing.assert_array_equal(indices.cpu().numpy()[:k], cols)
    np.testing.assert_array_equal(vals.cpu().numpy()[:k], (dinv[rows] * dinv[cols]).astype(np.float32))


# ---- minibatch --------------------------------------------------------------------------------

def test_minibatch_segment(native_lib, cuda):
    lib = native_lib
    n_rows, n_cols, batch = 6, 7, 2
    indptr = np.array([0, 3, 3, 5, 9, 10, 12], np.int32)
    indices = np.array([0, 3, 6, 1, 3, 0, 2, 3, 5, 4, 1, 6], np.int32)
    vals = np.arange(1, 13, dtype=np.float32)
    perm = np.array([3, 0, 5, 2], np.int32)            # two batches of two rows
    n_sel = len(perm)
    lens = np.diff(indptr)[perm]
    nnz_sel = int(lens.sum())
    cap, need = C.c_int64(0), C.c_size_t(0)
    assert lib.gcg_minibatch_segment_sizes(n_sel, batch, n_cols, nnz_sel, C.byref(cap),
                                           C.byref(need)) == GCG_OK
    nb = n_sel // batch
    assert cap.value == min(nnz_sel, nb * n_cols) + 1
    a, b_, c, p = dev(indptr, cuda), dev(indices, cuda), dev(vals, cuda), dev(perm, cuda)
    bsp, seg_col, seg_ptr = (out(nb + 1, torch.int32, cuda), out(cap.value, torch.int32, cuda),
                             out(cap.value + 1, torch.int32, cuda))
    ent_pos, ent_val = out(nnz_sel, torch.int32, cuda), out(nnz_sel, torch.float32, cuda)
    run_contract(lib, cuda, "gcg_minibatch_segment", need.value,
                 lambda ws, b: lib.gcg_minibatch_segment(
                     n_rows, n_cols, ptr(a), ptr(b_), ptr(c), ptr(p), n_sel, batch, nnz_sel, ptr(bsp),
                     ptr(seg_col), ptr(seg_ptr), ptr(ent_pos), ptr(ent_val), ptr(ws), b, None),
                 [bsp, seg_col, seg_ptr, ent_pos, ent_val])
    # reference: entries in (batch, column) order, stable in (position in batch, storage order)
    ents = []
    for i, r in enumerate(perm):
        for j in range(indptr[r], indptr[r + 1]):
            ents.append((i // batch, int(indices[j]), i % batch, float(vals[j])))
    ents.sort(key=lambda e: (e[0], e[1]))
    keys = [(e[0], e[1]) for e in ents]
    starts = [i for i, k in enumerate(keys) if i == 0 or k != keys[i - 1]]
    n_seg = len(starts)
    bsp_ref = np.searchsorted([keys[s][0] for s in starts], np.arange(nb + 1))
    np.testing.assert_array_equal(bsp.cpu().numpy(), bsp_ref)
    np.testing.assert_array_equal(seg_col.cpu().numpy()[:n_seg], [keys[s][1] for s in starts])
    np.testing.assert_array_equal(seg_ptr.cpu().numpy()[:n_seg + 1], starts + [len(ents)])
    np.testing.assert_array_equal(ent_pos.cpu().numpy(), [e[2] for e in ents])
    np.testing.assert_array_equal(ent_val.cpu().numpy(), np.array([e[3] for e in ents], np.float32))


# ---- tfidf: 5 documents, 40 tokens, 7 terms ------------------------------------------------------

N_DOCS, N_TERMS = 5, 7


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(7)
    lens = np.array([12, 0, 9, 14, 5])
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tokens = rng.integers(0, N_TERMS, 40).astype(np.int32)
    tokens[[3, 17]] = [-1, N_TERMS]                     # dropped ids
    dense = np.zeros((N_DOCS, N_TERMS), np.int32)
    for d in range(N_DOCS):
        for t in tokens[doc_ptr[d]:doc_ptr[d + 1]]:
            if 0 <= t < N_TERMS:
                dense[d, t] += 1
    return doc_ptr, tokens, dense


@pytest.mark.parametrize("df_mode", [0, 1])
def test_tfidf_count(native_lib, cuda, corpus, df_mode):
    lib = native_lib
    doc_ptr, tokens, dense = corpus
    n_tok = len(tokens)
    need = reported(lib, "gcg_tfidf_count_workspace_bytes", N_DOCS, n_tok, N_TERMS)
    p, t = dev(doc_ptr, cuda), dev(tokens, cuda)
    indptr, indices, counts = (out(N_DOCS + 1, torch.int32, cuda), out(n_tok, torch.int32, cuda),
                               out(n_tok, torch.int32, cuda))
    nnz = torch.zeros(1, dtype=torch.int64, device=cuda)
    df = torch.zeros(N_TERMS, dtype=torch.int64, device=cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    run_contract(lib, cuda, "gcg_tfidf_count", need,
                 lambda ws, b: lib.gcg_tfidf_count(N_DOCS, N_TERMS, n_tok, ptr(p), ptr(t), None,
                                                   ptr(indptr), ptr(indices), ptr(counts), n_tok,
                                                   ptr(nnz), ptr(df), df_mode, ptr(status), ptr(ws), b,
                                                   None), [indptr, indices, counts])
    rows, cols = np.nonzero(dense)
    k = int(nnz.item())
    assert status.item() == 0 and k == len(rows)
    np.testing.assert_array_equal(indptr.cpu().numpy(), np.searchsorted(rows, np.arange(N_DOCS + 1)))
    np.testing.assert_array_equal(indices.cpu().numpy()[:k], cols)
    np.testing.assert_array_equal(counts.cpu().numpy()[:k], dense[rows, cols])
    np.testing.assert_array_equal(df.cpu().numpy(), (dense > 0).sum(0))


def test_tfidf_select(native_lib, cuda, corpus):
    lib = native_lib
    df = (corpus[2] > 0).sum(0).astype(np.int64)
    lo, hi = 2, 3
    need = reported(lib, "gcg_tfidf_select_workspace_bytes", N_TERMS)
    df_d = dev(df, cuda)
    new_id, kept_df, n_kept = (out(N_TERMS, torch.int32, cuda), out(N_TERMS, torch.int64, cuda),
                               out(1, torch.int64, cuda))
    run_contract(lib, cuda, "gcg_tfidf_select", need,
                 lambda ws, b: lib.gcg_tfidf_select(N_TERMS, ptr(df_d), lo, hi, ptr(new_id), ptr(kept_df),
                                                    ptr(n_kept), ptr(ws), b, None),
                 [new_id, kept_df, n_kept])
    keep = (df >= lo) & (df <= hi)
    assert 0 < keep.sum() < N_TERMS
    np.testing.assert_array_equal(new_id.cpu().numpy(), np.where(keep, np.cumsum(keep) - 1, -1))
    assert n_kept.item() == keep.sum()
    np.testing.assert_array_equal(kept_df.cpu().numpy()[:keep.sum()], df[keep])


def test_tfidf_compact(native_lib, cuda, corpus):
    lib = native_lib
    dense = corpus[2]
    rows, cols = np.nonzero(dense)
    indptr = np.searchsorted(rows, np.arange(N_DOCS + 1)).astype(np.int32)
    new_id = np.array([0, -1, 1, 2, -1, -1, 3], np.int32)
    need = reported(lib, "gcg_tfidf_compact_workspace_bytes", N_DOCS)
    a, b_, c, d = (dev(indptr, cuda), dev(cols.astype(np.int32), cuda),
                   dev(dense[rows, cols].astype(np.int32), cuda), dev(new_id, cuda))
    o_ptr = out(N_DOCS + 1, torch.int32, cuda)
    run_contract(lib, cuda, "gcg_tfidf_compact", need,       # the sizing call is the one with scratch
                 lambda ws, b: lib.gcg_tfidf_compact(N_DOCS, N_TERMS, len(rows), ptr(a), ptr(b_), ptr(c),
                                                     ptr(d), ptr(o_ptr), None, None, 0, ptr(ws), b, None),
                 [o_ptr])
    kept = new_id[cols] >= 0
    np.testing.assert_array_equal(o_ptr.cpu().numpy(), np.searchsorted(rows[kept], np.arange(N_DOCS + 1)))


# ---- tokenize -----------------------------------------------------------------------------------

TEXTS = ["the cat sat on the mat", "", "a dog; the #cat and the d0g", "sat sat sat on x yz",
         "café olé the end"]


@pytest.fixture(scope="module")
def marked(native_lib, cuda):
    """The corpus marked once (with the full workspace): what the terms test starts from."""
    from graphconvgeo_amd import tfidf
    lib = native_lib
    buf = "\x00".join(TEXTS).encode("utf-8")
    n = len(buf)
    n16 = (n + 15) // 16 * 16
    text = torch.zeros(n16, dtype=torch.uint8, device=cuda)
    text[:n].copy_(torch.frombuffer(bytearray(buf), dtype=torch.uint8))
    table = torch.from_numpy(tfidf.word_char_table().copy()).to(cuda)
    tiles = -(-n // lib.gcg_tokenize_tile_bytes())
    return buf, text, table, n16, tiles


def host_tokens():
    docs = [re.findall(r"(?u)\b\w\w+\b", t) for t in TEXTS]
    flat = [w for d in docs for w in d]
    names = list(dict.fromkeys(flat))                   # the terms in order of first appearance
    tok_term = np.array([names.index(w) for w in flat], np.int32)
    doc_ptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return names, tok_term, doc_ptr


def mark(lib, cuda, marked, ws, claimed, flags, tile_base, totals):
    buf, text, table, _, _ = marked
    return lib.gcg_tokenize_mark(len(buf), ptr(text), ptr(table), 0, ptr(flags), ptr(tile_base),
                                 ptr(totals), ptr(ws), claimed, None)


def test_tokenize_mark(native_lib, cuda, marked):
    lib = native_lib
    buf, _, _, n16, tiles = marked
    need = reported(lib, "gcg_tokenize_mark_workspace_bytes", len(buf))
    flags, tile_base, totals = (out(n16, torch.uint8, cuda), out(tiles + 1, torch.int64, cuda),
                                out(2, torch.int64, cuda))
    run_contract(lib, cuda, "gcg_tokenize_mark", need,
                 lambda ws, b: mark(lib, cuda, marked, ws, b, flags, tile_base, totals),
                 [flags, tile_base, totals])
    names, tok_term, _ = host_tokens()
    assert totals.tolist() == [len(tok_term), len(TEXTS) - 1]


def test_tokenize_terms_and_remap(native_lib, cuda, marked):
    lib = native_lib
    buf, text, _, n16, tiles = marked
    names, tok_ref, ptr_ref = host_tokens()
    n_tok, n_docs = len(tok_ref), len(TEXTS)
    assert n_tok >= 20 and len(names) < n_tok
    flags = torch.empty(n16, dtype=torch.uint8, device=cuda)
    tile_base = torch.empty(tiles + 1, dtype=torch.int64, device=cuda)
    totals = torch.zeros(2, dtype=torch.int64, device=cuda)
    ws = torch.empty(reported(lib, "gcg_tokenize_mark_workspace_bytes", len(buf)), dtype=torch.uint8,
                     device=cuda)
    assert mark(lib, cuda, marked, ws, ws.numel(), flags, tile_base, totals) == GCG_OK
    for hash_bits in (64, 3):  # 3 bits: terms share hashes and the byte comparison decides
        need = reported(lib, "gcg_tokenize_terms_workspace_bytes", n_tok, hash_bits)
        doc_ptr, tok_term = out(n_docs + 1, torch.int64, cuda), out(n_tok, torch.int32, cuda)
        t_start, t_len = out(n_tok, torch.int64, cuda), out(n_tok, torch.int32, cuda)
        result = out(2, torch.int64, cuda)
        run_contract(lib, cuda, "gcg_tokenize_terms", need,
                     lambda w, b: lib.gcg_tokenize_terms(
                         len(buf), ptr(text), ptr(flags), ptr(tile_base), n_tok, n_docs, None, hash_bits,
                         ptr(doc_ptr), ptr(tok_term), ptr(t_start), ptr(t_len), ptr(result), ptr(w), b,
                         None), [doc_ptr, tok_term, t_start, t_len, result])
        n_terms, collision = result.tolist()
        if hash_bits == 64:
            assert collision == 0
        if not collision:
            np.testing.assert_array_equal(doc_ptr.cpu().numpy(), ptr_ref)
            assert n_terms == len(names)
            np.testing.assert_array_equal(tok_term.cpu().numpy(), tok_ref)
            s, ln = t_start.cpu().numpy()[:n_terms], t_len.cpu().numpy()[:n_terms]
            assert [buf[a:a + b].decode() for a, b in zip(s, ln)] == names
    # remap: drop "the" and "sat", number the rest
    keep = np.array([w not in ("the", "sat") for w in names])
    action = np.where(keep, np.cumsum(keep) - 1, -2).astype(np.int32)
    need = reported(lib, "gcg_tokenize_remap_workspace_bytes", n_tok)
    tt, act, pin = dev(tok_ref, cuda), dev(action, cuda), dev(ptr_ref, cuda)
    tokens, p_out = out(n_tok, torch.int32, cuda), out(n_docs + 1, torch.int64, cuda)
    run_contract(lib, cuda, "gcg_tokenize_remap", need,
                 lambda w, b: lib.gcg_tokenize_remap(n_tok, ptr(tt), len(names), ptr(act), n_docs, ptr(pin),
                                                     ptr(tokens), ptr(p_out), ptr(w), b, None),
                 [tokens, p_out])
    kept_tok = keep[tok_ref]
    pos = np.concatenate([[0], np.cumsum(kept_tok)])
    np.testing.assert_array_equal(p_out.cpu().numpy(), pos[ptr_ref])
    np.testing.assert_array_equal(tokens.cpu().numpy()[:pos[-1]], action[tok_ref][kept_tok])


# ---- kmeans: 9 points in 3 clusters --------------------------------------------------------------

LOCS = np.array([[0.0, 0.1], [0.2, -0.1], [-0.1, 0.3], [5.0, 5.2], [5.3, 4.9], [4.8, 5.1],
                 [-4.0, 6.0], [-4.2, 6.3], [-3.9, 5.8]])
LABELS = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2], np.int32)
F64 = 1e-13  # a few float64 roundings on values of order 1 to 100


def test_kmeans_assign(native_lib, cuda):
    lib = native_lib
    N, Cn = len(LOCS), 3
    centers = np.array([[0.0, 0.0], [5.0, 5.0], [-4.0, 6.0]])
    need = reported(lib, "gcg_kmeans_assign_f64_workspace_bytes", N)
    x, c = dev(LOCS, cuda), dev(centers, cuda)
    labels, dist2 = out(N, torch.int32, cuda), out(N, torch.float64, cuda)
    inertia, status = out(1, torch.float64, cuda), torch.zeros(1, dtype=torch.int32, device=cuda)
    # the workspace holds the inertia's partial sums: asked for only with inertia_dev
    run_contract(lib, cuda, "gcg_kmeans_assign_f64", need,
                 lambda ws, b: lib.gcg_kmeans_assign_f64(N, ptr(x), Cn, ptr(c), None, ptr(labels),
                                                         ptr(dist2), ptr(inertia), None, ptr(status),
                                                         ptr(ws), b, None), [labels, dist2, inertia])
    d2 = ((LOCS[:, None, :] - centers[None]) ** 2).sum(-1)
    assert status.item() == 0
    np.testing.assert_array_equal(labels.cpu().numpy(), d2.argmin(1))
    np.testing.assert_allclose(dist2.cpu().numpy(), d2.min(1), rtol=F64)
    np.testing.assert_allclose(inertia.item(), d2.min(1).sum(), rtol=F64)


def test_kmeans_update_and_cluster_stats(native_lib, cuda):
    lib = native_lib
    N, Cn = len(LOCS), 4                                 # cluster 3 is empty
    prev = np.arange(8, dtype=np.float64).reshape(4, 2)
    x, lab, pv = dev(LOCS, cuda), dev(LABELS, cuda), dev(prev, cuda)
    need = reported(lib, "gcg_kmeans_update_f64_workspace_bytes", N, Cn)
    centers, counts = out((Cn, 2), torch.float64, cuda), out(Cn, torch.int32, cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    run_contract(lib, cuda, "gcg_kmeans_update_f64", need,
                 lambda ws, b: lib.gcg_kmeans_update_f64(N, ptr(x), ptr(lab), Cn, ptr(pv), ptr(centers),
                                                         ptr(counts), ptr(status), ptr(ws), b, None),
                 [centers, counts])
    want = np.array([LOCS[LABELS == c].mean(0) if (LABELS == c).any() else prev[c] for c in range(Cn)])
    assert status.item() == 0
    np.testing.assert_array_equal(counts.cpu().numpy(), np.bincount(LABELS, minlength=Cn))
    np.testing.assert_allclose(centers.cpu().numpy(), want, rtol=F64)

    assert reported(lib, "gcg_cluster_stats_f64_workspace_bytes", N, Cn) == need
    means, sig, cor = (out((Cn, 2), torch.float64, cuda), out((Cn, 2), torch.float64, cuda),
                       out(Cn, torch.float64, cuda))
    cnt = out(Cn, torch.int32, cuda)
    run_contract(lib, cuda, "gcg_cluster_stats_f64", need,
                 lambda ws, b: lib.gcg_cluster_stats_f64(N, ptr(x), ptr(lab), Cn, 0, ptr(means), ptr(sig),
                                                         ptr(cor), ptr(cnt), ptr(status), ptr(ws), b, None),
                 [means, sig, cor, cnt])
    np.testing.assert_array_equal(cnt.cpu().numpy(), np.bincount(LABELS, minlength=Cn))
    for c in range(3):
        pts = LOCS[LABELS == c]
        np.testing.assert_allclose(means.cpu().numpy()[c], pts.mean(0), rtol=1e-12)
        np.testing.assert_allclose(sig.cpu().numpy()[c], pts.std(0, ddof=1), rtol=1e-10)
        np.testing.assert_allclose(cor.cpu().numpy()[c], np.corrcoef(pts.T)[0, 1], rtol=1e-9, atol=1e-12)
    assert sig.cpu().numpy()[3].tolist() == [1.0, 1.0] and cor.cpu().numpy()[3] == 0.0  # empty cluster


def test_kmeans_pp(native_lib, cuda):
    lib = native_lib
    N, Cn = len(LOCS), 3
    u = np.array([0.5, 0.25, 0.9])
    need = reported(lib, "gcg_kmeans_pp_f64_workspace_bytes", N)
    x, u_d = dev(LOCS, cuda), dev(u, cuda)
    idx, status = out(Cn, torch.int32, cuda), torch.zeros(1, dtype=torch.int32, device=cuda)
    run_contract(lib, cuda, "gcg_kmeans_pp_f64", need,
                 lambda ws, b: lib.gcg_kmeans_pp_f64(N, ptr(x), Cn, ptr(u_d), ptr(idx), ptr(status), ptr(ws),
                                                     b, None), [idx])
    chosen = [int(np.floor(u[0] * N))]
    for k in range(1, Cn):
        d2 = ((LOCS[:, None, :] - LOCS[chosen][None]) ** 2).sum(-1).min(1)
        s = np.cumsum(d2)
        target = u[k] * s[-1]
        assert np.abs(s - target).min() > 1e-6 * s[-1]  # no draw on a boundary: roundings cannot decide
        chosen.append(int(np.argmax(s > target)))
    assert status.item() == 0
    np.testing.assert_array_equal(idx.cpu().numpy(), chosen)


# ---- neighbours: 3 queries, 10 pairs, 20 words ---------------------------------------------------

@pytest.fixture(scope="module")
def words():
    rng = np.random.default_rng(3)
    E = rng.integers(-4, 5, (20, 5)).astype(np.float32)      # small integers: d2 is exact
    Q = rng.integers(-4, 5, (3, 5)).astype(np.float32)
    d2 = ((Q[:, None, :] - E[None]) ** 2).sum(-1).astype(np.float32)
    order = np.lexsort((np.broadcast_to(np.arange(20), d2.shape), d2), axis=1)  # by (d2, index)
    return E, Q, d2, order


def test_neighbour_ranks(native_lib, cuda, words):
    lib = native_lib
    E, Q, d2, order = words
    pair_ptr = np.array([0, 4, 4, 10], np.int32)             # the second query has no pair
    pair_word = np.array([3, 19, 0, 7, 5, 5, 12, 1, 18, 9], np.int32)
    P, V, D, nq = len(pair_word), len(E), E.shape[1], len(Q)
    need = reported(lib, "gcg_neighbour_ranks_f32_workspace_bytes", nq, P)
    e, q, pp, pw = dev(E, cuda), dev(Q, cuda), dev(pair_ptr, cuda), dev(pair_word, cuda)
    rank, status = out(P, torch.int32, cuda), torch.zeros(1, dtype=torch.int32, device=cuda)
    run_contract(lib, cuda, "gcg_neighbour_ranks_f32", need,
                 lambda ws, b: lib.gcg_neighbour_ranks_f32(V, D, ptr(e), D, nq, ptr(q), D, P, ptr(pp),
                                                           ptr(pw), ptr(rank), ptr(status), ptr(ws), b,
                                                           None), [rank])
    pair_q = np.repeat(np.arange(nq), np.diff(pair_ptr))
    want = [int(np.nonzero(order[qq] == w)[0][0]) for qq, w in zip(pair_q, pair_word)]
    assert status.item() == 0
    np.testing.assert_array_equal(rank.cpu().numpy(), want)


def test_kneighbors(native_lib, cuda, words):
    lib = native_lib
    E, Q, d2, order = words
    V, D, nq, k = len(E), E.shape[1], len(Q), 4
    need = reported(lib, "gcg_kneighbors_f32_workspace_bytes", V, nq, k)
    e, q = dev(E, cuda), dev(Q, cuda)
    dist, index = out((nq, k), torch.float32, cuda), out((nq, k), torch.int32, cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    run_contract(lib, cuda, "gcg_kneighbors_f32", need,
                 lambda ws, b: lib.gcg_kneighbors_f32(V, D, ptr(e), D, nq, ptr(q), D, k, ptr(dist), ptr(index),
                                                      ptr(status), ptr(ws), b, None), [dist, index])
    assert status.item() == 0
    np.testing.assert_array_equal(index.cpu().numpy(), order[:, :k])
    np.testing.assert_array_equal(dist.cpu().numpy(), np.take_along_axis(d2, order[:, :k], 1))


# ---- dense: M = 9 rows, N = 5 columns, K = 33 (two 32-deep chunks, the second with one live k) ----

MATH_F32, MATH_BF16X6 = 0, 1
DENSE_BAR = 2.0 ** -20  # of sum_k |a||b| per element: test_dense_gpu.py's bar for both maths


def padded(a, ld):
    """`a` in rows of ld floats (ld % 4 == 0, as the dwordx4 reads need), zeros behind."""
    p = np.zeros((a.shape[0], ld), np.float32)
    p[:, :a.shape[1]] = a
    return p


@pytest.fixture(scope="module")
def dense_case():
    rng = np.random.default_rng(11)
    M, N, K = 9, 5, 33
    A = rng.standard_normal((M, K)).astype(np.float32)
    W = rng.standard_normal((K, N)).astype(np.float32)
    prod = A.astype(np.float64) @ W.astype(np.float64)
    absprod = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64)
    return A, W, prod, absprod


def test_gemm_nt_bf16x6(native_lib, cuda, dense_case):
    lib = native_lib
    A, W, prod, absprod = dense_case
    (M, K), N = A.shape, W.shape[1]
    need = lib.gcg_gemm_nt_workspace(N, K, MATH_BF16X6)
    assert need == N * 2 * 192
    a, bt = dev(padded(A, 36), cuda), dev(padded(W.T, 36), cuda)
    c = out((M, 8), torch.float32, cuda)
    run_contract(lib, cuda, "gcg_gemm_nt", need,
                 lambda ws, b: lib.gcg_gemm_nt(M, N, K, ptr(a), 36, ptr(bt), 36, None, 0, ptr(c), 8,
                                               MATH_BF16X6, 0, ptr(ws), b, None), [c])
    err = np.abs(c.cpu().numpy()[:, :N].astype(np.float64) - prod)
    assert (err <= DENSE_BAR * absprod).all(), (err / absprod).max()


@pytest.mark.parametrize("math", [MATH_F32, MATH_BF16X6])
def test_gemm_tn(native_lib, cuda, math):
    lib = native_lib
    rng = np.random.default_rng(12)
    R, M, N = 40, 3, 5
    A = rng.standard_normal((R, M)).astype(np.float32)
    B = rng.standard_normal((R, N)).astype(np.float32)
    need = reported(lib, "gcg_gemm_tn_workspace_bytes", R, M, N, math, 0)
    a, b_ = dev(padded(A, 4), cuda), dev(padded(B, 8), cuda)
    c = out((M, 8), torch.float32, cuda)
    run_contract(lib, cuda, "gcg_gemm_tn", need,
                 lambda ws, b: lib.gcg_gemm_tn(R, M, N, ptr(a), 4, ptr(b_), 8, None, ptr(c), 8, math, 0,
                                               ptr(ws), b, None), [c])
    prod = A.T.astype(np.float64) @ B.astype(np.float64)
    absprod = np.abs(A.T).astype(np.float64) @ np.abs(B).astype(np.float64)
    err = np.abs(c.cpu().numpy()[:, :N].astype(np.float64) - prod)
    assert (err <= DENSE_BAR * absprod).all(), (err / absprod).max()


def test_project_softmax_xent_bf16x6(native_lib, cuda, dense_case):
    lib = native_lib
    A, W, logits, absprod = dense_case
    (M, K), N = A.shape, W.shape[1]
    labels = (np.arange(M) % N).astype(np.int32)
    scale = 0.25
    need = lib.gcg_project_softmax_xent_workspace(N, K, MATH_BF16X6)
    assert need == 1024 * 2 * 192
    a, w, y = dev(padded(A, 36), cuda), dev(padded(W, 8), cuda), dev(labels, cuda)
    o, loss, hit = (out((M, 8), torch.float32, cuda), out(M, torch.float32, cuda),
                    out(M, torch.float32, cuda))
    run_contract(lib, cuda, "gcg_project_softmax_xent", need,
                 lambda ws, b: lib.gcg_project_softmax_xent(
                     M, N, K, ptr(a), 36, ptr(w), 8, None, ptr(y), scale, None, ptr(o), 8, ptr(loss),
                     ptr(hit), None, MATH_BF16X6, 0, ptr(ws), b, None), [o, loss, hit])
    z = logits - logits.max(1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    onehot = np.eye(N)[labels]
    err = np.abs(o.cpu().numpy()[:, :N].astype(np.float64) - (p - onehot) * scale)
    assert (err <= DENSE_BAR * absprod).all(), (err / absprod).max()
    # The element bar above is the one test_dense_gpu.py uses. The two row outputs have none of
    # their own there; this one is derived here: the loss is a difference of two values (the
    # log-sum-exp and the label's logit) that each follow the logits, so twice the logits' bar,
    # taken over the row. The hits are checked only on logits further apart than that.
    row_bar = 2 * DENSE_BAR * absprod.max(1)
    want_loss = np.log(np.exp(z).sum(1)) - z[np.arange(M), labels]
    assert (np.abs(loss.cpu().numpy() - want_loss) <= row_bar).all()
    top2 = np.sort(logits, 1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0] > row_bar).all()
    np.testing.assert_array_equal(hit.cpu().numpy(), logits.argmax(1) == labels)
