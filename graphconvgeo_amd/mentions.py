"""Mention graph: parsing on the host (the default, per BASELINE north_star) or on the device,
+ the O(sum deg^2) projection on the GPU.

`mention_incidences` restates DataLoader.get_graph's parsing (data.py:302-362): users are
numbered train, dev, test in table order; every @mention (regex of data.py:311, lowercased)
that names a user maps to that user's id, any other name gets the next new id in order of
first appearance; each (mentioned id, user id) pair is one incidence.

`project_mentions` runs the celebrity filter (data.py:364-370) and the projection of
efficient_collaboration_weighted_projected_graph2 (data.py:226-250) on the GPU
(gcg_project_mention_graph) and returns the user-user edge list; `mention_graph_operator`
chains it into the normalized operator H (gcg_normalize_adjacency_f32).

`mention_incidences_device` is `mention_incidences` with the per-mention work on the device
(csrc/tokenize.hip: the regex as a rule over bytes, the names' dictionary, each user's sorted
ids); the host keeps the join and encode of the texts and one lookup per distinct name. With
`mention_graph_operator(parser="device")` nothing but sizes leaves the device between the texts
and H.
"""
from __future__ import annotations

import ctypes as C
import re
import time

import numpy as np
import torch

from ._native import call

MENTION_PATTERN = re.compile(r"(?<=^|(?<=[^a-zA-Z0-9-_\.]))@([A-Za-z]+[A-Za-z0-9_]+)")


def mention_incidences(df_train, df_dev, df_test):
    """(n_users, n_nodes, a, b) of the bipartite mention graph, as data.py:302-362 builds it.

    The frames are indexed by (lowercased, sorted) user name with a `text` column, as
    DataLoader.load_data leaves them (data.py:273-299)."""
    return _incidences(*_users_and_texts(df_train, df_dev, df_test))


def _users_and_texts(df_train, df_dev, df_test):
    """(users, node_id, texts) in train, dev, test order; the duplicate check of data.py:305."""
    frames = (df_train, df_dev, df_test)
    users = [u for df in frames for u in df.index]
    node_id = {u: i for i, u in enumerate(users)}
    if len(node_id) != len(users):
        raise ValueError("duplicate target node")  # data.py:305
    return users, node_id, [t for df in frames for t in df["text"].tolist()]


def _incidences(users, node_id, texts):
    a, b = [], []
    for uid, text in enumerate(texts):
        ids = set()
        for m in MENTION_PATTERN.findall(text):
            m = m.lower()
            if m not in node_id:
                node_id[m] = len(node_id)
            ids.add(node_id[m])
        for i in sorted(ids):
            a.append(i)
            b.append(uid)
    return len(users), len(node_id), np.asarray(a, np.int32), np.asarray(b, np.int32)


def mention_incidences_device(df_train, df_dev, df_test, device="cuda", hash_bits=64,
                              timings=None):
    """mention_incidences with the per-mention work on the device: the same (n_users, n_nodes,
    a, b), `a` and `b` int32 device tensors equal to its arrays element for element.

    The host joins and encodes the texts (not lowercased: lowering changes what the regex
    matches) and looks each distinct name up once; the device finds the mentions in the UTF-8
    bytes (gcg_mention_mark), numbers the names in order of first appearance with A-Z folded
    (gcg_tokenize_terms_folded), which is the order in which the reference hands out the ids of
    names that are no user, replaces every mention by its node id (gcg_tokenize_remap) and
    sorts each user's distinct ids (gcg_tfidf_count). The dictionary goes by a hash verified
    byte by byte: where two names share one, mention_incidences does the whole call and
    `mention_incidences_device.fallbacks` counts it (`hash_bits` below 64 cuts the hash: for
    tests). The limits are tokenize_corpus_device's. `timings`, a dict, receives the seconds of
    the stages (prep_s, upload_s, kernels_s, terms_s), each closed by a synchronisation."""
    from . import _native
    from .tfidf import TOKENIZE_TILE_BYTES, _corpus_bytes, _ptr

    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the device parser runs on the GPU: device must be a CUDA (HIP) device")
    if not 1 <= int(hash_bits) <= 64:
        raise ValueError("hash_bits must be in 1 .. 64")

    def lap(name, t0):
        if timings is None:
            return t0
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        if t0 is not None:
            timings[name] = timings.get(name, 0.0) + t1 - t0
        return t1

    t = lap(None, None)
    users, node_id, texts = _users_and_texts(df_train, df_dev, df_test)
    n_users = len(users)
    buf, doc_off = _corpus_bytes(texts, lowercase=False)
    n = len(buf)

    def nothing(n_nodes=n_users):
        return (n_users, n_nodes, torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev))

    if n_users == 0 or n == 0:
        return nothing()
    if n > 1 << 33:
        raise ValueError("the texts have more than 2^33 bytes")
    t = lap("prep_s", t)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    n16 = (n + 15) // 16 * 16
    tiles = -(-n // TOKENIZE_TILE_BYTES)
    with torch.cuda.device(dev):
        text = torch.empty(n16, dtype=torch.uint8, device=dev)
        text[:n].copy_(torch.frombuffer(bytearray(buf), dtype=torch.uint8))
        off_dev = None if doc_off is None else torch.from_numpy(doc_off).to(dev)
        t = lap("upload_s", t)
        flags = torch.empty(n16, dtype=torch.uint8, device=dev)
        tile_base = torch.empty(tiles + 1, dtype=torch.int64, device=dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        ws, nbytes = _native.workspace("gcg_mention_mark_workspace_bytes", dev, n)
        call("gcg_mention_mark", n, _ptr(text), _ptr(flags), _ptr(tile_base), _ptr(totals),
             _ptr(ws), nbytes, stream)
        n_ment, n_nul = totals.tolist()
        if doc_off is None and n_nul != n_users - 1:
            raise RuntimeError(f"gcg_mention_mark: {n_nul} separators for {n_users} texts")
        if n_ment >= 2**31 - 1:
            raise ValueError("too many mentions for int32 indices")
        if n_ment == 0:
            return nothing()
        raw_ptr = torch.empty(n_users + 1, dtype=torch.int64, device=dev)
        tok_term = torch.empty(n_ment, dtype=torch.int32, device=dev)
        term_start = torch.empty(n_ment, dtype=torch.int64, device=dev)
        term_len = torch.empty(n_ment, dtype=torch.int32, device=dev)
        result = torch.zeros(2, dtype=torch.int64, device=dev)
        ws, nbytes = _native.workspace("gcg_tokenize_terms_workspace_bytes", dev, n_ment,
                                       int(hash_bits))
        call("gcg_tokenize_terms_folded", n, _ptr(text), _ptr(flags), _ptr(tile_base), n_ment,
             n_users, _ptr(off_dev), int(hash_bits), 1, _ptr(raw_ptr), _ptr(tok_term),
             _ptr(term_start), _ptr(term_len), _ptr(result), _ptr(ws), nbytes, stream)
        n_terms, collision = result.tolist()
        del ws, flags, tile_base, text
        if collision:
            # two names under one hash: exact by the host's parser for this call
            mention_incidences_device.fallbacks += 1
            texts = [x.decode("utf-8") if isinstance(x, bytes) else x for x in texts]
            _, n_nodes, a, b = _incidences(users, node_id, texts)
            return n_users, n_nodes, torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        starts = term_start[:n_terms].cpu().numpy()
        lens = term_len[:n_terms].cpu().numpy()
        t = lap("kernels_s", t)
        # per distinct name, never per mention: a user's id, or the next new one in the order
        # of first appearance, which is the order of the terms
        get = node_id.get
        action = np.fromiter((get(buf[s:e].decode("ascii").lower(), -1)
                              for s, e in zip(starts.tolist(), (starts + lens).tolist())),
                             np.int64, n_terms)
        new = action < 0
        n_nodes = n_users + int(new.sum())
        if n_nodes >= 2**31 - 1:
            raise ValueError("too many nodes for int32 indices")
        action[new] = n_users + np.arange(n_nodes - n_users)
        action_dev = torch.from_numpy(action.astype(np.int32)).to(dev)
        t = lap("terms_s", t)
        ids = torch.empty(n_ment, dtype=torch.int32, device=dev)
        ptr_dev = torch.empty(n_users + 1, dtype=torch.int64, device=dev)
        ws, nbytes = _native.workspace("gcg_tokenize_remap_workspace_bytes", dev, n_ment)
        call("gcg_tokenize_remap", n_ment, _ptr(tok_term), n_terms, _ptr(action_dev), n_users,
             _ptr(raw_ptr), _ptr(ids), _ptr(ptr_dev), _ptr(ws), nbytes, stream)
        # each user's distinct ids, ascending: the rows of the (user, node) count matrix
        indptr = torch.empty(n_users + 1, dtype=torch.int32, device=dev)
        a = torch.empty(n_ment, dtype=torch.int32, device=dev)
        counts = torch.empty(n_ment, dtype=torch.int32, device=dev)
        state = torch.zeros(2, dtype=torch.int64, device=dev)  # entries; status (int32)
        ws, nbytes = _native.workspace("gcg_tfidf_count_workspace_bytes", dev, n_users, n_ment,
                                       n_nodes)
        call("gcg_tfidf_count", n_users, n_nodes, n_ment, _ptr(ptr_dev), _ptr(ids), None,
             _ptr(indptr), _ptr(a), _ptr(counts), n_ment, _ptr(state), None, 0, _ptr(state, 8),
             _ptr(ws), nbytes, stream)
        nnz, status = state.tolist()
        if status & 0xffffffff:
            raise RuntimeError("gcg_tfidf_count: more incidences than mentions")
        b = torch.repeat_interleave(torch.arange(n_users, dtype=torch.int32, device=dev),
                                    (indptr[1:] - indptr[:-1]).long(), output_size=nnz)
        lap("kernels_s", t)
    return n_users, n_nodes, a[:nnz].clone(), b


mention_incidences_device.fallbacks = 0
PARSERS = ("host", "device")


def project_mentions(n_users: int, n_nodes: int, a, b, celebrity_threshold: int = 10,
                     device="cuda"):
    """User-user edges (u < v, sorted, unique) of the projected mention graph, on the GPU.
    `a`, `b`: arrays or lists, or tensors already on the device, which stay there."""
    from .graph import device_ids

    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the projection runs on the GPU: device must be a CUDA (HIP) device")
    at, bt = device_ids(a, dev), device_ids(b, dev)
    if at.shape != bt.shape:
        raise ValueError("a and b must have the same length")
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ne = C.c_int64()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    args = (int(n_users), int(n_nodes), int(at.numel()), C.c_void_p(at.data_ptr()),
            C.c_void_p(bt.data_ptr()), int(celebrity_threshold))
    with torch.cuda.device(dev):
        call("gcg_project_mention_graph", *args, None, None, 0, C.byref(ne),
             C.c_void_p(status.data_ptr()), stream)
        if int(status.item()) != 0:
            raise ValueError("incidence id out of range [0, n_nodes)")
        cap = max(ne.value, 1)
        u = torch.empty(cap, dtype=torch.int32, device=dev)
        v = torch.empty(cap, dtype=torch.int32, device=dev)
        call("gcg_project_mention_graph", *args, C.c_void_p(u.data_ptr()), C.c_void_p(v.data_ptr()),
             cap, C.byref(ne), C.c_void_p(status.data_ptr()), stream)
    return u[: ne.value], v[: ne.value]


def mention_graph_operator(df_train, df_dev, df_test, celebrity_threshold: int = 10,
                           device="cuda", parser="host"):
    """H = D^-1/2 (A+I) D^-1/2 of the projected mention graph, built on the GPU
    (tensormain.py:168-181 over DataLoader.get_graph's graph). parser="host" finds the mentions
    with mention_incidences; "device" with mention_incidences_device, and then the incidences,
    the projected edges and H never leave the device: only sizes are read back."""
    from .graph import normalize_edges_device

    if parser not in PARSERS:
        raise ValueError(f"parser must be 'host' or 'device', not {parser!r}")
    if parser == "device":
        n_users, n_nodes, a, b = mention_incidences_device(df_train, df_dev, df_test, device)
        u, v = project_mentions(n_users, n_nodes, a, b, celebrity_threshold, device)
        return normalize_edges_device(n_users, u, v, device)
    n_users, n_nodes, a, b = mention_incidences(df_train, df_dev, df_test)
    u, v = project_mentions(n_users, n_nodes, a, b, celebrity_threshold, device)
    return normalize_edges_device(n_users, u.cpu().numpy(), v.cpu().numpy(), device)
