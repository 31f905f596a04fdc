#!/usr/bin/env python
"""The reference's dialect-embedding evaluation (main.py:364-384, 417-440) end to end on
synthetic tweets, with the training and the evaluation on the GPU:

  host  synthetic users in R regions; every region has planted words (its "DARE" entries) and
        one vocabulary entry with the region's name that co-occurs with the region
  GPU   mlp.MLP with a hidden layer, trained to predict the region from the bag of words
        (--dropout: mlp.DropoutMLP, the reference's drop_out=True)
  GPU   get_embedding of the one-word-per-row matrix: a hidden-layer vector per word
  GPU   dialect.eval_embeddings: min-max + l1 scaling, the rank of every planted word among
        the neighbours of its region's entry, recall@k
  GPU   dialect.kneighbors: the nearest words of every region

The planted words of a region must come out of the region entry's neighbourhood well above
chance (k / V); the script asserts so.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_problem(n_users=3000, regions=6, planted=40, vocab_size=3000, seed=7):
    """(X [users, V] float32 CSR of binary word counts, region labels, vocab, lexicon dict)."""
    rng = np.random.default_rng(seed)
    names = [f"region{r}" for r in range(regions)]
    words = [[f"r{r}word{j}" for j in range(planted)] for r in range(regions)]
    n_common = vocab_size - regions * (planted + 1)
    if n_common < 1:
        raise ValueError("vocab_size leaves no room for common words")
    vocab = names + [w for ws in words for w in ws] + [f"common{j}" for j in range(n_common)]
    order = rng.permutation(len(vocab))  # no structure in the row order
    vocab = [vocab[i] for i in order]
    index = {w: i for i, w in enumerate(vocab)}
    region = rng.integers(0, regions, n_users)
    rows, cols = [], []
    for u in range(n_users):
        r = int(region[u])
        toks = list(rng.choice(words[r], 6, replace=False))
        toks += [f"common{j}" for j in rng.integers(0, n_common, 15)]
        if rng.random() < 0.7:
            toks.append(names[r])
        if rng.random() < 0.1:  # noise: a word of another region
            toks.append(words[int(rng.integers(0, regions))][int(rng.integers(0, planted))])
        for c in {index[t] for t in toks}:
            rows.append(u)
            cols.append(c)
    X = sps.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)),
                       shape=(n_users, len(vocab)), dtype=np.float32)
    return X, region.astype(np.int64), vocab, {names[r]: set(words[r]) for r in range(regions)}


def word_embeddings(X, region, vocab, hidden=64, epochs=8, batch=500, seed=7, as_tensor=True,
                    dropout=False):
    """Train the MLP on 85 % of the users and return (model, the hidden-layer vector of every
    vocabulary word): get_embedding of the V x V identity, one word per row. dropout: the
    trainer of main.py:425-427, MLP(..., drop_out=True, drop_out_coefs=[0.5, 0.5]) -- there with
    hidden_layer_size=2048 (--hidden 2048)."""
    from graphconvgeo_amd.mlp import MLP, DropoutMLP

    n_train = int(0.85 * X.shape[0])
    # the Glorot draws, the dropout seeds and the epoch shuffles come from numpy's stream
    np.random.seed(seed)
    if dropout:
        clf = DropoutMLP(n_epochs=epochs, batch_size=batch, hidden_layer_size=hidden,
                         regul_coefs=(1e-6, 1e-6), add_hidden=True, drop_out_coefs=[0.5, 0.5])
    else:
        clf = MLP(n_epochs=epochs, batch_size=batch, hidden_layer_size=hidden,
                  regul_coefs=(1e-6, 1e-6), add_hidden=True)
    clf.fit(X[:n_train], region[:n_train], X[n_train:], region[n_train:])
    one_word_per_row = sps.identity(len(vocab), dtype=np.float32, format="csr")
    return clf, clf.get_embedding(one_word_per_row, as_tensor=as_tensor), n_train


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=3000)
    ap.add_argument("--regions", type=int, default=6)
    ap.add_argument("--planted", type=int, default=40)
    ap.add_argument("--vocab", type=int, default=3000)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--nearest", type=int, default=8)
    ap.add_argument("--dropout", action="store_true",
                    help="train the embedding model with input dropout, as main.py:425-427 does "
                         "(mlp.DropoutMLP)")
    args = ap.parse_args()
    from graphconvgeo_amd import dialect

    X, region, vocab, gold = synthetic_problem(args.users, args.regions, args.planted, args.vocab)
    clf, embs, n_train = word_embeddings(X, region, vocab, args.hidden, args.epochs,
                                         dropout=args.dropout)
    acc = clf.accuracy(X[n_train:], region[n_train:])
    lexicon = dialect.DialectLexicon(gold)
    ks = (args.planted, 2 * args.planted, 5 * args.planted)
    res = dialect.eval_embeddings(vocab, embs, lexicon, ks=ks)
    scaled = dialect.scale_embeddings(embs)
    pairs = lexicon.pairs(vocab)
    dist, idx = dialect.kneighbors(scaled, pairs.rows, args.nearest)
    idx = idx.cpu().numpy()
    for d, row in zip(pairs.dialects, idx):
        print(f"{d}: " + " ".join(vocab[i] for i in row))
    chance = [100.0 * k / len(vocab) for k in ks]
    rec = {"users": args.users, "vocab": len(vocab), "dialects": len(res.dialects),
           "gold_words": int(res.totals.sum()), "dev_acc": round(acc, 4), "ks": list(res.ks),
           "micro_recall": [round(m, 2) for m in res.micro],
           "chance_recall": [round(c, 2) for c in chance]}
    print(json.dumps(rec))
    # every region's first neighbour is the region entry itself (rank 0, as in the reference)
    assert [vocab[i] for i in idx[:, 0]] == res.dialects
    assert res.micro[0] > 5 * chance[0], "planted words are not found above chance"
    return rec


if __name__ == "__main__":
    main()
