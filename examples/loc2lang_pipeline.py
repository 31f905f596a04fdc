#!/usr/bin/env python
"""The location-to-language model on synthetic data, end to end on the GPU:

  k-d-tree regions of the training coordinates (geo.KDTreeClustering)
  -> the regions' means, deviations and correlations (mdn.cluster_params) as the initial Gaussians
     (--init kmeans: the reference's get_cluster_centers instead, k-means into --ncomp clusters
     on the device, kmeans.get_cluster_centers)
  -> NNModel_loc2lang.fit on (coordinate, bag of words) pairs
  -> the word distribution over a coordinate grid -> the most local words (local_words).

Three places, each with words of its own and a few that everybody uses; the local words found
at the end should be the places' own.

--analyses adds the model's own analyses, which never form the n x V probabilities on the host:
the most local words from the device (NNModel_loc2lang.local_words), and per planted place the
top-ranked words of region_word_scores over the test rows nearest to it, with the recall of the
place's own words (region_recall).

--nomdn trains the baseline the Gaussian layer is compared against instead, a rectified dense
layer in place of the Gaussians (NNModel_loc2lang_nomdn): on the raw coordinates, or with --grid
on their grid representation (grid.grid_representation: l1-normalised sparse rows over a 0.5
degree grid of the US box, built on the device and never brought to the host).

    python examples/loc2lang_pipeline.py [--epochs 40] [--init kmeans --ncomp 6] [--analyses]
    python examples/loc2lang_pipeline.py --nomdn --grid [--analyses]
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from graphconvgeo_amd import geo, grid, kmeans, loc2lang, mdn  # noqa: E402

PLACES = np.array([[40.7, -74.0], [34.0, -118.2], [29.8, -95.4]])
OWN, COMMON = 10, 10  # words per place, words of everybody


def synthetic(n, rng):
    place = rng.integers(0, len(PLACES), size=n)
    X = (PLACES[place] + 0.7 * rng.standard_normal((n, 2))).astype(np.float32)
    V = OWN * len(PLACES) + COMMON
    Y = np.zeros((n, V), np.float32)
    for r in range(n):
        Y[r, OWN * place[r] + rng.choice(OWN, size=4, replace=False)] = 1
        Y[r, OWN * len(PLACES) + rng.choice(COMMON, size=4, replace=False)] = 1
    Y /= Y.sum(axis=1, keepdims=True)  # the l1-normalised bag of words
    return X, sps.csr_matrix(Y)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--init", choices=("kdtree", "kmeans"), default="kdtree",
                    help="where the initial Gaussians come from")
    ap.add_argument("--ncomp", type=int, default=6, help="components of --init kmeans")
    ap.add_argument("--analyses", action="store_true",
                    help="also print the device local words and the places' top-ranked words")
    ap.add_argument("--nomdn", action="store_true",
                    help="the no-MDN baseline: a rectified dense layer in place of the Gaussians")
    ap.add_argument("--grid", action="store_true",
                    help="with --nomdn: the coordinates as sparse rows over a 0.5 degree grid")
    args = ap.parse_args()
    if args.grid and not args.nomdn:
        ap.error("--grid is the input of the no-MDN baseline: give --nomdn too")
    rng = np.random.default_rng(0)
    np.random.seed(0)
    (Xtr, Ytr), (Xdev, Ydev), (Xte, Yte) = (synthetic(n, rng) for n in (1200, 300, 300))

    # what the model takes for a coordinate array: itself, or its rows over the grid
    rep = (lambda X: grid.grid_representation(X, device=args.device)) if args.grid else (lambda X: X)
    if args.nomdn:
        clf = loc2lang.NNModel_loc2lang_nomdn(n_epochs=args.epochs, batch_size=100, hid_size=32,
                                              n_gaus_comp=64, early_stopping_max_down=5,
                                              device=args.device)
        print("no-MDN baseline on", "the grid representation" if args.grid else "raw coordinates")
    elif args.init == "kmeans":
        C = args.ncomp
        mus, sigmas, corxy = kmeans.get_cluster_centers(Xtr, C, seed=0, device=args.device)
        print(f"k-means -> {C} Gaussians")
    else:
        tree = geo.KDTreeClustering(bucket_size=200).fit(Xtr, device=args.device)
        labels, C = tree.clusters.cpu().numpy(), tree.num_clusters
        mus, sigmas, corxy = mdn.cluster_params(Xtr, labels, C, raw=True)
        print(f"{C} regions -> {C} Gaussians")

    if not args.nomdn:
        clf = loc2lang.NNModel_loc2lang(n_epochs=args.epochs, batch_size=100, hid_size=32,
                                        n_gaus_comp=C, mus=mus, sigmas=sigmas, corxy=corxy,
                                        early_stopping_max_down=5, device=args.device)
    Xte_in = rep(Xte)
    ppl_test, ppl_dev = clf.fit(rep(Xtr), Ytr, rep(Xdev), Ydev, Xte_in, Yte)
    first, last = clf.history[0], clf.history[-1]
    print(f"dev loss {first['val_loss']:.3f} -> {last['val_loss']:.3f} in {len(clf.history)} epochs; "
          f"perplexity dev {ppl_dev:.2f}, test {ppl_test:.2f}")

    lat, lon = np.meshgrid(np.linspace(27, 43, 17), np.linspace(-121, -71, 26), indexing="ij")
    mesh = rep(np.stack([lat.ravel(), lon.ravel()], axis=1).astype(np.float32))
    words = loc2lang.local_words(clf.predict(mesh), k=12)
    local = int((words < OWN * len(PLACES)).sum())
    print("most local words:", words.tolist(), f"({local} of 12 belong to one place)")
    if args.analyses:
        print("most local words, on the device:", clf.local_words(mesh, k=12).tolist())
        nearest = np.abs(Xte[:, None, :] - PLACES[None]).sum(axis=-1).argmin(axis=1)
        group_rows = np.argsort(nearest, kind="stable")
        group_ptr = np.concatenate([[0], np.cumsum(np.bincount(nearest, minlength=len(PLACES)))])
        scores = clf.region_word_scores(Xte_in, group_ptr, group_rows)
        gold_ptr = OWN * np.arange(len(PLACES) + 1)
        rec = loc2lang.region_recall(scores, gold_ptr, np.arange(OWN * len(PLACES)),
                                     fractions=(0.1, 0.25))
        order = scores.argsort(dim=1, descending=True, stable=True)[:, :OWN].cpu().numpy()
        for g in range(len(PLACES)):
            print(f"place {g}: top-ranked words {order[g].tolist()}")
        print("recall of the places' own words at k =", rec.ks, "->",
              [round(r, 3) for r in rec.recall], "(oracle", [round(r, 3) for r in rec.oracle], ")")
    return 0 if local >= 10 else 1


if __name__ == "__main__":
    sys.exit(main())
