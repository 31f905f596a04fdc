"""Plain NumPy float64 restatement of the k-means rules of csrc/kmeans.hip (include/gcg_spmm.h),
in the direct distance formula d = (x0 - c0) * (x0 - c0) + (x1 - c1) * (x1 - c1):

  assign      nearest centre by strict <, so the lowest index wins a tie; a NaN never wins
  update      the members' sum (math.fsum: exactly rounded) over the count; an empty cluster
              keeps its centre
  plusplus    k-means++, one trial per centre, as a pure function of the draws u
  lloyd       assignment then update, stopped after the first assignment that equals the one
              before (sklearn's strict convergence at tol = 0)
  stats       mdn.cluster_params' statistics with the device's fallbacks

It agrees with sklearn.cluster.KMeans(init=<array>, n_init=1, tol=0, algorithm="lloyd") label
for label where no distance tie is exact (tests/golden/make_kmeans_golden.py checks that before
it writes a fixture); on exact ties sklearn's expanded formula decides otherwise.
"""
from __future__ import annotations

import math

import numpy as np


def sq_dist(x, c):
    """Squared distances of the points x [N, 2] from one centre c [2]."""
    a = x[:, 0] - c[0]
    b = x[:, 1] - c[1]
    return a * a + b * b


def assign(x, centers):
    """(labels int32 [N], the minimal squared distance [N])."""
    x = np.asarray(x, np.float64)
    centers = np.asarray(centers, np.float64)
    best = np.full(x.shape[0], np.inf)
    lab = np.zeros(x.shape[0], np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(centers.shape[0]):
            d = sq_dist(x, centers[c])
            m = d < best
            best[m] = d[m]
            lab[m] = c
    return lab, best


def gap(x, centers):
    """The smallest relative gap between a point's best and second-best squared distance."""
    x = np.asarray(x, np.float64)
    d = np.stack([sq_dist(x, c) for c in np.asarray(centers, np.float64)], axis=1)
    if d.shape[1] < 2:
        return np.inf
    part = np.partition(d, 1, axis=1)
    return float(np.min((part[:, 1] - part[:, 0]) / np.maximum(part[:, 1], np.finfo(float).tiny)))


def update(x, labels, centers):
    """(new centres [C, 2], counts int32 [C]): exactly rounded sums over the count."""
    x = np.asarray(x, np.float64)
    new = np.array(centers, np.float64, copy=True)
    counts = np.bincount(labels, minlength=new.shape[0]).astype(np.int32)
    order = np.argsort(labels, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(counts)])
    for c in range(new.shape[0]):
        if counts[c]:
            m = x[order[ptr[c]:ptr[c + 1]]]
            new[c] = (math.fsum(m[:, 0]) / counts[c], math.fsum(m[:, 1]) / counts[c])
    return new, counts


def plusplus(x, n_clusters, u, return_margin=False):
    """int32 indices [C] of the seeds (and the smallest distance of a target u_k * S_{N-1} from
    a prefix-sum boundary, as a fraction of the total)."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    idx = np.zeros(n_clusters, np.int32)
    idx[0] = min(n - 1, int(math.floor(u[0] * n)))
    d2 = sq_dist(x, x[idx[0]])
    margin = np.inf
    for k in range(1, n_clusters):
        cs = np.cumsum(d2)
        total = cs[-1]
        if not total > 0:
            raise ValueError("fewer distinct points than clusters")
        target = u[k] * total
        j = int(np.searchsorted(cs, target, side="right"))      # first i with cs[i] > target
        j = min(j, int(np.flatnonzero(d2 > 0)[-1]))
        idx[k] = j
        margin = min(margin, float(np.min(np.abs(cs - target))) / total)
        d2 = np.minimum(d2, sq_dist(x, x[j]))
    return (idx, margin) if return_margin else idx


def lloyd(x, init, max_iter=300, return_gap=False):
    """dict(centers, labels, counts, inertia, n_iter): sklearn's loop at tol = 0. labels are the
    assignment to the returned centres."""
    x = np.asarray(x, np.float64)
    centers = np.array(init, np.float64, copy=True)
    prev = None
    counts = None
    n_iter = 0
    g = np.inf
    converged = False
    for it in range(1, max_iter + 1):
        labels, best = assign(x, centers)
        if return_gap:
            g = min(g, gap(x, centers))
        n_iter = it
        if prev is not None and np.array_equal(labels, prev):
            converged = True        # update(labels) is the centres these labels came from
            break
        centers, counts = update(x, labels, centers)
        prev = labels
    if not converged:
        labels, best = assign(x, centers)
        if return_gap:
            g = min(g, gap(x, centers))
    out = dict(centers=centers, labels=labels, counts=counts, inertia=math.fsum(best), n_iter=n_iter)
    if return_gap:
        out["gap"] = g
    return out


def raw_sigma(s):
    with np.errstate(divide="ignore"):
        return s + np.log1p(-np.exp(-s))


def raw_corxy(c):
    return c / (1.0 - np.abs(c))


def stats(x, labels, n_cluster, centers=None, raw=True):
    """(means [C, 2], sigmas [C, 2], corxys [C], counts): np.cov's ddof-1 statistics; (1, 1, 0)
    for a single member, a zero variance, a NaN or an empty cluster (whose mean is centers[c],
    NaN without centers)."""
    x = np.asarray(x, np.float64)
    means = np.full((n_cluster, 2), np.nan) if centers is None else np.array(centers, np.float64)
    sig = np.ones((n_cluster, 2))
    cor = np.zeros(n_cluster)
    counts = np.bincount(labels, minlength=n_cluster).astype(np.int32)
    for c in range(n_cluster):
        m = x[labels == c]
        if m.shape[0] == 0:
            continue
        means[c] = m.mean(axis=0)
        if m.shape[0] > 1:
            cov = np.cov(m, rowvar=False)
            with np.errstate(invalid="ignore", divide="ignore"):
                s = np.sqrt(np.array([cov[0, 0], cov[1, 1]]))
                r = cov[0, 1] / (s[0] * s[1])
            if s[0] > 0 and s[1] > 0 and not np.isnan(r):
                sig[c], cor[c] = s, r
    if raw:
        sig, cor = raw_sigma(sig), raw_corxy(cor)
    return means, sig, cor, counts


def blobs(n, k, seed, spread=1.0):
    """n points of k Gaussian blobs over the map, rounded through float32."""
    rng = np.random.default_rng(seed)
    mid = np.column_stack([rng.uniform(-60, 70, k), rng.uniform(-180, 180, k)])
    x = mid[rng.integers(0, k, n)] + spread * rng.standard_normal((n, 2))
    return x.astype(np.float32)


def grid_points(n=8000, seed=5, step=0.5):
    """n points snapped to a `step` degree grid (float64): exact distance ties, exact sums."""
    rng = np.random.default_rng(seed)
    mid = np.column_stack([rng.uniform(-40, 40, 12), rng.uniform(-100, 100, 12)])
    x = mid[rng.integers(0, 12, n)] + 3.5 * rng.standard_normal((n, 2))
    return np.round(x / step) * step
