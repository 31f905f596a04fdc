"""k-means initialisation of the Gaussian components on the GPU (csrc/kmeans.hip).

  get_cluster_centers  the reference's function (lang2loc.py:473-478,
                       lang2loc_mdnshared.py:127-185, loc2lang.py:326-371) in one call: the
                       (mus, sigmas, corxys) the three mixture models take
  KMeans               full Lloyd k-means, k-means++ seeded, float64, deterministic
  kmeans_plusplus      the seeding: plain k-means++, one trial per centre, a pure function of
                       the uniform draws u
  kmeans_assign        nearest centre of every point (+ squared distance, inertia, "changed")
  kmeans_update        the members' mean per cluster and the counts
  cluster_stats        mdn.cluster_params on the device

The reference runs sklearn's MiniBatchKMeans(n_clusters=ncomp, batch_size=1000) without a
random_state; this is full k-means instead (the variant the reference keeps commented out as
too slow on its host), so the centres differ from any one run of the reference and are the
same on every run here. Not built: the mini-batch update rule, the greedy multi-trial
k-means++ and the relocation of empty clusters (an empty cluster keeps its centre). The metric
is Euclidean on raw degrees, as the reference's.

Coordinates are (N, 2) [latitude, longitude], numpy arrays or tensors; float32 is widened to
float64 on the device. Labels, indices and counts are int32 device tensors.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from ._native import call, workspace as _workspace
from .geo import _coords, _ptr, _stream

Assignment = namedtuple("Assignment", "labels distances inertia changed")

_PP_ERRORS = {1: "fewer distinct points than clusters", 2: "locs holds a non-finite coordinate",
              3: "u must lie in [0, 1)"}


def _n_points(locs, name="locs") -> int:
    """The number of rows of `locs` after the checks that need no device: the shape, and for
    host data the finiteness (device data is checked by the kernels)."""
    a = locs if torch.is_tensor(locs) else np.asarray(locs)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{name} must have shape (N, 2) [lat, lon], got {tuple(a.shape)}")
    if not torch.is_tensor(a) and a.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be numeric, got {a.dtype}")
    if not (torch.is_tensor(a) and a.is_cuda):
        finite = torch.isfinite(a).all() if torch.is_tensor(a) else np.isfinite(a).all()
        if not bool(finite):
            raise ValueError(f"{name} holds a non-finite coordinate")
    return int(a.shape[0])


def _labels(labels, n, dev, name="labels"):
    lab = torch.as_tensor(labels).to(dev)
    if lab.dim() != 1 or lab.shape[0] != n:
        raise ValueError(f"{name} must have shape ({n},), got {tuple(lab.shape)}")
    if lab.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name} must be int32 or int64, got {lab.dtype}")
    return lab.to(torch.int32).contiguous()


def _n_clusters(n_clusters, n):
    if int(n_clusters) != n_clusters:
        raise ValueError(f"n_clusters must be an integer, got {n_clusters}")
    c = int(n_clusters)
    if not 1 <= c <= n:
        raise ValueError(f"need 1 <= n_clusters <= the number of points, got {c} for {n} points")
    return c


def _assign(x, centers, prev, want_distances=True):
    """The ABI call without a readback: (labels, dist2, inertia[1], changed[1], status[1])."""
    dev, n = x.device, x.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.float64, device=dev) if want_distances else None
    inertia = torch.empty(1, dtype=torch.float64, device=dev)
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    ws, nbytes = _workspace("gcg_kmeans_assign_f64_workspace_bytes", dev, n)
    call("gcg_kmeans_assign_f64", n, _ptr(x), centers.shape[0], _ptr(centers), _ptr(prev),
         _ptr(labels), _ptr(dist), _ptr(inertia), C.c_void_p(flags.data_ptr()),
         C.c_void_p(flags.data_ptr() + 4), _ptr(ws), nbytes, _stream(dev))
    return labels, dist, inertia, flags[0:1], flags[1:2]


def _update(x, labels, centers):
    """The ABI call without a readback: (centers, counts, status[1])."""
    dev, n, c = x.device, x.shape[0], centers.shape[0]
    new = torch.empty_like(centers)
    counts = torch.empty(c, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, nbytes = _workspace("gcg_kmeans_update_f64_workspace_bytes", dev, n, c)
    call("gcg_kmeans_update_f64", n, _ptr(x), _ptr(labels), c, _ptr(centers), _ptr(new),
         _ptr(counts), _ptr(status), _ptr(ws), nbytes, _stream(dev))
    return new, counts, status


def kmeans_assign(locs, centers, prev_labels=None, device=None) -> Assignment:
    """Assignment(labels, distances, inertia, changed): the index of the nearest centre of every
    point (the lowest on a tie), its squared distance, their sum (0-dim float64 tensor) and,
    with prev_labels, whether some label differs from it (bool; None without). Everything but
    `changed` stays on the device."""
    if _n_points(locs) > 0 and _n_points(centers, "centers") == 0:
        raise ValueError("no centre to choose from")
    x = _coords(locs, device)
    cen = _coords(centers, x.device, "centers")
    n = x.shape[0]
    prev = None if prev_labels is None else _labels(prev_labels, n, x.device, "prev_labels")
    with torch.cuda.device(x.device):
        labels, dist, inertia, changed, status = _assign(x, cen, prev)
    changed, status = torch.cat([changed, status]).tolist()
    if status != 0:
        raise ValueError("locs holds a non-finite coordinate")
    return Assignment(labels, dist, inertia[0], None if prev is None else bool(changed))


def kmeans_update(locs, labels, centers, device=None):
    """(centers [C, 2] float64, counts [C] int32): the mean of every cluster's members; an empty
    cluster keeps its row of `centers` and gets count 0. Bitwise the same on every call."""
    if _n_points(locs) > 0 and _n_points(centers, "centers") == 0:
        raise ValueError("points but no cluster")
    x = _coords(locs, device)
    cen = _coords(centers, x.device, "centers")
    n = x.shape[0]
    lab = _labels(labels, n, x.device)
    with torch.cuda.device(x.device):
        new, counts, status = _update(x, lab, cen)
    if int(status.item()) != 0:
        raise ValueError(f"a label outside [0, {cen.shape[0]})")
    return new, counts


def _draws(n_clusters, u, seed):
    if u is None:
        return np.random.default_rng(seed).random(n_clusters)
    u = np.ascontiguousarray(u, dtype=np.float64)
    if u.shape != (n_clusters,):
        raise ValueError(f"u must have shape ({n_clusters},), got {u.shape}")
    if not np.all((u >= 0) & (u < 1)):
        raise ValueError("u must lie in [0, 1)")
    return u


def _plusplus(x, c, u):
    """The ABI call without a readback: (indices, status[1])."""
    dev, n = x.device, x.shape[0]
    idx = torch.empty(c, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ud = torch.from_numpy(u).pin_memory().to(dev, non_blocking=True)  # no host wait before the rounds
    ws, nbytes = _workspace("gcg_kmeans_pp_f64_workspace_bytes", dev, n)
    call("gcg_kmeans_pp_f64", n, _ptr(x), c, _ptr(ud), _ptr(idx), _ptr(status), _ptr(ws), nbytes,
         _stream(dev))
    return idx, status


def kmeans_plusplus(locs, n_clusters, u=None, seed=None, device=None) -> torch.Tensor:
    """int32 (n_clusters,) indices of the k-means++ seeds among `locs`. u: the uniform draws in
    [0, 1), one per centre (default np.random.default_rng(seed).random(n_clusters)); the result
    is a pure function of (locs, u). ValueError when locs has fewer distinct points than
    n_clusters. One readback, of the status."""
    c = _n_clusters(n_clusters, _n_points(locs))
    u = _draws(c, u, seed)
    x = _coords(locs, device)
    with torch.cuda.device(x.device):
        idx, status = _plusplus(x, c, u)
    st = int(status.item())
    if st != 0:
        raise ValueError(_PP_ERRORS[st])
    return idx


class KMeans:
    """Lloyd k-means on the GPU: assignment then update, stopped after the first assignment that
    equals the one before (sklearn's strict convergence at tol = 0) or after max_iter.
    init: "k-means++" (seeded by `seed`) or a (C, 2) array of centres.

    After fit: cluster_centers_ ((C, 2) float64, device), labels_ (int32, device: the assignment
    to cluster_centers_), counts_ (int32, device), inertia_ (float), n_iter_ (assignments made
    in the loop, as sklearn counts) and readbacks_ (host copies of the fit: one 4-byte flag per
    iteration, the seeding's status, the final inertia)."""

    def __init__(self, n_clusters, init="k-means++", max_iter: int = 300, seed=None):
        self.n_clusters = n_clusters
        self.init = init
        self.max_iter = max_iter
        self.seed = seed

    def fit(self, locs, device=None):
        c = _n_clusters(self.n_clusters, _n_points(locs))
        if int(self.max_iter) != self.max_iter or int(self.max_iter) < 1:
            raise ValueError(f"max_iter must be an integer >= 1, got {self.max_iter}")
        if isinstance(self.init, str):
            if self.init != "k-means++":
                raise ValueError(f"init must be 'k-means++' or a (C, 2) array, got {self.init!r}")
        elif _n_points(self.init, "init") != c:
            raise ValueError(f"init must have shape ({c}, 2)")
        x = _coords(locs, device)
        dev = x.device
        readbacks = 0
        with torch.cuda.device(dev):
            if isinstance(self.init, str):
                idx, status = _plusplus(x, c, _draws(c, None, self.seed))
                readbacks += 1
                st = int(status.item())
                if st != 0:
                    raise ValueError(_PP_ERRORS[st])
                centers = x[idx.long()]
            else:
                centers = _coords(self.init, dev, "init").clone()
            prev = counts = None
            converged = False
            for it in range(1, int(self.max_iter) + 1):
                labels, _, inertia, changed, status = _assign(x, centers, prev, False)
                # the iteration's one readback: the input check first, then "some label changed"
                flag = int((status if prev is None else changed).item())
                readbacks += 1
                if prev is None and flag != 0:
                    raise ValueError("locs holds a non-finite coordinate")
                if prev is not None and flag == 0:
                    converged = True  # update(labels) is bitwise the centres they came from
                    break
                centers, counts, _ = _update(x, labels, centers)
                prev = labels
            if not converged:
                labels, _, inertia, _, _ = _assign(x, centers, None, False)
            self.inertia_ = float(inertia.item())
            readbacks += 1
        self.cluster_centers_ = centers
        self.labels_ = labels
        self.counts_ = counts
        self.n_iter_ = it
        self.readbacks_ = readbacks
        return self


def cluster_stats(locs, labels, n_cluster, centers=None, raw: bool = True, device=None):
    """mdn.cluster_params on the device: (mus (C, 2), sigmas (C, 2), corxys (C,)) float64 device
    tensors of the clusters 0 .. n_cluster - 1 of `labels` -- the mean, the ddof-1 standard
    deviations and the correlation; (1, 1, 0) for a single member, a zero variance, a NaN or an
    empty cluster. With raw, sigmas and corxys go through the inverse softplus and the inverse
    softsign. An empty cluster's mean is its row of `centers` (NaN without centers)."""
    n, c = _n_points(locs), int(n_cluster)
    if c < 0 or (n > 0 and c == 0):
        raise ValueError(f"n_cluster must be >= 1 for {n} points, got {n_cluster}")
    if centers is not None and _n_points(centers, "centers") != c:
        raise ValueError(f"centers must have shape ({c}, 2)")
    x = _coords(locs, device)
    dev = x.device
    lab = _labels(labels, n, dev)
    if centers is None:
        means = torch.full((c, 2), float("nan"), dtype=torch.float64, device=dev)
    else:
        means = _coords(centers, dev, "centers").clone()
    sigmas = torch.empty((c, 2), dtype=torch.float64, device=dev)
    corxys = torch.empty(c, dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws, nbytes = _workspace("gcg_cluster_stats_f64_workspace_bytes", dev, n, c)
        call("gcg_cluster_stats_f64", n, _ptr(x), _ptr(lab), c, int(bool(raw)), _ptr(means),
             _ptr(sigmas), _ptr(corxys), None, _ptr(status), _ptr(ws), nbytes, _stream(dev))
    if int(status.item()) != 0:
        raise ValueError(f"a label outside [0, {c})")
    return means, sigmas, corxys


def get_cluster_centers(latlon, n_cluster, raw: bool = True, seed=None, max_iter: int = 300,
                        device=None):
    """The reference's get_cluster_centers: k-means of the training (lat, lon) into n_cluster
    clusters, then (mus [C, 2], sigmas [C, 2], corxys [C]) as float32 NumPy arrays, ready for
    the `mus=, sigmas=, corxy=` arguments of NNModel_lang2loc, NNModel_lang2locshared and
    NNModel_loc2lang. mus are the k-means centres; sigmas and corxys are the raw parameters
    (see cluster_stats) unless raw=False."""
    km = KMeans(n_cluster, max_iter=max_iter, seed=seed).fit(latlon, device)
    x = _coords(latlon, km.labels_.device)
    _, sigmas, corxys = cluster_stats(x, km.labels_, km.cluster_centers_.shape[0],
                                      centers=km.cluster_centers_, raw=raw)
    return (km.cluster_centers_.cpu().numpy().astype(np.float32),
            sigmas.cpu().numpy().astype(np.float32), corxys.cpu().numpy().astype(np.float32))
