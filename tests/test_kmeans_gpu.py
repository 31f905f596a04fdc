"""The k-means initialisation on the GPU (graphconvgeo_amd.kmeans, csrc/kmeans.hip) against the
NumPy restatement (tests/kmeans_reference.py), the committed sklearn fixtures
(tests/golden/kmeans_*.npz) and the host mdn.cluster_params.

Bitwise where the rules make it so: the labels and squared distances of an assignment (one
rounding per operation, strict <), everything on the 0.5-degree grid data (its sums are exact
in any order), and any two runs of the same call. Elsewhere the bars are a-priori: a sum of n
float64 terms in any order is within (n - 1) 2^-53 sum|x| of the exact one."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import kmeans_reference as ref
import loc2lang_reference as R
from graphconvgeo_amd import _native, geo
from graphconvgeo_amd import kmeans as K
from graphconvgeo_amd import loc2lang as L
from graphconvgeo_amd import mdn as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("small", "medium", "large")
EPS = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def fixture(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"kmeans_{name}.npz"))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def grid_case():
    """8000 points on the 0.5-degree grid, C = 48, and the restatement's fit of them."""
    x = ref.grid_points()
    u = np.random.default_rng(8).random(48)
    seeds = ref.plusplus(x, 48, u)
    return x, u, seeds, ref.lloyd(x, x[seeds])


def host(t):
    return t.cpu().numpy()


def points(n, seed=0):
    rng = np.random.default_rng(seed)
    return np.column_stack([rng.uniform(-60, 70, n), rng.uniform(-180, 180, n)])


# -- 1. assignment -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_assign_is_bitwise_the_restatement(cuda, n):
    T = _native.load().gcg_kmeans_centre_tile()
    x = points(n, seed=n)
    for c in (1, 2, T - 1, T, T + 1, 2 * T + 3):
        centers = points(c, seed=1000 + c)
        want_lab, want_d = ref.assign(x, centers)
        got = K.kmeans_assign(x, centers, device=cuda)
        assert got.labels.dtype == torch.int32 and got.changed is None
        assert np.array_equal(host(got.labels), want_lab), (n, c)
        assert np.array_equal(host(got.distances), want_d), (n, c)
        exact = math.fsum(want_d)
        assert abs(float(got.inertia) - exact) <= n * EPS * exact


def test_assign_ties_duplicates_and_nan_centres(cuda):
    x, _, _, _ = grid_case()
    # centres on the grid around its most frequent point: many points are exactly as far from
    # two of them
    uniq, freq = np.unique(x, axis=0, return_counts=True)
    p = uniq[np.argmax(freq)]
    centers = np.array([p, p + [1, 0], p + [0, 1], p + [1, 0], p + [-3, 2.5], p])
    d = np.stack([ref.sq_dist(x, c) for c in centers[[0, 1, 2, 4]]], axis=1)
    srt = np.sort(d, axis=1)
    assert (srt[:, 0] == srt[:, 1]).sum() >= 20  # the case holds exact ties
    want_lab, want_d = ref.assign(x, centers)
    got = K.kmeans_assign(x, centers, device=cuda)
    assert np.array_equal(host(got.labels), want_lab) and np.array_equal(host(got.distances), want_d)
    assert not np.isin(host(got.labels), [3, 5]).any()  # a duplicate never beats the first copy
    withnan = torch.as_tensor(np.vstack([[[np.nan, 0.0]], centers]), device=cuda)
    got = K.kmeans_assign(x, withnan, device=cuda)
    assert np.array_equal(host(got.labels), want_lab + 1)  # a NaN centre is never the nearest


def test_assign_edges(cuda):
    centers = points(5, seed=3)
    empty = K.kmeans_assign(np.zeros((0, 2)), centers, device=cuda)
    assert empty.labels.shape == (0,) and float(empty.inertia) == 0.0
    x32 = points(700, seed=4).astype(np.float32)
    a, b = K.kmeans_assign(x32, centers, device=cuda), K.kmeans_assign(x32.astype(np.float64), centers, device=cuda)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.distances, b.distances)
    assert torch.equal(a.inertia, b.inertia)
    same = K.kmeans_assign(x32, centers, prev_labels=a.labels, device=cuda)
    assert same.changed is False
    other = a.labels.clone()
    other[699] = (other[699] + 1) % 5
    assert K.kmeans_assign(x32, centers, prev_labels=other, device=cuda).changed is True
    with pytest.raises(ValueError):
        K.kmeans_assign(torch.tensor([[0.0, float("nan")]], device=cuda), centers)


def test_assign_optional_outputs_are_null_in_turn(cuda):
    n, c = 1500, 7
    x = torch.as_tensor(points(n, seed=5), device=cuda)
    centers = torch.as_tensor(points(c, seed=6), device=cuda)
    full = K.kmeans_assign(x, centers, prev_labels=torch.zeros(n, dtype=torch.int32, device=cuda))
    nbytes = C.c_size_t()
    _native.call("gcg_kmeans_assign_f64_workspace_bytes", n, C.byref(nbytes))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=cuda)
    prev = torch.zeros(n, dtype=torch.int32, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for drop in ("prev", "dist", "inertia", "changed", "all"):
        labels = torch.full((n,), -1, dtype=torch.int32, device=cuda)
        dist = torch.full((n,), -1.0, dtype=torch.float64, device=cuda)
        inertia = torch.full((1,), -1.0, dtype=torch.float64, device=cuda)
        changed = torch.full((1,), -1, dtype=torch.int32, device=cuda)
        status = torch.full((1,), -1, dtype=torch.int32, device=cuda)
        off = lambda name: drop in (name, "all")  # noqa: E731
        no_ws = off("inertia")
        _native.call("gcg_kmeans_assign_f64", n, p(x), c, p(centers),
                     None if off("prev") else p(prev), p(labels), None if off("dist") else p(dist),
                     None if off("inertia") else p(inertia), None if off("changed") else p(changed),
                     p(status), None if no_ws else p(ws), 0 if no_ws else nbytes.value, stream)
        assert torch.equal(labels, full.labels) and int(status) == 0
        assert float(dist[0]) == -1.0 if off("dist") else torch.equal(dist, full.distances)
        assert float(inertia) == -1.0 if off("inertia") else float(inertia) == float(full.inertia)
        if not off("changed"):
            assert int(changed) == (0 if off("prev") else 1)
    with pytest.raises(_native.NativeError):  # the inertia needs the workspace
        _native.call("gcg_kmeans_assign_f64", n, p(x), c, p(centers), None, p(labels), None,
                     p(inertia), None, p(status), None, 0, stream)


# -- 2. update -----------------------------------------------------------------------------------
def test_update_counts_means_and_empty_clusters(cuda):
    n, c = 20000, 9
    x = points(n, seed=7)
    rng = np.random.default_rng(8)
    labels = rng.choice([0, 1, 2, 4, 5, 6, 8], size=n).astype(np.int32)  # 3 and 7 stay empty
    labels[:3] = [8, 0, 8]
    prev = points(c, seed=9)
    new, counts = K.kmeans_update(x, labels, prev, device=cuda)
    new, counts = host(new), host(counts)
    assert np.array_equal(counts, np.bincount(labels, minlength=c))
    assert np.array_equal(new[[3, 7]], prev[[3, 7]]) and counts[3] == counts[7] == 0
    for k in np.flatnonzero(counts):
        m = x[labels == k]
        for d in (0, 1):
            exact = math.fsum(m[:, d]) / len(m)
            assert abs(new[k, d] - exact) <= (len(m) - 1) * EPS * np.abs(m[:, d]).max(), (k, d)
    # one cluster owns every point; int64 labels; a label out of range
    one, cnt = K.kmeans_update(x, np.full(n, 2, np.int64), prev, device=cuda)
    assert host(cnt).tolist() == [0, 0, n] + [0] * 6
    assert abs(host(one)[2, 0] - math.fsum(x[:, 0]) / n) <= (n - 1) * EPS * np.abs(x[:, 0]).max()
    assert np.array_equal(np.delete(host(one), 2, axis=0), np.delete(prev, 2, axis=0))
    with pytest.raises(ValueError):
        K.kmeans_update(x, np.full(n, c, np.int32), prev, device=cuda)


def test_update_is_bitwise_reproducible(cuda):
    n, c = 30011, 37
    x = torch.as_tensor(points(n, seed=10), device=cuda)
    labels = torch.as_tensor(np.random.default_rng(11).integers(0, c, n).astype(np.int32), device=cuda)
    prev = torch.zeros((c, 2), dtype=torch.float64, device=cuda)
    a = K.kmeans_update(x, labels, prev)
    b = K.kmeans_update(x, labels, prev)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        s = K.kmeans_update(x, labels, prev)
    side.synchronize()
    for other in (b, s):
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])


def test_update_on_grid_data_is_bitwise(cuda):
    x, _, _, fit = grid_case()
    labels, _ = ref.assign(x, fit["centers"])
    want, counts = ref.update(x, labels, fit["centers"])
    got, cnt = K.kmeans_update(x, labels, fit["centers"], device=cuda)
    assert np.array_equal(host(got), want) and np.array_equal(host(cnt), counts)


# -- 3. seeding ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_plusplus_equals_the_restatement_on_the_fixtures(cuda, name):
    g = fixture(name)
    got = K.kmeans_plusplus(g["points"], len(g["u"]), u=g["u"], device=cuda)
    assert got.dtype == torch.int32 and np.array_equal(host(got), g["seeds"])
    seeded = K.kmeans_plusplus(g["points"], len(g["u"]), seed=int(g["u_seed"]), device=cuda)
    assert torch.equal(seeded, got)  # the default draws are default_rng(seed).random(C)


def check_picks(x, u, idx):
    """Every pick is valid given the device's own earlier picks."""
    n = len(x)
    assert idx[0] == min(n - 1, int(math.floor(u[0] * n)))
    d2 = ref.sq_dist(x, x[idx[0]])
    for k in range(1, len(idx)):
        j = int(idx[k])
        cs = np.cumsum(d2)
        total = cs[-1]
        eps = n * 2.0 ** -52 * total
        assert d2[j] > 0, k
        below = cs[j - 1] if j > 0 else 0.0
        last = int(np.flatnonzero(d2 > 0)[-1])
        assert below - eps <= u[k] * total, k
        assert u[k] * total <= cs[j] + eps or j == last, k
        d2 = np.minimum(d2, ref.sq_dist(x, x[j]))


def test_plusplus_picks_are_valid_on_arbitrary_data(cuda):
    x = points(5001, seed=12)          # 3 workgroups of 2048 points, a ragged tail
    x[100:160] = x[7]                  # duplicated points
    x[4000:4100] = x[4500]
    u = np.random.default_rng(13).random(40)
    idx = host(K.kmeans_plusplus(x, 40, u=u, device=cuda))
    check_picks(x, u, idx)
    assert len({tuple(x[i]) for i in idx}) == 40  # no location twice
    assert np.array_equal(idx, host(K.kmeans_plusplus(x, 40, u=u, device=cuda)))


def test_plusplus_edge_draws_and_too_few_points(cuda):
    x = points(3000, seed=14)
    below_one = np.nextafter(1.0, 0.0)
    for u in (np.zeros(6), np.full(6, below_one), np.array([0.0, below_one] * 3)):
        idx = host(K.kmeans_plusplus(x, 6, u=u, device=cuda))
        check_picks(x, u, idx)
        assert len(set(idx.tolist())) == 6
    assert host(K.kmeans_plusplus(x, 1, u=[below_one], device=cuda)).tolist() == [2999]
    few = np.repeat(points(5, seed=15), 40, axis=0)  # 200 points, 5 distinct
    idx = host(K.kmeans_plusplus(few, 5, seed=1, device=cuda))
    assert len({tuple(few[i]) for i in idx}) == 5
    with pytest.raises(ValueError, match="distinct"):
        K.kmeans_plusplus(few, 6, seed=1, device=cuda)
    with pytest.raises(ValueError, match="distinct"):
        K.KMeans(6, seed=1).fit(few, device=cuda)
    with pytest.raises(ValueError, match="non-finite"):
        K.kmeans_plusplus(torch.tensor([[0.0, 1.0], [float("inf"), 0.0]], device=cuda), 2, seed=0)


# -- 4. Lloyd ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_fit_reproduces_the_sklearn_fixture(cuda, name):
    g = fixture(name)
    km = K.KMeans(len(g["u"]), seed=int(g["u_seed"])).fit(g["points"], device=cuda)
    assert np.array_equal(host(km.labels_), g["labels"]) and km.n_iter_ == int(g["n_iter"])
    counts = host(km.counts_)
    assert np.array_equal(counts, np.bincount(g["labels"]))
    err = np.abs(host(km.cluster_centers_) - g["centers"]).max()
    rel = abs(km.inertia_ - float(g["inertia"])) / float(g["inertia"])
    print(name, "centres within", err, "inertia rel", rel, "n_iter", km.n_iter_, "readbacks", km.readbacks_)
    assert err <= counts.max() * EPS * 180
    assert rel <= 1e-12
    assert km.readbacks_ <= km.n_iter_ + 2
    fresh = K.kmeans_assign(g["points"], km.cluster_centers_, device=cuda)
    assert torch.equal(fresh.labels, km.labels_) and float(fresh.inertia) == km.inertia_
    again = K.KMeans(len(g["u"]), seed=int(g["u_seed"])).fit(g["points"], device=cuda)
    assert torch.equal(again.cluster_centers_, km.cluster_centers_)
    assert torch.equal(again.labels_, km.labels_) and again.inertia_ == km.inertia_


def test_fit_on_grid_data_is_bitwise_the_restatement(cuda):
    x, u, seeds, want = grid_case()
    assert np.array_equal(host(K.kmeans_plusplus(x, 48, u=u, device=cuda)), seeds)
    km = K.KMeans(48, init=x[seeds]).fit(x, device=cuda)
    assert km.n_iter_ == want["n_iter"] and km.readbacks_ <= km.n_iter_ + 2
    assert np.array_equal(host(km.labels_), want["labels"])
    assert np.array_equal(host(km.cluster_centers_), want["centers"])
    assert np.array_equal(host(km.counts_), want["counts"])
    assert abs(km.inertia_ - want["inertia"]) <= len(x) * EPS * want["inertia"]


@pytest.mark.parametrize("max_iter", [1, 5])
def test_fit_stopped_early_equals_the_restatement(cuda, max_iter):
    g = fixture("small")
    x = g["points"].astype(np.float64)
    want = ref.lloyd(x, x[g["seeds"]], max_iter=max_iter)
    assert want["n_iter"] == max_iter < int(g["n_iter"])
    km = K.KMeans(16, init=x[g["seeds"]], max_iter=max_iter).fit(g["points"], device=cuda)
    assert km.n_iter_ == max_iter and np.array_equal(host(km.labels_), want["labels"])
    assert np.array_equal(host(km.counts_), want["counts"])
    assert np.abs(host(km.cluster_centers_) - want["centers"]).max() <= want["counts"].max() * EPS * 180
    fresh = K.kmeans_assign(x, km.cluster_centers_, device=cuda)
    assert torch.equal(fresh.labels, km.labels_)


def torch_visible_syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, len([w for w in caught if "synchroniz" in str(w.message).lower()])


def test_readbacks_are_all_the_synchronisation(cuda):
    g = fixture("small")
    x = torch.as_tensor(g["points"], device=cuda)
    u = g["u"]
    K.KMeans(16, seed=1).fit(x)  # warm: allocator, library
    _, syncs = torch_visible_syncs(lambda: K.kmeans_plusplus(x, 16, u=u))
    assert syncs <= 1  # the status, at the end
    km, syncs = torch_visible_syncs(lambda: K.KMeans(16, seed=int(g["u_seed"])).fit(x))
    print("fit: n_iter", km.n_iter_, "readbacks", km.readbacks_, "torch-visible syncs", syncs)
    assert syncs <= km.readbacks_ <= km.n_iter_ + 2


# -- 5. statistics -------------------------------------------------------------------------------
def stats_case(cuda, which):
    g = fixture("medium")
    x = g["points"].astype(np.float64)[:3000]
    if which == "kdtree":
        tree = geo.KDTreeClustering(200).fit(x, device=cuda)
        return x, host(tree.clusters), tree.num_clusters
    km = K.KMeans(24, seed=3).fit(x, device=cuda)
    return x, host(km.labels_), 24


@pytest.mark.parametrize("which", ["kdtree", "kmeans"])
def test_cluster_stats_match_cluster_params(cuda, which):
    x, labels, c = stats_case(cuda, which)
    mus, std, cor = (host(t) for t in K.cluster_stats(x, labels, c, raw=False, device=cuda))
    for k in range(c):
        m = x[labels == k]
        cov = np.cov(m, rowvar=False)
        s = np.sqrt(np.diag(cov))
        assert np.all(np.abs(std[k] - s) <= 1e-9 * s), k
        assert abs(cor[k] * std[k, 0] * std[k, 1] - cov[0, 1]) <= 1e-9 * s[0] * s[1], k
        assert np.all(np.abs(mus[k] - m.mean(axis=0)) <= len(m) * EPS * np.abs(m).max(axis=0)), k
    # the raw transforms, on the device's own (std, cor)
    _, raw_s, raw_c = (host(t) for t in K.cluster_stats(x, labels, c, raw=True, device=cuda))
    np.testing.assert_allclose(raw_s, ref.raw_sigma(std), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(raw_c, ref.raw_corxy(cor), rtol=1e-12, atol=1e-14)
    # the host function's float32 results: one rounding to float32 apart at the most
    for raw in (False, True):
        want = M.cluster_params(x, labels, c, raw=raw)
        got = K.cluster_stats(x, labels, c, raw=raw, device=cuda)
        for w, t in zip(want, got):
            np.testing.assert_allclose(host(t).astype(np.float32), w, rtol=2.0 ** -22, atol=1e-7)


def test_cluster_stats_fallbacks(cuda):
    rng = np.random.default_rng(16)
    x = np.vstack([rng.normal([10, 20], [1, 2], (40, 2)),      # 0: an ordinary cluster
                   [[5.0, 5.0]],                                # 1: a single member
                   [[1.0, 2.0], [2.0, 4.5]],                    # 2: two members
                   np.full((4, 2), 37.5),                       # 3: identical points
                   np.column_stack([np.full(5, 3.25), np.arange(5.0)])])  # 5: one zero variance
    labels = np.array([0] * 40 + [1] + [2] * 2 + [3] * 4 + [5] * 5, np.int32)  # 4 is empty
    centers = np.arange(12.0).reshape(6, 2)
    for raw in (False, True):
        mus, sig, cor = (host(t) for t in K.cluster_stats(x, labels, 6, centers=centers, raw=raw,
                                                          device=cuda))
        one = np.float32(ref.raw_sigma(np.float64(1.0)) if raw else 1.0)
        for k in (1, 3, 4, 5):
            assert sig[k].astype(np.float32).tolist() == [one, one] and cor[k] == 0.0, (raw, k)
        assert mus[4].tolist() == [8.0, 9.0]                   # the centre passed in
        assert mus[3].tolist() == [37.5, 37.5] and mus[1].tolist() == [5.0, 5.0]
        keep = labels != 4
        lab5 = np.where(labels[keep] == 5, 4, labels[keep])
        h_mus, h_sig, h_cor = M.cluster_params(x[keep], lab5, 5, raw=raw)
        for k, hk in ((1, 1), (3, 3), (5, 4)):                 # the host's fallbacks, exactly
            assert np.array_equal(sig[k].astype(np.float32), h_sig[hk])
            assert np.float32(cor[k]) == h_cor[hk]
        np.testing.assert_allclose(sig[0].astype(np.float32), h_sig[0], rtol=2.0 ** -22)
        np.testing.assert_allclose(mus[[0, 2]].astype(np.float32), h_mus[[0, 2]], rtol=2.0 ** -22)
    _, std, cor = (host(t) for t in K.cluster_stats(x, labels, 6, raw=False, device=cuda))
    s2 = np.sqrt(np.diag(np.cov(x[41:43], rowvar=False)))
    assert np.all(np.abs(std[2] - s2) <= 1e-9 * s2) and abs(cor[2] - 1.0) <= 1e-9
    nomean = K.cluster_stats(x, labels, 6, raw=False, device=cuda)[0]
    assert bool(torch.isnan(nomean[4]).all())
    with pytest.raises(ValueError):
        K.cluster_stats(x, np.full(len(x), 6, np.int32), 6, device=cuda)


# -- 6. the models -------------------------------------------------------------------------------
def best_seed(x, c, cuda):
    """k-means' usual restarts: of three seeds the one with the lowest inertia."""
    return min(range(3), key=lambda s: K.KMeans(c, seed=s).fit(x, device=cuda).inertia_)


def test_get_cluster_centers_feeds_the_shared_model(cuda):
    """test_mdn_shared_gpu.test_two_melbournes' problem with C = 4, once from the k-d-tree
    regions as there and once from get_cluster_centers: the k-means centres land on the two
    places, and the dev loss after training does not exceed the k-d-tree fit's by more than
    that test's margin, 1e-4 max(1, |loss|)."""
    n = 300
    rs = np.random.RandomState(11)
    centres = np.array([[28.0836, -80.6081], [-37.8136, 144.9631]])
    fl = rs.multivariate_normal(centres[0], np.eye(2), size=n).astype(np.float32)
    au = rs.multivariate_normal(centres[1], np.eye(2), size=2 * n).astype(np.float32)
    X = sps.csr_matrix(rs.uniform(-0.1, 0.1, size=(3 * n, 2)) + np.array([1, 0])).astype(np.float32)
    Y = np.vstack((fl, au))
    idx = np.arange(3 * n)
    rs.shuffle(idx)
    X, Y = X[idx], Y[idx]
    n_tr, n_dev, batch, epochs = 2 * n, n // 2, 20, 10
    Xtr, Ytr, Xdev, Ydev = X[:n_tr], Y[:n_tr], X[n_tr:n_tr + n_dev], Y[n_tr:n_tr + n_dev]
    tree = geo.KDTreeClustering(150).fit(Ytr, device=cuda)
    assert tree.num_clusters == 4
    kd = M.cluster_params(Ytr, host(tree.clusters), 4, raw=True)
    km = K.get_cluster_centers(Ytr, 4, seed=best_seed(Ytr, 4, cuda), device=cuda)
    assert [a.shape for a in km] == [(4, 2), (4, 2), (4,)] and all(a.dtype == np.float32 for a in km)
    near = np.abs(km[0][:, None, :] - centres[None]).max(axis=-1) < 3.0
    assert near.sum(axis=1).tolist() == [1, 1, 1, 1] and near[:, 0].any() and near[:, 1].any()

    def final_loss(mus, sigmas, corxy):
        rs = np.random.RandomState(5)
        init = []
        for fan_in, fan_out in ((2, 100), (100, 4)):
            a = np.sqrt(6.0 / (fan_in + fan_out))
            init += [rs.uniform(-a, a, size=(fan_in, fan_out)).astype(np.float32),
                     np.zeros(fan_out, np.float32)]
        init += [mus, sigmas, corxy]
        orders = [rs.permutation(n_tr) for _ in range(epochs)]
        clf = M.NNModel_lang2locshared(n_epochs=epochs, batch_size=batch, regul_coef=1e-6,
                                       hid_size=100, ncomp=4, early_stopping_max_down=epochs,
                                       mus=mus, sigmas=sigmas, corxy=corxy,
                                       init_parameters=init, device=cuda)
        clf.fit(Xtr, Ytr, Xdev, Ydev, epoch_orders=orders)
        return clf.history[-1]["val_loss"]

    loss_kd, loss_km = final_loss(*kd), final_loss(*km)
    print("dev loss: k-d-tree", loss_kd, "k-means", loss_km)
    assert loss_km <= loss_kd + 1e-4 * max(1.0, abs(loss_kd))


def test_get_cluster_centers_feeds_loc2lang(cuda):
    """test_loc2lang_gpu.test_two_regions' problem (no hidden layer), from the k-d-tree regions
    as there and from get_cluster_centers with C = 4; the margin is that test's 1e-4 |loss|."""
    Xtr, Ytr, Xdev, Ydev = R.two_regions_data()
    tree = geo.KDTreeClustering(100).fit(Xtr, device=cuda)
    assert tree.num_clusters == 4
    kd = M.cluster_params(Xtr, host(tree.clusters), 4, raw=True)
    km = K.get_cluster_centers(Xtr, 4, seed=best_seed(Xtr, 4, cuda), device=cuda)
    near = np.abs(km[0][:, None, :] - R.MELBOURNES[None]).max(axis=-1) < 3.0
    assert near.sum(axis=1).tolist() == [1, 1, 1, 1] and near[:, 0].any() and near[:, 1].any()

    def final_loss(comp):
        rs = np.random.RandomState(7)
        orders = [rs.permutation(400) for _ in range(60)]
        clf = L.NNModel_loc2lang(n_epochs=60, batch_size=50, hid_size=0, n_gaus_comp=4,
                                 early_stopping_max_down=60,
                                 init_parameters=R.two_regions_init(comp, 0), device=cuda)
        clf.fit(Xtr, Ytr, Xdev, Ydev, Xdev, Ydev, epoch_orders=orders)
        return clf.history[-1]["val_loss"]

    loss_kd, loss_km = final_loss(kd), final_loss(km)
    print("dev loss: k-d-tree", loss_kd, "k-means", loss_km)
    assert loss_km <= loss_kd + 1e-4 * abs(loss_kd)


def test_example_runs_with_kmeans_init(cuda):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "loc2lang_pipeline.py"),
                          "--init", "kmeans", "--ncomp", "6"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout, res.stderr)
    assert "k-means -> 6 Gaussians" in res.stdout
