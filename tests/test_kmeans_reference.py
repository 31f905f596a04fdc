"""CPU side of the k-means initialisation (graphconvgeo_amd.kmeans, csrc/kmeans.hip): the NumPy
restatement (tests/kmeans_reference.py) against the committed sklearn fixtures
(tests/golden/kmeans_*.npz, written by tests/golden/make_kmeans_golden.py) and, where sklearn is
installed, against a live KMeans run; the ABI's argument checks and every ValueError of the
Python layer, none of which needs a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import kmeans_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("small", "medium", "large")
KMEANS_ENTRIES = ("gcg_kmeans_centre_tile", "gcg_kmeans_assign_f64_workspace_bytes",
                  "gcg_kmeans_assign_f64", "gcg_kmeans_update_f64_workspace_bytes",
                  "gcg_kmeans_update_f64", "gcg_kmeans_pp_f64_workspace_bytes",
                  "gcg_kmeans_pp_f64", "gcg_cluster_stats_f64_workspace_bytes",
                  "gcg_cluster_stats_f64")


def load(name):
    return np.load(os.path.join(GOLDEN, f"kmeans_{name}.npz"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_sklearn_fixture(name):
    g = load(name)
    x = g["points"].astype(np.float64)
    assert g["points"].dtype == np.float32 and g["gap"] >= 1e-7 and g["margin"] >= 1e-9
    c = g["centers"].shape[0]
    seeds, margin = ref.plusplus(x, c, g["u"], return_margin=True)
    assert np.array_equal(seeds, g["seeds"]) and margin == g["margin"]
    assert np.array_equal(g["u"], np.random.default_rng(int(g["u_seed"])).random(c))
    got = ref.lloyd(x, x[seeds])
    assert np.array_equal(got["labels"], g["labels"]) and got["n_iter"] == int(g["n_iter"])
    n_max = int(got["counts"].max())
    assert got["counts"].min() > 0
    assert np.abs(got["centers"] - g["centers"]).max() <= n_max * 2.0 ** -53 * 180
    assert abs(got["inertia"] - float(g["inertia"])) <= 1e-12 * float(g["inertia"])


def test_restatement_against_a_live_sklearn_run():
    cluster = pytest.importorskip("sklearn.cluster")
    x = ref.blobs(2000, 12, seed=31).astype(np.float64)
    seeds = ref.plusplus(x, 12, np.random.default_rng(4).random(12))
    got = ref.lloyd(x, x[seeds], return_gap=True)
    assert got["gap"] >= 1e-7  # no label hangs on the summation order
    sk = cluster.KMeans(n_clusters=12, init=x[seeds], n_init=1, tol=0, algorithm="lloyd").fit(x)
    assert np.array_equal(sk.labels_, got["labels"]) and sk.n_iter_ == got["n_iter"]
    assert np.abs(sk.cluster_centers_ - got["centers"]).max() <= got["counts"].max() * 2.0 ** -53 * 180
    assert abs(sk.inertia_ - got["inertia"]) <= 1e-12 * got["inertia"]


def test_restatement_rules():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 0.0], [4.0, 4.0], [4.0, 4.0]])
    lab, d = ref.assign(x, np.array([[1.0, 0.0], [0.0, 0.0], [0.0, 0.0], [np.nan, 0.0]]))
    assert lab.tolist() == [1, 0, 0, 0, 0] and d[2] == 0.25  # tie and duplicate: the first index
    new, counts = ref.update(x, lab, np.full((4, 2), 9.0))
    assert counts.tolist() == [4, 1, 0, 0] and new[2].tolist() == [9.0, 9.0]
    # a point at distance 0 from a chosen centre is never picked: 3 distinct points, 3 seeds
    for u in ([0.99, 0.0, 0.0], [0.0, 0.999999, 0.5], [0.7, np.nextafter(1.0, 0), 0.0]):
        seeds = ref.plusplus(x, 3, np.array(u))
        assert len({tuple(x[i]) for i in seeds}) == 3
    with pytest.raises(ValueError):
        ref.plusplus(x, 5, np.full(5, 0.5))
    out = ref.lloyd(x, x[[0, 3]], max_iter=1)
    assert out["n_iter"] == 1 and np.array_equal(out["labels"], ref.assign(x, out["centers"])[0])


def test_stats_restatement_matches_cluster_params():
    from graphconvgeo_amd.mdn import cluster_params
    rng = np.random.default_rng(3)
    x = np.vstack([rng.normal([10, 20], [1, 2], (50, 2)), [[5.0, 5.0]], np.full((4, 2), 37.5)])
    lab = np.array([0] * 25 + [1] * 25 + [2] + [3] * 4)
    for raw in (True, False):
        mus, sig, cor = cluster_params(x, lab, 4, raw=raw)
        m, s, c, counts = ref.stats(x, lab, 4, raw=raw)
        assert counts.tolist() == [25, 25, 1, 4]
        np.testing.assert_allclose(m, mus, rtol=1e-6)
        np.testing.assert_allclose(s, sig, rtol=1e-6)
        np.testing.assert_allclose(c, cor, rtol=1e-6, atol=1e-7)
        assert np.array_equal(s[2:].astype(np.float32), sig[2:])  # the fallbacks, exactly
        assert np.array_equal(c[2:].astype(np.float32), cor[2:])


def test_kmeans_entries_are_declared_bound_and_built():
    from graphconvgeo_amd import _build, _native
    header = open(os.path.join(ROOT, "include", "gcg_spmm.h")).read()
    for name in KMEANS_ENTRIES:
        assert name + "(" in header and name in _native.SIGNATURES
    assert any(os.path.basename(s) == "kmeans.hip" for s in _build.SOURCES)


def test_kmeans_abi_argument_validation_without_gpu(native_lib):
    lib = native_lib
    a8, b8, c8, d8 = (C.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000))
    odd, odd2 = C.c_void_p(0x10004), C.c_void_p(0x10002)  # not 8-B / not 4-B aligned
    nb = C.c_size_t(7)
    assert lib.gcg_kmeans_centre_tile() >= 1
    assert lib.gcg_kmeans_assign_f64_workspace_bytes(5000, C.byref(nb)) == 0 and nb.value >= 5 * 8
    assert lib.gcg_kmeans_assign_f64_workspace_bytes(-1, C.byref(nb)) == 1
    assert lib.gcg_kmeans_assign_f64_workspace_bytes(5, None) == 1
    assert lib.gcg_kmeans_pp_f64_workspace_bytes(5000, C.byref(nb)) == 0 and nb.value >= 5000 * 8
    assert lib.gcg_kmeans_pp_f64_workspace_bytes(1 << 31, C.byref(nb)) == 1
    asg = lib.gcg_kmeans_assign_f64
    assert asg(-1, a8, 3, b8, None, c8, None, None, None, d8, None, 0, None) == 1
    assert asg(5, a8, 3, b8, None, c8, None, None, None, None, None, 0, None) == 1  # no status_dev
    assert b"status_dev" in lib.gcg_last_error()
    assert asg(5, a8, 3, b8, None, c8, None, d8, None, odd2, None, 0, None) == 2    # status misaligned
    upd = lib.gcg_kmeans_update_f64
    assert upd(-1, a8, b8, 3, c8, c8, d8, a8, b8, 1 << 20, None) == 1
    assert upd(5, a8, b8, 3, c8, c8, d8, None, b8, 1 << 20, None) == 1             # no status_dev
    assert upd(5, a8, b8, 3, c8, c8, d8, odd2, b8, 1 << 20, None) == 2
    st = lib.gcg_cluster_stats_f64
    assert st(5, a8, b8, 3, 2, c8, c8, c8, None, d8, a8, 1 << 20, None) == 1        # raw not 0 / 1
    assert st(5, a8, b8, -1, 1, c8, c8, c8, None, d8, a8, 1 << 20, None) == 1
    assert st(5, a8, b8, 3, 1, c8, c8, c8, None, None, a8, 1 << 20, None) == 1      # no status_dev
    pp = lib.gcg_kmeans_pp_f64
    assert pp(5, a8, 0, b8, c8, d8, a8, 1 << 20, None) == 1                          # C < 1
    assert pp(5, a8, 6, b8, c8, d8, a8, 1 << 20, None) == 1                          # C > N
    assert b"1 <= C <= N" in lib.gcg_last_error()
    assert pp(5, None, 2, b8, c8, d8, a8, 1 << 20, None) == 1
    assert pp(5, odd, 2, b8, c8, d8, a8, 1 << 20, None) == 2
    assert pp(5, a8, 2, b8, c8, d8, a8, 8, None) == 6                                # workspace
    assert pp(5, a8, 2, b8, c8, d8, None, 0, None) == 6


def test_python_layer_refuses_bad_input_without_gpu():
    from graphconvgeo_amd import kmeans as K
    good = np.arange(10.0).reshape(5, 2)
    bad = good.copy()
    bad[3, 1] = np.inf
    for call in (
            lambda: K.kmeans_plusplus(np.zeros((5, 3)), 2),              # shape
            lambda: K.kmeans_plusplus(np.zeros(5), 2),
            lambda: K.kmeans_plusplus(good, 0),                          # 1 <= C <= N
            lambda: K.kmeans_plusplus(good, 6),
            lambda: K.kmeans_plusplus(good, 2.5),
            lambda: K.kmeans_plusplus(bad, 2),                           # non-finite
            lambda: K.kmeans_plusplus(good, 2, u=[0.5, 1.0]),            # u in [0, 1)
            lambda: K.kmeans_plusplus(good, 2, u=[-0.1, 0.5]),
            lambda: K.kmeans_plusplus(good, 2, u=[0.5, np.nan]),
            lambda: K.kmeans_plusplus(good, 2, u=[0.5]),
            lambda: K.KMeans(6).fit(good),
            lambda: K.KMeans(2, max_iter=0).fit(good),
            lambda: K.KMeans(2, init="random").fit(good),
            lambda: K.KMeans(2, init=np.zeros((3, 2))).fit(good),
            lambda: K.KMeans(2, init=bad[2:4]).fit(good),
            lambda: K.KMeans(2).fit(bad),
            lambda: K.kmeans_assign(good, np.zeros((0, 2))),
            lambda: K.kmeans_assign(bad, good[:2]),
            lambda: K.kmeans_update(good, np.zeros(5, np.int32), np.zeros((0, 2))),
            lambda: K.cluster_stats(good, np.zeros(5, np.int32), 0),
            lambda: K.cluster_stats(good, np.zeros(5, np.int32), 2, centers=np.zeros((3, 2))),
            lambda: K.get_cluster_centers(good, 9),
            lambda: K.get_cluster_centers(bad, 2)):
        with pytest.raises(ValueError):
            call()
