"""graphconvgeo_amd.geo on the GPU against the float64 numpy restatement (tests/geo_reference.py)
and the reference's own labels (tests/golden/kdtree_labels.npz): k-d-tree labels, class
medians, nearest class, haversine, geo_eval, errors, stream reuse and the example."""
import json
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

import geo_reference as ref
from graphconvgeo_amd import geo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kdtree_labels.npz")
# readbacks of one KDTreeClustering.fit beyond the tree depth: the level that
# finds nothing left to split, and the cluster count
FIT_EXTRA_READBACKS = 2


def golden_cases():
    z = np.load(GOLDEN)
    return [(str(n), z[f"{n}_locs"], int(z[f"{n}_bucket"]), z[f"{n}_labels"], int(z[f"{n}_num"]))
            for n in z["names"]]


def us_points(rng, n):
    return np.column_stack([rng.uniform(25, 50, n), rng.uniform(-125, -65, n)])


@pytest.fixture(scope="module")
def case1_medians():
    """The 64 class medians of the fixture's uniform case, from numpy."""
    name, locs, bucket, labels, num = golden_cases()[0]
    assert name == "uniform" and num == 64
    return ref.class_medians(locs, labels, num)


def assert_bitwise(got: torch.Tensor, want: np.ndarray):
    g = got.cpu().numpy()
    assert g.dtype == np.float64 and g.shape == want.shape
    assert np.array_equal(g.view(np.int64), np.ascontiguousarray(want).view(np.int64))


# ---------------------------------------------------------------- labels and medians

@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_labels_and_medians_on_the_fixture(cuda, case):
    name, locs, bucket, labels, num = case
    tree = geo.KDTreeClustering(bucket).fit(locs, device=cuda)
    assert tree.clusters.dtype == torch.int32 and tree.clusters.device.type == "cuda"
    assert tree.num_clusters == num
    assert np.array_equal(tree.clusters.cpu().numpy(), labels)
    want = ref.class_medians(locs.astype(np.float64), labels, num)
    assert_bitwise(tree.medians, want)
    # the general entry (any labels) gives the same medians
    assert_bitwise(geo.class_medians(locs, labels, num, device=cuda), want)
    if locs.dtype == np.float32:  # widened on the device = widened on the host
        wide = geo.KDTreeClustering(bucket).fit(locs.astype(np.float64), device=cuda)
        assert torch.equal(wide.clusters, tree.clusters)
        assert torch.equal(wide.medians, tree.medians)


def test_class_medians_of_arbitrary_labels(cuda):
    rng = np.random.default_rng(77)
    locs = np.round(us_points(rng, 5001), 1)
    labels = rng.integers(0, 300, 5001)
    labels[labels == 17] = 18  # an empty class: NaN, as np.median of nothing
    want = ref.class_medians(locs, labels, 301)
    got = geo.class_medians(torch.as_tensor(locs, device=cuda), torch.as_tensor(labels, device=cuda), 301)
    assert np.isnan(want[17]).all() and np.isnan(want[300]).all()
    g = got.cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(want))
    assert np.array_equal(g[~np.isnan(want)], want[~np.isnan(want)])


@pytest.mark.parametrize("rounded", [False, True], ids=["uniform", "rounded_half_degree"])
def test_labels_at_scale(cuda, rounded):
    """N = 70,001 crosses workgroup and scan-block boundaries; the 0.5-degree grid makes the
    data duplicate-heavy (about 11 points per distinct location)."""
    rng = np.random.default_rng(77)
    locs = us_points(rng, 70_001)
    if rounded:
        locs = np.round(locs * 2) / 2
    want, num, depth = ref.kdtree_labels(locs, 300)
    tree = geo.KDTreeClustering(300).fit(locs, device=cuda)
    assert tree.num_clusters == num and tree.depth == depth
    assert np.array_equal(tree.clusters.cpu().numpy(), want)
    assert_bitwise(tree.medians, ref.class_medians(locs, want, num))


# ---------------------------------------------------------------- nearest class

def check_nearest(cuda, queries, medians):
    d = ref.distance_matrix(queries, medians)
    want = d.argmin(axis=1)
    if medians.shape[0] > 1:
        two = np.partition(d, 1, axis=1)[:, :2]
        gap = float((two[:, 1] - two[:, 0]).min())
        print(f"nearest_class: C={medians.shape[0]} min gap best/second = {gap:.3e} km")
        assert gap > 1e-6  # the argmin is decided well above float64 rounding
    idx, dist = geo.nearest_class(queries, medians, return_distance=True, device=cuda)
    assert idx.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), want)  # every query, no exemptions
    err = np.abs(dist.cpu().numpy() - d[np.arange(len(want)), want]).max()
    print(f"nearest_class: max distance error {err:.3e} km")
    assert err < 1e-6
    assert torch.equal(geo.nearest_class(queries, medians, device=cuda), idx)


def test_nearest_class_against_numpy(cuda, case1_medians):
    rng = np.random.default_rng(77)
    check_nearest(cuda, us_points(rng, 1000), case1_medians)


def test_nearest_class_one_class_and_beyond_one_lds_tile(cuda):
    rng = np.random.default_rng(77)
    queries = us_points(rng, 64)
    check_nearest(cuda, queries, np.array([[40.0, -100.0]]))
    check_nearest(cuda, queries, us_points(rng, 9000))
    # the first index wins a tie
    med = np.array([[10.0, 10.0], [30.0, -90.0], [30.0, -90.0], [10.0, 10.0]])
    idx = geo.nearest_class(np.array([[31.0, -91.0], [9.0, 11.0]]), med, device=cuda)
    assert idx.tolist() == [1, 0]


# ---------------------------------------------------------------- haversine and geo_eval

def test_haversine_km(cuda):
    rng = np.random.default_rng(77)
    a = np.column_stack([rng.uniform(-90, 90, 4099), rng.uniform(-180, 180, 4099)])
    b = np.column_stack([rng.uniform(-90, 90, 4099), rng.uniform(-180, 180, 4099)])
    a[:3], b[:3] = [[0, 0], [12.5, 7.0], [-33.0, 151.0]], [[0, 90], [12.5, 7.0], [51.5, -0.1]]
    for radius in (6371.0088, 6371.0):
        want = ref.haversine_km(a, b, radius)
        assert want.max() < math.pi * radius - 1.0  # at least 1 km from antipodal
        got = geo.haversine_km(a, b, radius, device=cuda).cpu().numpy()
        err = np.abs(got - want).max()
        print(f"haversine_km: R={radius} max error {err:.3e} km")
        assert err < 1e-6
        assert got[1] == 0.0
    f32 = geo.haversine_km(a.astype(np.float32), b.astype(np.float32), device=cuda).cpu().numpy()
    assert np.abs(f32 - ref.haversine_km(a.astype(np.float32), b.astype(np.float32))).max() < 1e-6


def check_geo_eval(got, pred, locs, medians, **kw):
    mean, median, acc, d = ref.geo_eval(pred, locs, medians, **kw)
    radius = kw.get("earth_radius_km", ref.EARTH_RADIUS_KM)
    thr = kw.get("threshold_km", 161.0)
    assert d.max() < math.pi * radius - 1.0
    near = float(np.abs(d - thr).min())
    print(f"geo_eval: M={len(d)} nearest distance to the threshold {near:.3e} km")
    assert near > 1e-6  # Acc@161 is decided well above float64 rounding
    g_mean, g_median, g_acc, g_d = got
    err = np.abs(g_d.cpu().numpy() - d).max()
    print(f"geo_eval: max distance error {err:.3e} km, mean {g_mean} vs {mean}, "
          f"median {g_median} vs {median}, acc {g_acc} vs {acc}")
    assert err < 1e-6
    assert abs(g_mean - mean) <= 1e-12 * abs(mean)
    assert abs(g_median - median) < 1e-6
    assert g_acc == acc


@pytest.mark.parametrize("m", [1000, 999, 1], ids=["even", "odd", "one"])
def test_geo_eval_against_numpy(cuda, case1_medians, m):
    rng = np.random.default_rng(77)
    locs = us_points(rng, m)
    pred = rng.integers(0, 64, m)
    pred[: m // 2] = ref.nearest_class(locs[: m // 2], case1_medians)[0]  # half near, half far
    for dtype in (torch.int64, torch.int32):
        p = torch.as_tensor(pred, device=cuda).to(dtype)
        got = geo.geo_eval(p, locs, case1_medians, return_distances=True)
        check_geo_eval(got, pred, locs, case1_medians)
    got = geo.geo_eval(pred, locs.astype(np.float32), case1_medians, earth_radius_km=6371.0,
                       threshold_km=500.0, return_distances=True, device=cuda)
    check_geo_eval(got, pred, locs.astype(np.float32), case1_medians, earth_radius_km=6371.0,
                   threshold_km=500.0)
    assert len(geo.geo_eval(pred, locs, case1_medians, device=cuda)) == 3


def test_mlpconv_geo_eval(cuda):
    """MLPCONV.geo_eval feeds the device predictions of predict() into geo_eval."""
    from graphconvgeo_amd.mlpconv import MLPCONV
    from graphconvgeo_amd.synth import synthetic_features, synthetic_graph

    n, c = 600, 8
    rng = np.random.default_rng(77)
    H = synthetic_graph(n, 3000)
    X = synthetic_features(n, 64, nnz_per_row=8, empty_frac=0.0)
    locs = us_points(rng, n)
    tr, dv, te = np.arange(0, 400, dtype=np.int32), np.arange(400, 500, dtype=np.int32), \
        np.arange(500, n, dtype=np.int32)
    train_lab, dev_lab, test_lab, medians = geo.assign_classes(locs[tr], locs[dv], locs[te], 50,
                                                               device=cuda)
    Y = torch.cat([train_lab, dev_lab, test_lab]).cpu().numpy()
    assert medians.shape == (c, 2) and Y.max() == c - 1
    clf = MLPCONV(n_epochs=3, hidden_layer_size=16, device=cuda, seed=1)
    clf.fit(X, tr, dv, te, Y, H)
    pred = clf.predict("test")
    got = clf.geo_eval("test", locs[te], medians)
    mean, median, acc, d = ref.geo_eval(pred, locs[te], medians.cpu().numpy())
    assert abs(got[0] - mean) <= 1e-12 * mean and abs(got[1] - median) < 1e-6
    assert np.abs(d - 161.0).min() > 1e-6 and got[2] == acc
    with pytest.raises(ValueError):
        clf.geo_eval("nope", locs[te], medians)


def test_assign_classes_mirrors_assignClasses(cuda):
    rng = np.random.default_rng(77)
    train, dev, test = us_points(rng, 3000), us_points(rng, 400), us_points(rng, 401)
    tl, dl, sl, med = geo.assign_classes(train, dev, test, 50, device=cuda)
    want, num, _ = ref.kdtree_labels(train, 50)
    want_med = ref.class_medians(train, want, num)
    assert np.array_equal(tl.cpu().numpy(), want)
    assert_bitwise(med, want_med)
    for got, q in ((dl, dev), (sl, test)):
        d = ref.distance_matrix(q, want_med)
        two = np.partition(d, 1, axis=1)[:, :2]
        assert (two[:, 1] - two[:, 0]).min() > 1e-6
        assert np.array_equal(got.cpu().numpy(), d.argmin(axis=1))


# ---------------------------------------------------------------- errors

def test_errors_leave_the_device_usable(cuda, case1_medians):
    good = np.array([[40.0, -100.0], [41.0, -101.0], [42.0, -99.0]])

    def still_works():
        tree = geo.KDTreeClustering(1).fit(good, device=cuda)
        assert tree.num_clusters == 3 and sorted(tree.clusters.tolist()) == [0, 1, 2]

    for bad in (np.nan, np.inf, -np.inf):
        locs = us_points(np.random.default_rng(1), 1000)
        locs[517, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            geo.KDTreeClustering(10).fit(locs, device=cuda)
        still_works()
    for bucket in (0, -3, 2.5):
        with pytest.raises(ValueError, match="bucket_size"):
            geo.KDTreeClustering(bucket).fit(good, device=cuda)
    for shape in ((3,), (3, 3), (2, 3, 2)):
        with pytest.raises(ValueError, match="shape"):
            geo.KDTreeClustering(2).fit(np.zeros(shape), device=cuda)
        with pytest.raises(ValueError, match="shape"):
            geo.nearest_class(np.zeros(shape), case1_medians, device=cuda)
    with pytest.raises(ValueError, match="shape"):
        geo.haversine_km(good, good[:2], device=cuda)
    for wrong in (64, -1):
        pred = np.array([0, wrong, 5])
        for dtype in (np.int32, np.int64):
            with pytest.raises(ValueError, match="prediction outside"):
                geo.geo_eval(pred.astype(dtype), good, case1_medians, device=cuda)
        still_works()
    with pytest.raises(ValueError, match="no rows"):
        geo.geo_eval(np.zeros(0, np.int64), np.zeros((0, 2)), case1_medians, device=cuda)
    with pytest.raises(ValueError, match="shape"):
        geo.geo_eval(np.zeros(2, np.int64), good, case1_medians, device=cuda)
    with pytest.raises(ValueError, match="label outside"):
        geo.class_medians(good, np.array([0, 1, 2]), 2, device=cuda)
    with pytest.raises(ValueError, match="radius"):
        geo.haversine_km(good, good, earth_radius_km=0.0, device=cuda)
    with pytest.raises(ValueError, match="CUDA"):
        geo.KDTreeClustering(2).fit(good, device="cpu")
    still_works()
    empty = geo.KDTreeClustering(5).fit(np.zeros((0, 2)), device=cuda)
    assert empty.num_clusters == 0 and empty.clusters.shape == (0,) and empty.medians.shape == (0, 2)
    assert geo.geo_eval([63], good[:1], case1_medians, device=cuda)[0] > 0


# ---------------------------------------------------------------- stream, reuse, syncs

def test_fit_twice_on_a_side_stream_and_sync_count(cuda):
    name, locs, bucket, labels, num = golden_cases()[1]  # the deep, duplicate-heavy case
    _, _, depth = ref.kdtree_labels(locs, bucket)
    x = torch.as_tensor(locs, device=cuda)
    tree = geo.KDTreeClustering(bucket)
    first = tree.fit(x).clusters.clone()
    first_med = tree.medians.clone()
    assert tree.depth == depth and tree.readbacks == depth + FIT_EXTRA_READBACKS
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        tree.fit(x)
        again, again_med = tree.clusters, tree.medians
    side.synchronize()
    assert torch.equal(first, again) and torch.equal(first_med, again_med)
    assert np.array_equal(again.cpu().numpy(), labels)
    # no host synchronization beyond the per-level scalar: the build's own readbacks are the
    # count above; whatever torch itself would add on top is caught here
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            tree.fit(x)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [w for w in caught if "synchroniz" in str(w.message).lower()]
    print(f"fit: depth {depth}, readbacks {tree.readbacks}, torch-visible syncs {len(syncs)}")
    assert len(syncs) + tree.readbacks <= depth + FIT_EXTRA_READBACKS
    assert torch.equal(tree.clusters, first)


# ---------------------------------------------------------------- the example

def test_geolocate_pipeline_with_kdtree_labels(cuda, monkeypatch, capsys):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import geolocate_pipeline as gp
    monkeypatch.setattr(sys, "argv", ["geolocate_pipeline.py", "--users", "3000", "--epochs", "60",
                                      "--kdtree-bucket", "150"])
    acc = gp.main()
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["classes"] > 1
    assert math.isfinite(rec["mean_km"]) and math.isfinite(rec["median_km"])
    assert rec["mean_km"] >= 0 and rec["median_km"] >= 0
    assert 0 <= rec["acc_at_161"] <= 100
    assert rec["chance"] == round(1.0 / rec["classes"], 4)
    assert acc == pytest.approx(rec["test_acc"], abs=1e-4) and acc > rec["chance"]
