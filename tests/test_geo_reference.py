"""The numpy restatement of the k-d-tree labels (tests/geo_reference.py) equals the reference's
own KDTreeClustering label for label on the nine committed cases (tests/golden/
kdtree_labels.npz, written by tests/golden/make_geo_golden.py), and the restated metrics hold
their defining properties. No GPU."""
import os

import numpy as np
import pytest

import geo_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kdtree_labels.npz")
# cluster counts fixed by the construction of the case, whatever the generator draws
KNOWN_COUNTS = {"uniform": 64, "identical": 1, "const_lat": 7, "split_eq_max": 2,
                "bucket_one": 257, "n_eq_bucket": 1, "width_tie": 3, "float32": 32}


def golden_cases():
    z = np.load(GOLDEN)
    return [(str(n), z[f"{n}_locs"], int(z[f"{n}_bucket"]), z[f"{n}_labels"], int(z[f"{n}_num"]))
            for n in z["names"]]


def test_fixture_holds_the_nine_cases():
    cases = golden_cases()
    assert len(cases) == 9
    for name, locs, bucket, labels, num in cases:
        assert locs.ndim == 2 and locs.shape[1] == 2 and labels.shape == (locs.shape[0],)
        assert num == labels.max() + 1 == np.unique(labels).size
        if name in KNOWN_COUNTS:
            assert num == KNOWN_COUNTS[name], name
    by_name = {c[0]: c for c in cases}
    assert by_name["float32"][1].dtype == np.float32
    assert by_name["cities"][4] > 100  # duplicate-heavy: many small and over-full leaves


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_restatement_equals_reference_labels(case):
    name, locs, bucket, labels, num = case
    got, got_num, depth = ref.kdtree_labels(locs, bucket)
    assert got_num == num
    assert np.array_equal(got, labels)
    assert got.dtype == np.int32 and depth >= (1 if num > 1 else 0)


def test_cities_case_has_overfull_leaves_of_identical_points():
    name, locs, bucket, labels, num = [c for c in golden_cases() if c[0] == "cities"][0]
    sizes = np.bincount(labels)
    full = np.flatnonzero(sizes > bucket)
    assert full.size > 0
    for c in full:
        assert np.unique(locs[labels == c], axis=0).shape[0] == 1


def test_metric_restatements():
    # a quarter of a great circle, and one degree of latitude
    r = ref.EARTH_RADIUS_KM
    d = ref.haversine_km(np.array([[0.0, 0.0], [10.0, 20.0]]), np.array([[0.0, 90.0], [11.0, 20.0]]))
    assert abs(d[0] - np.pi * r / 2) < 1e-9 and abs(d[1] - np.pi * r / 180) < 1e-9
    assert ref.haversine_km([[1.0, 2.0]], [[1.0, 2.0]], 6371.0)[0] == 0.0
    med = np.array([[0.0, 0.0], [0.0, 0.0], [5.0, 5.0]])
    idx, dist = ref.nearest_class(np.array([[0.1, 0.0], [4.0, 5.0]]), med)
    assert idx.tolist() == [0, 2]  # the first index on a tie
    mean, median, acc, dd = ref.geo_eval([0, 2, 2], np.array([[0.0, 1.0], [5.0, 5.0], [50.0, 5.0]]), med)
    assert dd[1] == 0.0 and median == dd[0] and acc == 100 * 2 / 3.0
    assert abs(mean - dd.sum() / 3) < 1e-9
    cm = ref.class_medians(np.array([[1.0, 2.0], [3.0, 5.0], [9.0, 9.0]]), [0, 0, 2], 3)
    assert cm[0].tolist() == [2.0, 3.5] and np.isnan(cm[1]).all() and cm[2].tolist() == [9.0, 9.0]
