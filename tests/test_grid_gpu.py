"""The grid representation on the GPU (csrc/grid.hip, graphconvgeo_amd.grid) against the numpy
restatement tests/grid_reference.py: structure exactly, values within one float32 ulp."""
import numpy as np
import pytest
import torch

import grid_reference as R

pytestmark = pytest.mark.gpu


def host(X):
    return X.indptr.cpu().numpy(), X.indices.cpu().numpy(), X.data.cpu().numpy()


def same(A, B):
    return all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(host(A), host(B)))


SETS = {
    "us": (R.us_set, dict(bbox=R.US_BBOX, grid_size=0.5, radius_km=161.0)),
    "world": (R.world_set, dict(bbox=R.WORLD_BBOX, grid_size=2.0, radius_km=500.0)),
}
# (entries, empty rows, rows with a coincident point, longest row), counted on the CPU
EXPECTED = {"us": (6258, 42, None, 41), "world": (14923, None, 4, 540)}
_reference = {}


def reference(name, R_km):
    """The restatement of an input set at an earth radius, computed once and left unchanged."""
    if (name, R_km) not in _reference:
        make, kw = SETS[name]
        x = make()
        ref, d = R.grid_representation(x, earth_radius_km=R_km, return_distances=True, **kw)
        for a in (ref.indptr, ref.indices, ref.data, d):
            a.setflags(write=False)
        _reference[(name, R_km)] = (x, ref, d)
    return _reference[(name, R_km)]


@pytest.mark.parametrize("name,R_km", [("us", 6371.0088), ("world", 6371.0088), ("world", 6371.0)])
def test_grid_matches_the_restatement(cuda, name, R_km):
    from graphconvgeo_amd import grid
    x, ref, d = reference(name, R_km)
    kw = SETS[name][1]
    # what makes the comparison fair, asserted on the restatement
    to_radius, smallest, not_coincident, at_pole = R.fairness(x, d, kw["radius_km"], kw["bbox"],
                                                              kw["grid_size"])
    assert to_radius > 1e-5 and smallest >= 1e-4 and not_coincident == 0 and at_pole == 0
    lens = np.diff(ref.indptr)
    entries, empty, coincident, longest = EXPECTED[name]
    assert ref.nnz == entries and lens.max() == longest
    if empty is not None:
        assert int((lens == 0).sum()) == empty
    zero_rows = np.nonzero((d == 0).any(axis=1))[0]
    if coincident is not None:
        assert zero_rows.size == coincident

    X = grid.grid_representation(x, earth_radius_km=R_km, device=cuda, **kw)
    assert X.shape == ref.shape and X.data.dtype == torch.float32
    assert X.indptr.dtype == torch.int32 and X.indices.dtype == torch.int32
    indptr, indices, data = host(X)
    assert np.array_equal(indptr, ref.indptr)
    assert np.array_equal(indices, ref.indices)
    ulps = R.ulp_distance(data, ref.data)
    print(name, R_km, "entries", ref.nnz, "max ulp", int(ulps.max()), "values off by one ulp",
          int((ulps > 0).sum()), "closest to the radius", to_radius, "smallest distance", smallest)
    assert ulps.max() <= 1
    for i in zero_rows:  # exactly 1.0 at the coincident column, +0.0 elsewhere
        row = data[indptr[i]:indptr[i + 1]]
        cols = indices[indptr[i]:indptr[i + 1]]
        at = d[i, cols] == 0
        assert at.sum() == 1 and row[at][0] == 1.0
        assert np.array_equal(row[~at].view(np.int32), np.zeros((~at).sum(), np.int32))
    # canonical: columns strictly ascending in every row
    inner = np.ones(indices.size, bool)
    inner[indptr[:-1][lens > 0]] = False
    assert (np.diff(indices.astype(np.int64), prepend=-1)[inner] > 0).all()


def test_window_against_all_columns(cuda):
    """The candidate window is a superset: at 259,200 columns the default and exhaustive=True give
    bitwise the same arrays, poles and antimeridian included."""
    from graphconvgeo_amd import grid
    rng = np.random.default_rng(5)
    lat = rng.uniform(-90, 90, 2000)
    lon = rng.uniform(-180, 180, 2000)
    x = np.concatenate([np.stack([lat, lon], axis=1), R.SPECIAL_WORLD,
                        [[37, -200], [-90, 13], [89.75, -179.75], [12.25, 359.9], [0.1, -540.2]]])
    kw = dict(bbox=R.WORLD_BBOX, grid_size=0.5, radius_km=161.0, device=cuda)
    A = grid.grid_representation(x, **kw)
    B = grid.grid_representation(x, exhaustive=True, **kw)
    assert A.shape == (x.shape[0], 360 * 720) and A.nnz > 0
    assert same(A, B)
    lens = np.diff(host(A)[0])
    # [90, 0]: whole latitude rows, every longitude of each
    assert lens[2000] >= 720 and lens[2000] % 720 == 0 and lens.min() > 0
    print("entries", A.nnz, "longest row", lens.max(), "mean", lens.mean())


def test_input_forms_and_reproducibility(cuda):
    from graphconvgeo_amd import grid, sparse as gs
    x = R.us_set()  # float32-representable
    kw = dict(bbox=R.US_BBOX, grid_size=0.5, radius_km=161.0, device=cuda)
    A = grid.grid_representation(x, **kw)
    assert same(A, grid.grid_representation(x, **kw))                                # two runs
    assert same(A, grid.grid_representation(x.astype(np.float32), **kw))
    assert same(A, grid.grid_representation(torch.from_numpy(x), **kw))              # host tensor
    assert same(A, grid.grid_representation(torch.from_numpy(x).to(cuda), **kw))
    assert same(A, grid.grid_representation(torch.from_numpy(x.astype(np.float32)).to(cuda), **kw))
    halves = [grid.grid_representation(x[:100], **kw), grid.grid_representation(x[100:], **kw)]
    assert same(A, gs.vstack(halves))
    E = grid.grid_representation(np.zeros((0, 2)), **kw)
    assert E.shape == (0, 5800) and E.nnz == 0 and E.indptr.tolist() == [0]
    A.validate()


@pytest.mark.parametrize("bad", [[float("nan"), 0.0], [30.0, float("inf")], [91.0, -100.0],
                                 [-90.5, 0.0]])
def test_refusals_found_on_the_device(cuda, bad):
    from graphconvgeo_amd import grid
    x = R.us_set()[:70].copy()
    x[67] = bad
    with pytest.raises(ValueError, match="non-finite coordinate or a latitude"):
        grid.grid_representation(x, device=cuda)
