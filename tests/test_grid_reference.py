"""CPU tests of the grid representation and of loc2lang's no-MDN baseline: the numpy restatement
(tests/grid_reference.py) against the reference's literal double loop, the C-ABI's argument
checks, every host-side refusal, and the restated float32 trainer against float64."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sps

import grid_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_ENTRIES = ("gcg_grid_count_f64_workspace_bytes", "gcg_grid_count_f64", "gcg_grid_fill_f64",
                "gcg_minibatch_w1_adamax_step_f32")
OK, INVAL, MISALIGNED, WORKSPACE = 0, 1, 2, 6


def small_problem():
    """12 points over a 6 x 7 grid at 1.5 degrees (radius 300 km): two on grid points, one out
    of every point's range."""
    bbox = (30.0, -100.0, 39.0, -89.5)
    lats, lons, coords = R.grid_tables(bbox, 1.5)
    assert (lats.size, lons.size) == (6, 7)
    rng = np.random.default_rng(3)
    x = np.stack([rng.uniform(29.5, 39.0, 12), rng.uniform(-100.5, -90.0, 12)], axis=1)
    x[4], x[9], x[11] = coords[10], coords[41], [50.0, -70.0]
    return x, bbox


def test_restatement_equals_the_reference_loop():
    x, bbox = small_problem()
    ref, d = R.grid_representation(x, 1.5, bbox, 300.0, return_distances=True)
    dense, mask = R.reference_loop(x, 1.5, bbox, 300.0)
    assert ref.shape == (12, 42) and ref.has_canonical_format
    # structure: exactly the pairs the loop stored, explicit zeros included
    stored = np.zeros_like(mask)
    stored[np.repeat(np.arange(12), np.diff(ref.indptr)), ref.indices] = True
    assert np.array_equal(stored, mask)
    assert np.array_equal(ref.toarray(), dense)
    lens = np.diff(ref.indptr)
    assert lens[11] == 0 and lens[:11].min() >= 1
    # the two coincident rows: 1.0 on the grid point, +0.0 on the others in range
    for i, col in ((4, 10), (9, 41)):
        row = ref.getrow(i)
        assert row.nnz == lens[i] > 1 and row[0, col] == 1.0 and row.sum() == 1.0
        assert (d[i, row.indices] < 300.0).all()


def test_rows_sum_to_one_or_are_empty():
    for make, kw in ((R.us_set, dict(bbox=R.US_BBOX, grid_size=0.5, radius_km=161.0)),
                     (R.world_set, dict(bbox=R.WORLD_BBOX, grid_size=4.0, radius_km=500.0))):
        X = R.grid_representation(make(), **kw)
        sums = np.asarray(X.astype(np.float64).sum(axis=1)).ravel()
        lens = np.diff(X.indptr)
        assert np.all(sums[lens == 0] == 0) and (kw["grid_size"] != 0.5 or (lens == 0).sum() == 42)
        assert np.abs(sums[lens > 0] - 1).max() < 1e-6
        assert X.data.dtype == np.float32 and X.indices.dtype == np.int32
        assert X.data.min() >= 0


def test_latlon_grid_and_exports():
    import graphconvgeo_amd as G
    from graphconvgeo_amd import grid
    assert G.US_BBOX == R.US_BBOX and G.WORLD_BBOX == R.WORLD_BBOX
    assert G.grid_representation is grid.grid_representation and G.LatLonGrid is grid.LatLonGrid
    g = G.LatLonGrid()
    lats, lons, coords = R.grid_tables(R.US_BBOX, 0.5)
    assert (g.lats.size, g.lons.size, g.n_points) == (50, 116, 5800)
    assert np.array_equal(g.lats, lats) and np.array_equal(g.lons, lons)
    assert g.coords().dtype == np.float64 and np.array_equal(g.coords(), coords)
    w = G.LatLonGrid(G.WORLD_BBOX, 2.0)
    assert w.n_points == 16200 and w.lats[0] == -90.0 and w.lons[-1] == 178.0


def test_entries_are_declared_bound_and_built():
    from graphconvgeo_amd import _build, _native
    header = open(os.path.join(ROOT, "include", "gcg_spmm.h")).read()
    for name in GRID_ENTRIES:
        assert name + "(" in header and name in _native.SIGNATURES
    assert any(os.path.basename(s) == "grid.hip" for s in _build.SOURCES)
    assert any(os.path.basename(h) == "haversine.h" for h in _build.INTERNAL_HEADERS)


def test_grid_abi_argument_validation_without_gpu(native_lib):
    lib = native_lib
    a, b, c, d, e, w = (C.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000))
    odd = C.c_void_p(0x10004)
    count, fill = lib.gcg_grid_count_f64, lib.gcg_grid_fill_f64
    grid_ = (50, b, 116, c, 161.0, 6371.0088, 0)

    def cnt(n=5, coords=a, g=grid_, indptr=d, norm=e, info=a, ws=w, nbytes=1 << 20):
        return count(n, coords, *g, indptr, norm, info, ws, nbytes, None)

    assert cnt(n=-1) == INVAL
    assert b"gcg_grid_count_f64" in lib.gcg_last_error()
    assert cnt(coords=None) == INVAL and cnt(indptr=None) == INVAL and cnt(norm=None) == INVAL
    assert cnt(info=None) == INVAL
    assert cnt(g=(50, None, 116, c, 161.0, 6371.0088, 0)) == INVAL
    assert cnt(g=(0, b, 116, c, 161.0, 6371.0088, 0)) == INVAL             # an empty grid
    assert cnt(g=(50, b, 0, c, 161.0, 6371.0088, 0)) == INVAL
    assert cnt(g=(3000, b, 200, c, 161.0, 6371.0088, 0)) == INVAL          # the tables' LDS bound
    assert b"LDS" in lib.gcg_last_error()
    assert cnt(g=(50, b, 116, c, 0.0, 6371.0088, 0)) == INVAL              # radius
    assert cnt(g=(50, b, 116, c, float("nan"), 6371.0088, 0)) == INVAL
    assert cnt(g=(50, b, 116, c, 20100.0, 6371.0088, 0)) == INVAL          # >= pi R
    assert cnt(g=(50, b, 116, c, 161.0, 0.0, 0)) == INVAL                  # earth radius
    assert cnt(g=(50, b, 116, c, 161.0, float("inf"), 0)) == INVAL
    assert cnt(g=(50, b, 116, c, 161.0, 6371.0088, 2)) == INVAL            # exhaustive
    assert cnt(coords=odd) == MISALIGNED and cnt(norm=odd) == MISALIGNED
    assert cnt(info=odd) == MISALIGNED
    assert cnt(g=(50, odd, 116, c, 161.0, 6371.0088, 0)) == MISALIGNED
    assert cnt(indptr=C.c_void_p(0x40002)) == MISALIGNED
    assert cnt(ws=None, nbytes=0) == WORKSPACE
    assert cnt(nbytes=64) == WORKSPACE                                      # short
    assert b"workspace" in lib.gcg_last_error()
    assert cnt(n=0, coords=None, indptr=None, norm=None, info=None, ws=None, nbytes=0) == OK

    def fil(n=5, coords=a, g=grid_, indptr=d, norm=e, nnz=40, indices=a, values=b):
        return fill(n, coords, *g, indptr, norm, nnz, indices, values, None)

    assert fil(n=-1) == INVAL and fil(nnz=-1) == INVAL and fil(nnz=1 << 31) == INVAL
    assert fil(coords=None) == INVAL and fil(indptr=None) == INVAL and fil(norm=None) == INVAL
    assert fil(indices=None) == INVAL and fil(values=None) == INVAL
    assert fil(g=(50, b, 116, c, -1.0, 6371.0088, 0)) == INVAL
    assert fil(norm=odd) == MISALIGNED and fil(values=C.c_void_p(0x20002)) == MISALIGNED
    assert fil(n=0, coords=None, indptr=None, norm=None, indices=None, values=None) == OK
    assert fil(nnz=0, indices=None, values=None) == OK                      # nothing to write
    nb = C.c_size_t(7)
    assert lib.gcg_grid_count_f64_workspace_bytes(0, C.byref(nb)) == OK and nb.value == 0
    assert lib.gcg_grid_count_f64_workspace_bytes(-1, C.byref(nb)) == INVAL
    assert lib.gcg_grid_count_f64_workspace_bytes(5, None) == INVAL


def test_w1_adamax_step_argument_validation_without_gpu(native_lib):
    step = native_lib.gcg_minibatch_w1_adamax_step_f32
    a = C.c_void_p(0x10000)
    tail = (a, a, a, a, a, a, 0.9, 0.999, 1e-8, None)
    assert step(-1, 4, a, a, a, a, 4, 8, *tail) == INVAL
    assert step(10, -4, a, a, a, a, 4, 8, *tail) == INVAL
    assert step(10, 4, a, a, a, a, 3, 8, *tail) == INVAL                       # ldg < K
    assert step(10, 4, None, a, a, a, 4, 8, *tail) == INVAL                    # NULL W
    assert step(10, 4, a, a, None, a, 4, 8, *tail) == INVAL                    # NULL u
    assert step(10, 4, a, a, a, None, 4, 8, *tail) == INVAL                    # NULL G
    assert step(10, 4, a, a, a, a, 4, 8, a, a, a, a, a, None, 0.9, 0.999, 1e-8,
                None) == INVAL                                                 # NULL step size
    assert "gcg_minibatch_w1_adamax_step_f32" in native_lib.gcg_last_error().decode()
    assert step(10, 4, C.c_void_p(0x10002), a, a, a, 4, 8, *tail) == MISALIGNED
    assert step(0, 4, None, None, None, None, 4, 8, None, None, None, None, None, None, 0.9,
                0.999, 1e-8, None) == OK                                       # empty: no launch
    assert step(10, 0, None, None, None, None, 0, 8, None, None, None, None, None, None, 0.9,
                0.999, 1e-8, None) == OK


def test_grid_representation_host_refusals():
    from graphconvgeo_amd import grid
    x = np.array([[40.0, -100.0], [30.0, -90.0]])
    for bad in (np.zeros((3, 3)), np.zeros(4), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match=r"shape \(N, 2\)"):
            grid.grid_representation(bad)
    for gs_ in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="grid_size"):
            grid.grid_representation(x, grid_size=gs_)
    with pytest.raises(ValueError, match="grid is empty"):
        grid.grid_representation(x, bbox=(40.0, -100.0, 40.0, -90.0))
    with pytest.raises(ValueError, match="grid is empty"):
        grid.grid_representation(x, bbox=(40.0, -90.0, 45.0, -100.0))
    with pytest.raises(ValueError, match="LDS"):
        grid.grid_representation(x, grid_size=1e-6)
    for radius in (0.0, -1.0, float("nan"), np.pi * 6371.0088, 1e9):
        with pytest.raises(ValueError, match="radius_km"):
            grid.grid_representation(x, radius_km=radius)
    for R_km in (0.0, -6371.0, float("inf")):
        with pytest.raises(ValueError, match="earth_radius_km"):
            grid.grid_representation(x, earth_radius_km=R_km)
    with pytest.raises(ValueError, match="GPU"):
        grid.grid_representation(x, device="cpu")


# -- loc2lang's no-MDN baseline: the restated trainer and the class's host-side refusals ---------
@pytest.mark.parametrize("hid", [8, 0])
@pytest.mark.parametrize("kind", ["dense", "grid"])
def test_float32_trainer_stays_within_the_trajectory_bound_of_float64(kind, hid):
    """What entitles tests/test_loc2lang_nomdn_gpu.py to hold the GPU fit to these bounds: the
    restated trainer in float32 on the CPU meets them against float64 on the same problems."""
    import torch
    import test_loc2lang_nomdn_gpu as T
    Xtr, Ytr, Xdev, Ydev, init, orders, B, _ = T.nomdn_problem(kind, hid)
    assert Xtr.shape == (96, 377 if kind == "grid" else 2) and Xdev.shape[0] == 40 and B == 32
    assert Ytr.shape[1] == 37 and len(orders) == 8
    if kind == "grid":
        assert sps.issparse(Xtr) and (np.diff(Xtr.indptr) == 0).sum() == 2
    ref_hist, ref_params = T.train(Xtr, Ytr, Xdev, Ydev, init, orders, B)
    hist, params = T.train(Xtr, Ytr, Xdev, Ydev, init, orders, B, dtype=torch.float32)
    assert all(v.dtype == np.float32 for v in params.values())
    T.within_trajectory_bound(hist, params, ref_hist, ref_params, f"float32 {kind} hid={hid}")
    ref_b = np.array([h["batch_losses"] for h in ref_hist])
    assert ref_b[-1].mean() < ref_b[0].mean()  # it trains
    assert all((ref_params[k] != np.asarray(v)).any() for k, v in zip(T.names(hid), init))


def test_nomdn_class_host_refusals():
    from graphconvgeo_amd import loc2lang as L
    N = L.NNModel_loc2lang_nomdn
    with pytest.raises(NotImplementedError, match="reload"):
        N(reload=True)
    with pytest.raises(ValueError, match="float32"):
        N(dtype="float64")
    for bad in (0, L.MAX_HIDDEN + 1):
        with pytest.raises(ValueError, match="n_gaus_comp"):
            N(n_gaus_comp=bad)
    with pytest.raises(ValueError, match="hid_size"):
        N(hid_size=L.MAX_HIDDEN + 1)
    with pytest.raises(ValueError, match="batch_size"):
        N(batch_size=0)
    with pytest.raises(ValueError, match="input_size"):
        N(input_size=0)
    clf = N(nomdn=True, input_size=5800, mus=np.zeros((3, 3)))  # mus is the Gaussians': unused
    assert clf.nomdn is True and clf.input_size == 5800 and clf.params is None
    assert clf.names == ["Wg", "bg", "Wh", "bh", "Wo", "bo"] and N(hid_size=0).names[2] == "Wo"
    with pytest.raises(RuntimeError, match="no parameters yet"):
        clf.get_params()
    # the Gaussian model keeps refusing both, and names the class that does not
    with pytest.raises(NotImplementedError, match="nomdn.*NNModel_loc2lang_nomdn"):
        L.NNModel_loc2lang(nomdn=True)
    with pytest.raises(NotImplementedError, match="grid.*NNModel_loc2lang_nomdn"):
        L.NNModel_loc2lang(input_size=7000)
    assert L.NNModel_loc2lang().nomdn is False and L.NNModel_loc2lang().input_size == 2
