"""The grid representation of loc2lang's no-MDN baseline on the GPU (csrc/grid.hip).

  LatLonGrid            the regular lat/lon grid of loc2lang.py:298-311: np.arange tables, the
                        points lat-major (column i_lat * n_lon + i_lon)
  grid_representation   loc2lang.py:298-322: every coordinate as a sparse row over the grid, an
                        entry 1 / haversine_km for every grid point nearer than radius_km (strict),
                        the row l1-normalised; a float32 sparse.DeviceCSR, canonical

The reference fills a lil_matrix in a Python double loop, one `haversine` call per (sample, grid
point), and pickles the result (grid<N>.pkl); here a wave per coordinate looks at the few dozen
grid cells that can be in range (the bounds: include/gcg_spmm.h), in float64.

Deviations. A sample exactly on a grid point makes the reference divide by zero
(ZeroDivisionError); here the limit is taken: the Z >= 1 coincident columns get 1 / Z and the
row's other in-range columns stay as explicit +0.0 entries, so the structure never depends on the
values. The reference stores 1 / d rounded to float32 and lets sklearn normalise in float32; here
the weights and their sum are float64 and the stored value is rounded once (a few float32 ulps
apart). The `haversine` package's earth radius differs between its versions, so it is an argument
(geo.EARTH_RADIUS_KM by default). The pickle cache is not built.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import sparse as gs
from ._native import call, workspace
from .geo import EARTH_RADIUS_KM, _coords, _ptr, _radius, _stream

# (lllat, lllon, urlat, urlon), loc2lang.py:299-302 and 723-726
US_BBOX = (24.396308, -124.848974, 49.384358, -66.885444)
WORLD_BBOX = (-90.0, -180.0, 90.0, 180.0)

# doubles of LDS the kernel's three tables may take: 2 * n_lat + n_lon (csrc/grid.hip)
MAX_TABLE = 6144


class LatLonGrid:
    """The grid of loc2lang.py:303-311: lats = np.arange(lllat, urlat, grid_size), lons =
    np.arange(lllon, urlon, grid_size); point i_lat * n_lon + i_lon is (lats[i_lat], lons[i_lon]).
    The two tables are the doubles numpy's arange gives -- the kernel reads them, it never
    re-derives a coordinate from a start and a step."""

    def __init__(self, bbox=US_BBOX, grid_size: float = 0.5):
        bbox = tuple(float(x) for x in bbox)
        if len(bbox) != 4 or not all(math.isfinite(x) for x in bbox):
            raise ValueError("bbox must be four finite numbers (lllat, lllon, urlat, urlon)")
        grid_size = float(grid_size)
        if not (math.isfinite(grid_size) and grid_size > 0):
            raise ValueError(f"grid_size must be positive and finite, got {grid_size}")
        lllat, lllon, urlat, urlon = bbox
        # the table bound first: a tiny step must not allocate the arange it asks for
        est = 2 * max(urlat - lllat, 0.0) / grid_size + max(urlon - lllon, 0.0) / grid_size
        if est > MAX_TABLE + 3:
            raise ValueError(f"the grid's tables (2 x latitudes + longitudes = about {est:.0f} "
                             f"entries) exceed the {MAX_TABLE} that the kernel keeps in LDS")
        self.bbox, self.grid_size = bbox, grid_size
        self.lats = np.arange(lllat, urlat, grid_size, dtype=np.float64)
        self.lons = np.arange(lllon, urlon, grid_size, dtype=np.float64)
        if self.lats.size == 0 or self.lons.size == 0:
            raise ValueError(f"the grid is empty: bbox {bbox} holds no point at step {grid_size}")
        if 2 * self.lats.size + self.lons.size > MAX_TABLE:
            raise ValueError(f"the grid's tables (2 x {self.lats.size} latitudes + "
                             f"{self.lons.size} longitudes) exceed the {MAX_TABLE} entries that "
                             "the kernel keeps in LDS")
        self.n_lat, self.n_lon = int(self.lats.size), int(self.lons.size)
        self.n_points = self.n_lat * self.n_lon

    def coords(self) -> np.ndarray:
        """float64 [P, 2]: the grid points, lat-major as the reference's `coords` list."""
        out = np.empty((self.n_points, 2), np.float64)
        out[:, 0] = np.repeat(self.lats, self.n_lon)
        out[:, 1] = np.tile(self.lons, self.n_lat)
        return out

    def __repr__(self):
        return f"LatLonGrid({self.n_lat} x {self.n_lon} points at {self.grid_size} deg)"


def grid_representation(input, grid_size: float = 0.5, bbox=US_BBOX, radius_km: float = 161.0,
                        earth_radius_km: float = EARTH_RADIUS_KM, device="cuda",
                        exhaustive: bool = False) -> gs.DeviceCSR:
    """loc2lang.grid_representation (loc2lang.py:298-322) as a float32 DeviceCSR [n, P], canonical
    (columns strictly ascending in every row), int32 indptr and indices. input: [n, 2] [lat, lon]
    degrees, numpy or tensor, host or device, float32 (widened exactly) or float64.

    Column p is an entry of row i iff d(i, p) < radius_km, d = 2R asin(sqrt(min(a, 1))) in
    float64 (geo.haversine_km's); its value is float32((1/d) / sum of the row's 1/d). A row with
    no grid point in range is empty. exhaustive=True looks at every column instead of the window
    of candidates (the same code path and bitwise the same result; for tests).

    ValueError: a shape other than (n, 2), a non-finite coordinate or |lat| > 90 (found on the
    device; the status comes back with the entry count), grid_size <= 0, an empty grid, radius_km
    outside (0, pi R), earth_radius_km <= 0, 2^31 entries or more."""
    r = _radius(earth_radius_km)
    radius = float(radius_km)
    if not (radius > 0 and radius < math.pi * r):
        raise ValueError(f"radius_km must lie in (0, pi * earth_radius_km), got {radius_km}")
    grid = bbox if isinstance(bbox, LatLonGrid) else LatLonGrid(bbox, grid_size)
    x = _coords(input, device if not (torch.is_tensor(input) and input.is_cuda) else None, "input")
    dev, n, P = x.device, x.shape[0], grid.n_points
    if n == 0:
        return gs.DeviceCSR(torch.zeros(1, dtype=torch.int32, device=dev),
                            torch.zeros(0, dtype=torch.int32, device=dev),
                            torch.zeros(0, dtype=torch.float32, device=dev), (0, P), validate=False)
    lats = torch.from_numpy(grid.lats).to(dev)
    lons = torch.from_numpy(grid.lons).to(dev)
    indptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    norm = torch.empty(n, dtype=torch.float64, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    args = (n, _ptr(x), grid.n_lat, _ptr(lats), grid.n_lon, _ptr(lons), radius, r, int(bool(exhaustive)))
    with torch.cuda.device(dev):
        ws, nbytes = workspace("gcg_grid_count_f64_workspace_bytes", dev, n)
        call("gcg_grid_count_f64", *args, _ptr(indptr), _ptr(norm), _ptr(info), _ptr(ws), nbytes,
             _stream(dev))
        nnz, status = info.tolist()  # the one readback: the entry count, with the input check
        if status != 0:
            raise ValueError("input holds a non-finite coordinate or a latitude outside [-90, 90]")
        if nnz >= 2 ** 31:
            raise ValueError(f"{n} rows over {P} grid points within {radius} km give {nnz} "
                             "entries, 2^31 or more: int32 indptr cannot hold them")
        indices = torch.empty(nnz, dtype=torch.int32, device=dev)
        values = torch.empty(nnz, dtype=torch.float32, device=dev)
        call("gcg_grid_fill_f64", *args, _ptr(indptr), _ptr(norm), nnz, _ptr(indices),
             _ptr(values), _stream(dev))
    return gs.DeviceCSR(indptr, indices, values, (n, P), validate=False)
