"""Float64 numpy restatement of the grid representation of loc2lang's no-MDN baseline
(reference loc2lang.py:298-322), the yardstick of graphconvgeo_amd.grid:

  grid_tables           the grid's np.arange tables and its lat-major points
  distances             the [n, P] float64 haversine distances (geo_reference.haversine_km)
  grid_representation   the canonical float32 CSR: an entry 1/d for every grid point with
                        d < radius_km, the row l1-normalised in float64 and cast once
  reference_loop        the reference's literal double loop, one scalar haversine call per pair
  input_sets            the two fixed input sets of the GPU tests (us_set, world_set)

Where the reference divides by zero (a sample exactly on a grid point) the limit is taken: the
Z >= 1 coincident columns get 1/Z, the row's other in-range columns an explicit +0.0.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sps

from geo_reference import EARTH_RADIUS_KM, haversine_km

US_BBOX = (24.396308, -124.848974, 49.384358, -66.885444)
WORLD_BBOX = (-90.0, -180.0, 90.0, 180.0)


def grid_tables(bbox, grid_size):
    """(lats, lons, coords [P, 2]) of loc2lang.py:303-311."""
    lllat, lllon, urlat, urlon = bbox
    lats = np.arange(lllat, urlat, grid_size)
    lons = np.arange(lllon, urlon, grid_size)
    coords = np.stack([np.repeat(lats, lons.size), np.tile(lons, lats.size)], axis=1)
    return lats, lons, coords


def distances(input, grid_size=0.5, bbox=US_BBOX, earth_radius_km=EARTH_RADIUS_KM):
    x = np.asarray(input, dtype=np.float64)
    coords = grid_tables(bbox, grid_size)[2]
    return haversine_km(x[:, None, :], coords[None, :, :], earth_radius_km)


def grid_representation(input, grid_size=0.5, bbox=US_BBOX, radius_km=161.0,
                        earth_radius_km=EARTH_RADIUS_KM, return_distances=False):
    d = distances(input, grid_size, bbox, earth_radius_km)
    n, P = d.shape
    keep = d < radius_km
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum(keep.sum(axis=1))
    indices = np.nonzero(keep)[1].astype(np.int32)
    data = np.zeros(indices.size, np.float32)
    for i in range(n):
        cols = indices[indptr[i]:indptr[i + 1]]
        di = d[i, cols]
        zero = di == 0.0
        if zero.any():
            v = np.where(zero, 1.0 / zero.sum(), 0.0)
        else:
            w = 1.0 / di
            v = w / w.sum()
        data[indptr[i]:indptr[i + 1]] = v.astype(np.float32)
    out = sps.csr_matrix((data, indices, indptr), shape=(n, P))
    return (out, d) if return_distances else out


def scalar_haversine(p1, p2, earth_radius_km=EARTH_RADIUS_KM):
    """The `haversine` package's function, one pair at a time, with math's scalar functions."""
    lat1, lng1, lat2, lng2 = (math.radians(float(v)) for v in (*p1, *p2))
    lat, lng = lat2 - lat1, lng2 - lng1
    d = math.sin(lat * 0.5) ** 2 + math.cos(lat1) * math.cos(lat2) * math.sin(lng * 0.5) ** 2
    return 2 * earth_radius_km * math.asin(math.sqrt(d))


def reference_loop(input, grid_size, bbox, radius_km=161.0, earth_radius_km=EARTH_RADIUS_KM):
    """loc2lang.py:312-322 as written: a lil_matrix filled pair by pair, then l1-normalised --
    except that the weights stay float64 until the one cast (the reference's lil_matrix is
    float32) and a zero distance takes the limit."""
    x = np.asarray(input, dtype=np.float64)
    coords = grid_tables(bbox, grid_size)[2]
    out = sps.lil_matrix((x.shape[0], coords.shape[0]), dtype=np.float64)
    zero_rows = {}
    for i in range(x.shape[0]):
        for j in range(coords.shape[0]):
            dist = scalar_haversine(x[i], coords[j], earth_radius_km)
            if dist < radius_km:
                if dist == 0.0:
                    zero_rows.setdefault(i, []).append(j)
                    out[i, j] = 1.0
                else:
                    out[i, j] = 1.0 / dist
    dense = out.toarray()
    mask = dense != 0
    for i, cols in zero_rows.items():
        dense[i] = 0.0
        dense[i, cols] = 1.0
    s = dense.sum(axis=1, keepdims=True)
    dense = np.divide(dense, s, out=np.zeros_like(dense), where=s != 0)
    return dense.astype(np.float32), mask


SPECIAL_WORLD = np.array([
    [90, 0], [89.9, 77], [-89.5, -179.9], [0, 179.95], [10, -179.95], [45, 180], [0, 0],
    [88, -180], [-88.7, 179], [30.3, 179.2], [-60.1, -179.4], [86.2, 10], [-87.1, -20], [2, 4],
    [-88, -180], [44, 179], [-89.99, 50]], dtype=np.float64)


def input_sets():
    """(US set, world set), both drawn from one np.random.default_rng(77), latitudes before
    longitudes, the US set first.

    US: 257 rows -- 250 points over the US box widened by 3 degrees, then grid points 0, P - 1
    and 1234, the box's corners with [60, -100] and [37, -200] between them; the whole array
    float32-representable. World: 257 rows -- 240 points uniform in latitude and longitude, then
    SPECIAL_WORLD, in float64."""
    rng = np.random.default_rng(77)
    lllat, lllon, urlat, urlon = US_BBOX
    lat = rng.uniform(lllat - 3, urlat + 3, 250)
    lon = rng.uniform(lllon - 3, urlon + 3, 250)
    coords = grid_tables(US_BBOX, 0.5)[2]
    extra = np.array([coords[0], coords[-1], coords[1234], [lllat, lllon], [60, -100], [37, -200],
                      [urlat, urlon]])
    us = np.concatenate([np.stack([lat, lon], axis=1), extra]).astype(np.float32).astype(np.float64)
    lat = rng.uniform(-90, 90, 240)
    lon = rng.uniform(-180, 180, 240)
    world = np.concatenate([np.stack([lat, lon], axis=1), SPECIAL_WORLD])
    return us, world


def us_set():
    return input_sets()[0]


def world_set():
    return input_sets()[1]


def fairness(x, d, radius_km, bbox, grid_size):
    """The figures that make a device comparison fair: (smallest |d - radius|, smallest positive
    d, zero distances that are not bitwise-coincident coordinates, samples at a pole whose
    latitude is a grid row)."""
    lats, _lons, coords = grid_tables(bbox, grid_size)
    zi, zj = np.nonzero(d == 0.0)
    not_coincident = int(sum(not np.array_equal(x[i], coords[j]) for i, j in zip(zi, zj)))
    pole = int(sum(abs(la) == 90.0 and (lats == la).any() for la in x[:, 0]))
    return float(np.abs(d - radius_km).min()), float(d[d > 0].min()), not_coincident, pole


def ulp_distance(a, b) -> np.ndarray:
    """Distance in float32 ulps between two float32 arrays of non-negative values."""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)
