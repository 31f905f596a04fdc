"""Geolocation labels and metrics on the GPU (csrc/geo.hip).

  KDTreeClustering   kdtree.KDTreeClustering (kdtree.py:121-151): the k-d-tree region labels
  class_medians      the per-class medians of DataLoader.assignClasses (data.py:408-413)
  haversine_km       the `haversine` package's distance, row-wise
  nearest_class      the brute-force 1-NN over the medians (data.py:416-419)
  assign_classes     DataLoader.assignClasses in one call (without the one-hot branch)
  geo_eval           tensormain.geo_eval (tensormain.py:38-54): mean, median, Acc@161

Coordinates are (N, 2) [latitude, longitude] in degrees, numpy arrays or tensors; float32 is
widened to float64 on the device and every result is float64. Labels and indices are int32
device tensors. The reference's `haversine` package is unpinned and its earth radius differs
between versions (6371 / 6371.0088 km), so the radius is an argument everywhere.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._native import NativeError, call

EARTH_RADIUS_KM = 6371.0088


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else None


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _coords(locs, device=None, name="locs") -> torch.Tensor:
    """(N, 2) float64 contiguous device tensor of `locs` (float32 is widened on the device)."""
    if not torch.is_tensor(locs):
        a = np.asarray(locs)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        locs = torch.from_numpy(np.ascontiguousarray(a))
    if locs.dim() != 2 or locs.shape[1] != 2:
        raise ValueError(f"{name} must have shape (N, 2) [lat, lon], got {tuple(locs.shape)}")
    if locs.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be float32 or float64, got {locs.dtype}")
    if device is None:
        device = locs.device if locs.is_cuda else "cuda"
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the geolocation kernels run on the GPU: device must be a CUDA (HIP) device")
    return locs.to(dev).to(torch.float64).contiguous()


def _radius(earth_radius_km) -> float:
    r = float(earth_radius_km)
    if not (np.isfinite(r) and r > 0):
        raise ValueError(f"earth_radius_km must be positive and finite, got {earth_radius_km}")
    return r


class KDTreeClustering:
    """kdtree.KDTreeClustering on the GPU. After fit: `clusters` (int32 device tensor, the
    reference's labels exactly), `num_clusters`, `medians` ((C, 2) float64: the per-class medians
    of assignClasses, read off the tree's sorted lists), `depth` (levels on which a node split)
    and `readbacks` (stream synchronizations of the build: depth + 2)."""

    def __init__(self, bucket_size: int = 10):
        self.bucket_size = bucket_size
        self.is_fitted = False

    def fit(self, locs, device=None):
        if int(self.bucket_size) != self.bucket_size or int(self.bucket_size) < 1:
            raise ValueError(f"bucket_size must be an integer >= 1, got {self.bucket_size}")
        x = _coords(locs, device)
        dev, n = x.device, x.shape[0]
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        perm_lat = torch.empty(n, dtype=torch.int32, device=dev)
        perm_lon = torch.empty(n, dtype=torch.int32, device=dev)
        leaf_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        nc, depth, rb = C.c_int64(), C.c_int64(), C.c_int64()
        with torch.cuda.device(dev):
            stream = _stream(dev)
            try:
                call("gcg_kdtree_fit_f64", n, _ptr(x), int(self.bucket_size), _ptr(labels),
                     _ptr(perm_lat), _ptr(perm_lon), _ptr(leaf_ptr), C.byref(nc), C.byref(depth),
                     C.byref(rb), _ptr(status), stream)
            except NativeError as e:
                if "non-finite" in str(e):
                    raise ValueError("locs holds a non-finite coordinate") from None
                raise
            medians = torch.empty((nc.value, 2), dtype=torch.float64, device=dev)
            call("gcg_segment_medians_f64", nc.value, n, _ptr(x), _ptr(leaf_ptr), _ptr(perm_lat),
                 _ptr(perm_lon), _ptr(medians), stream)
        self.clusters = labels
        self.num_clusters = int(nc.value)
        self.medians = medians
        self.depth = int(depth.value)
        self.readbacks = int(rb.value)
        self.is_fitted = True
        return self

    def get_clusters(self):
        if self.is_fitted:
            return self.clusters


def class_medians(locs, labels, num_classes: int, device=None) -> torch.Tensor:
    """(num_classes, 2) float64: np.median of the latitudes and of the longitudes of every class
    (bitwise numpy's); NaN for a class without points."""
    x = _coords(locs, device)
    dev, n = x.device, x.shape[0]
    num_classes = int(num_classes)
    if num_classes < 0:
        raise ValueError("num_classes must be >= 0")
    lab = torch.as_tensor(labels).to(dev)
    if lab.dim() != 1 or lab.shape[0] != n:
        raise ValueError(f"labels must have shape ({n},), got {tuple(lab.shape)}")
    if lab.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"labels must be int32 or int64, got {lab.dtype}")
    if n > 0 and num_classes == 0:
        raise ValueError("points but num_classes = 0")
    lab = lab.to(torch.int32).contiguous()
    medians = torch.empty((num_classes, 2), dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("gcg_class_medians_f64", n, _ptr(x), _ptr(lab), num_classes, _ptr(medians),
             _ptr(status), _stream(dev))
    if int(status.item()) != 0:
        raise ValueError("a label outside [0, num_classes) or a non-finite coordinate")
    return medians


def haversine_km(a, b, earth_radius_km: float = EARTH_RADIUS_KM, device=None) -> torch.Tensor:
    """Row-wise great-circle distance in km between a[i] and b[i] ((M, 2) degrees)."""
    r = _radius(earth_radius_km)
    ta = _coords(a, device, "a")
    tb = _coords(b, ta.device, "b")
    if ta.shape != tb.shape:
        raise ValueError(f"a and b must have the same shape, got {tuple(ta.shape)} and {tuple(tb.shape)}")
    out = torch.empty(ta.shape[0], dtype=torch.float64, device=ta.device)
    with torch.cuda.device(ta.device):
        call("gcg_haversine_km_f64", ta.shape[0], _ptr(ta), _ptr(tb), r, _ptr(out), _stream(ta.device))
    return out


def nearest_class(locs, medians, earth_radius_km: float = EARTH_RADIUS_KM,
                  return_distance: bool = False, device=None):
    """int32 (M,) index of the nearest median by haversine distance, the first on ties (and its
    distance with return_distance=True)."""
    r = _radius(earth_radius_km)
    x = _coords(locs, device)
    med = _coords(medians, x.device, "medians")
    m, c = x.shape[0], med.shape[0]
    if m > 0 and c == 0:
        raise ValueError("no class to choose from")
    idx = torch.empty(m, dtype=torch.int32, device=x.device)
    dist = torch.empty(m, dtype=torch.float64, device=x.device) if return_distance else None
    with torch.cuda.device(x.device):
        call("gcg_nearest_class_f64", m, _ptr(x), c, _ptr(med), r, _ptr(idx), _ptr(dist),
             _stream(x.device))
    return (idx, dist) if return_distance else idx


def geo_eval(pred, locs, medians, earth_radius_km: float = EARTH_RADIUS_KM,
             threshold_km: float = 161.0, return_distances: bool = False, device=None):
    """(mean km, median km, acc_at_161) of tensormain.geo_eval: the distance from every true
    location to the median of its predicted class; Acc@161 = 100 * count(d < threshold) / M.
    `pred` may be a device tensor (int32 or int64) and stays on the device; one host copy of
    the four result scalars ends the call."""
    r = _radius(earth_radius_km)
    x = _coords(locs, device)
    dev, m = x.device, x.shape[0]
    med = _coords(medians, dev, "medians")
    p = torch.as_tensor(pred).to(dev)
    if p.dim() != 1 or p.shape[0] != m:
        raise ValueError(f"pred must have shape ({m},), got {tuple(p.shape)}")
    if m == 0:
        raise ValueError("geo_eval of no rows")
    if p.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"pred must be int32 or int64, got {p.dtype}")
    p = p.contiguous()
    dist = torch.empty(m, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("gcg_geo_eval_f64", m, _ptr(p), int(p.dtype == torch.int64), _ptr(x), med.shape[0],
             _ptr(med), r, float(threshold_km), _ptr(dist), _ptr(count), _ptr(status), _stream(dev))
    srt = torch.sort(dist).values
    median = (srt[(m - 1) // 2] + srt[m // 2]) / 2 if m % 2 == 0 else srt[m // 2]
    mean, median, cnt, st = torch.stack(
        [dist.mean(), median, count[0].to(torch.float64), status[0].to(torch.float64)]).tolist()
    if st != 0:
        raise ValueError(f"a prediction outside [0, {med.shape[0]})")
    out = (mean, median, 100 * int(cnt) / float(m))
    return (*out, dist) if return_distances else out


def assign_classes(train_locs, dev_locs, test_locs, bucket_size: int,
                   earth_radius_km: float = EARTH_RADIUS_KM, device=None):
    """DataLoader.assignClasses (data.py:399-421): (train, dev, test labels, medians). The train
    labels are the k-d-tree regions of the training coordinates; a dev / test user gets the
    class whose median is nearest by haversine distance."""
    tree = KDTreeClustering(bucket_size).fit(train_locs, device)
    dev_ = tree.clusters.device
    dev_lab = nearest_class(dev_locs, tree.medians, earth_radius_km, device=dev_)
    test_lab = nearest_class(test_locs, tree.medians, earth_radius_km, device=dev_)
    return tree.clusters, dev_lab, test_lab, tree.medians
