"""The geolocation entries of the C-ABI (csrc/geo.hip): argument checks that run on the host
before any launch, and a plain C caller on the GPU (tests/c/geo_gpu_consumer.c)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO_ENTRIES = ("gcg_kdtree_fit_f64", "gcg_segment_medians_f64", "gcg_class_medians_f64",
               "gcg_haversine_km_f64", "gcg_nearest_class_f64", "gcg_geo_eval_f64")


def test_geo_entries_are_declared_bound_and_built():
    from graphconvgeo_amd import _build, _native
    header = open(os.path.join(ROOT, "include", "gcg_spmm.h")).read()
    for name in GEO_ENTRIES:
        assert name + "(" in header and name in _native.SIGNATURES
    assert any(os.path.basename(s) == "geo.hip" for s in _build.SOURCES)


def test_geo_abi_argument_validation_without_gpu(native_lib):
    lib = native_lib
    a8, b8, c8, d8 = (C.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000))
    odd = C.c_void_p(0x10004)
    nc, depth, rb = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    out = (C.byref(nc), C.byref(depth), C.byref(rb))
    fit = lib.gcg_kdtree_fit_f64
    assert fit(5, a8, 0, b8, b8, b8, b8, *out, c8, None) == 1          # bucket_size < 1
    assert b"bucket_size" in lib.gcg_last_error()
    assert fit(-1, a8, 2, b8, b8, b8, b8, *out, c8, None) == 1         # N < 0
    assert fit(5, a8, 2, b8, b8, b8, b8, None, None, None, c8, None) == 1  # no n_clusters_host
    assert fit(5, None, 2, b8, b8, b8, b8, *out, c8, None) == 1        # null locs
    assert nc.value == 0 and depth.value == 0 and rb.value == 0
    assert fit(5, odd, 2, b8, b8, b8, b8, *out, c8, None) == 2         # locs not 8-B aligned
    hav = lib.gcg_haversine_km_f64
    assert hav(-1, a8, b8, 6371.0, c8, None) == 1
    assert hav(4, a8, b8, 0.0, c8, None) == 1                          # radius
    assert hav(4, a8, b8, float("nan"), c8, None) == 1
    assert hav(4, None, b8, 6371.0, c8, None) == 1
    assert hav(4, odd, b8, 6371.0, c8, None) == 2
    assert hav(0, None, None, 6371.0, None, None) == 0                 # M = 0: no-op
    near = lib.gcg_nearest_class_f64
    assert near(4, a8, 0, b8, 6371.0, c8, None, None) == 1             # no class
    assert near(4, a8, 3, None, 6371.0, c8, None, None) == 1
    assert near(4, a8, 3, b8, 6371.0, c8, odd, None) == 2              # distance misaligned
    assert near(0, None, 0, None, 6371.0, None, None, None) == 0
    ev = lib.gcg_geo_eval_f64
    assert ev(4, a8, 2, b8, 3, c8, 6371.0, 161.0, d8, a8, b8, None) == 1   # pred_is_int64
    assert ev(4, a8, 1, b8, 3, c8, 6371.0, 161.0, d8, None, b8, None) == 1  # no count_dev
    assert ev(4, a8, 1, b8, 3, c8, -1.0, 161.0, d8, a8, b8, None) == 1
    assert lib.gcg_segment_medians_f64(-1, 4, a8, b8, b8, b8, c8, None) == 1
    assert lib.gcg_segment_medians_f64(0, 4, a8, b8, b8, b8, c8, None) == 0
    assert lib.gcg_class_medians_f64(4, a8, b8, 3, c8, None, None) == 1    # no status_dev
    assert lib.gcg_class_medians_f64(-1, a8, b8, 3, c8, d8, None) == 1


@pytest.mark.gpu
def test_geo_c_caller_on_gpu(cuda, tmp_path):
    from graphconvgeo_amd import _native
    lib = _native.lib_path()
    exe = tmp_path / "geo_gpu_consumer"
    src = os.path.join(ROOT, "tests", "c", "geo_gpu_consumer.c")
    subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"), src, lib,
                    "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath,/opt/rocm/lib",
                    f"-Wl,-rpath,{os.path.dirname(lib)}", "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
    assert "geo abi ok" in res.stdout
