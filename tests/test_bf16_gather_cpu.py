"""CPU checks of the bf16-gather mode: the row-stride rule, the C-ABI surface and the float64
reference restatement the GPU trajectory test is measured against."""
import os
import re

import numpy as np

import bf16_gather_reference as R
from oracle import gcn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gcg_rows_f32_to_bf16", "gcg_spmm_csr_bf16z_f32", "gcg_spmm_csr_bf16z_f32_planned")


def test_row_stride_bf16_properties():
    from graphconvgeo_amd.sparse import row_stride_bf16
    for k in range(1, 2049):
        ld = row_stride_bf16(k)
        assert ld % 8 == 0 and ld >= k and ld - k <= 63, (k, ld)
    assert row_stride_bf16(8) == 8 and row_stride_bf16(512) == 512  # no padding where none helps
    # every k = 300 row (600 B) on exactly five 128-B lines
    ld = row_stride_bf16(300)
    assert {(2 * ld * r % 128 + 600 + 127) // 128 for r in range(64)} == {5}


def test_new_symbols_declared_and_exported(native_lib):
    from graphconvgeo_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gcg_spmm.h")).read(),
                  flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bgcg_status\s+%s\s*\(" % name, text), name
        assert hasattr(native_lib, name) and name in _native.SIGNATURES
    # argument checks come before any device access: bad shape / misalignment without a GPU
    assert native_lib.gcg_rows_f32_to_bf16(4, 8, 16, 4, 16, 8, None) == 1  # lds < K
    assert native_lib.gcg_rows_f32_to_bf16(4, 8, 18, 8, 16, 8, None) == 2  # src not 4-B aligned
    assert native_lib.gcg_spmm_csr_bf16z_f32(4, 4, 0, 16, None, None, 16, 4, 8, 16, 8, None, 0,
                                             None, 4, None, 0, None) == 1  # ldz < K
    assert native_lib.gcg_spmm_csr_bf16z_f32(4, 4, 0, 16, None, None, 17, 8, 8, 16, 8, None, 0,
                                             None, 4, None, 0, None) == 2  # Zb not 2-B aligned


def test_reference_without_rounding_is_the_oracle():
    from graphconvgeo_amd.synth import glorot_uniform, synthetic_features, synthetic_graph
    n, f, k, c = 600, 80, 12, 4
    H = synthetic_graph(n, 3000)
    X = synthetic_features(n, f, nnz_per_row=8, empty_frac=0.02)
    Y = np.random.default_rng(0).integers(0, c, size=n)
    train = np.random.default_rng(1).choice(400, size=400).astype(np.int32)
    dev = np.arange(400, 500, dtype=np.int32)
    init = (glorot_uniform(f, k), np.zeros(k, np.float32), glorot_uniform(k, c, seed=3),
            np.zeros(c, np.float32))
    want, pw = O.mlpconv_train(X, H, Y, train, dev, *init, n_epochs=6, regul_coefs=(1e-5, 1e-5),
                               report_k_epoch=2)
    got, pg = R.mlpconv_train(X, H, Y, train, dev, *init, n_epochs=6, regul_coefs=(1e-5, 1e-5),
                              report_k_epoch=2)
    for a, b in zip(got, want):
        assert a.keys() == b.keys()
        for key in a:
            assert abs(a[key] - b[key]) <= 1e-12, (key, a, b)
    for key in pw:
        assert np.abs(pg[key] - pw[key]).max() <= 1e-12
    rounded, _ = R.mlpconv_train(X, H, Y, train, dev, *init, n_epochs=6, regul_coefs=(1e-5, 1e-5),
                                 report_k_epoch=2, round_operand=R.bf16r)
    d = max(abs(a["train_loss"] - b["train_loss"]) for a, b in zip(rounded, want))
    assert 0 < d < 1e-3  # the rounding moves the trajectory, slightly
    x = np.array([1.00390625, 1.01171875], dtype=np.float64)  # ties: to even, down and up
    assert np.array_equal(R.bf16r(x), [1.0, 1.015625]) and R.bf16r(x).dtype == np.float64
