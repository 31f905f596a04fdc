"""Dropout without a GPU: the NumPy statement of the mask rule (Philox4x32-10 known answers,
keep counts, independence of steps and streams), construction, and the host-side argument
checks of the three entry points."""
import ctypes as C

import numpy as np
import pytest

from graphconvgeo_amd.dropout import (dropout_scale, dropout_threshold, keep_mask_reference,
                                      philox4x32_10)

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert tuple(int(x) for x in got) == want
    # the array forms: four broadcast words, and one [..., 4] array
    many = philox4x32_10(tuple(np.full((2, 3), c, dtype=np.uint32) for c in counter), key)
    assert many.shape == (2, 3, 4) and all(tuple(int(x) for x in r) == want for r in many[0])
    assert np.array_equal(philox4x32_10(np.array([counter, counter], dtype=np.uint32), key),
                          np.array([want, want], dtype=np.uint32))


def _mask(shape, p, seed, step, stream):
    M, K = shape
    return keep_mask_reference(np.arange(M)[:, None], np.arange(K)[None, :], p, seed, step, stream)


@pytest.mark.parametrize("shape", [(65, 301), (130, 1024), (7, 300)])
@pytest.mark.parametrize("p", [0.4, 0.5, 0.6])
@pytest.mark.parametrize("sss", [(77, 0, 1), (77, 1, 1), (77, 0, 0), (2 ** 40 + 5, 3, 1)])
def test_keep_count_within_four_sigma(shape, p, sss):
    n = shape[0] * shape[1]
    kept = int(_mask(shape, p, *sss).sum())
    assert abs(kept - n * (1 - p)) <= 4 * np.sqrt(n * p * (1 - p)), (kept, n, p)


def test_masks_of_steps_and_streams_differ():
    base = _mask((65, 301), 0.5, 77, 0, 1)
    for other in (_mask((65, 301), 0.5, 77, 1, 1), _mask((65, 301), 0.5, 77, 0, 0)):
        frac = float((base != other).mean())
        assert 0.45 <= frac <= 0.55, frac
    assert np.array_equal(base, _mask((65, 301), 0.5, 77, 0, 1))  # a pure function
    # the high key word matters: seeds that agree in their low 32 bits differ
    assert (base != _mask((65, 301), 0.5, 77 + 2 ** 32, 0, 1)).any()


def test_threshold_and_scale():
    assert dropout_threshold(0.0) == 0 and dropout_threshold(0.5) == 2 ** 31
    assert dropout_threshold(0.999) == int(np.floor(0.999 * 2.0 ** 32))
    assert dropout_scale(0.5) == 2.0 and dropout_scale(0.5, rescale=False) == 1.0
    assert dropout_scale(0.6) == float(np.float32(1.0 / (1.0 - 0.6)))
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            dropout_threshold(bad)
    assert _mask((5, 9), 0.0, 1, 0, 0).all()
    # a row slice and a column offset see the coordinates, not their position in the block
    full = _mask((40, 50), 0.5, 9, 2, 3)
    part = keep_mask_reference(np.arange(10, 20)[:, None], np.arange(7, 31)[None, :], 0.5, 9, 2, 3)
    assert np.array_equal(full[10:20, 7:31], part)


def test_construction():
    from graphconvgeo_amd.dist_train import RowPartitionedMLPCONV
    from graphconvgeo_amd.mlpconv import MLPCONV

    clf = MLPCONV(drop_out=True, hidden_layer_size=8)
    assert clf.drop_out and clf.dropout_coefs == [0.5, 0.5]
    assert MLPCONV(hidden_layer_size=8).drop_out is False
    with pytest.raises(ValueError):
        MLPCONV(drop_out=True, dropout_coefs=[1.0, 0.5], hidden_layer_size=8)
    with pytest.raises(NotImplementedError, match="row-partitioned"):
        RowPartitionedMLPCONV(drop_out=True)


def test_layer_names_and_input_check():
    from graphconvgeo_amd import dropout as D

    assert D.dropout is D.DropoutLayer
    layer = D.SparseInputDropoutLayer(p=0.5, stream=D.DropoutStream(3, 0, "cpu"), device="cpu")
    with pytest.raises(ValueError, match="Input for this layer must be sparse"):
        layer.forward(np.zeros((3, 3), np.float32))
    import scipy.sparse as sps
    X = sps.identity(3, format="csr", dtype=np.float32)
    assert layer.forward(X, deterministic=True) is X  # returned as is, nothing launched
    assert D.SparseInputDropoutLayer(p=0.0, stream=layer.stream, device="cpu").forward(X) is X


def test_dropout_seed_draw_order():
    """Lasagne's DropoutLayer draws randint(1, 2147462579) from the weights' stream."""
    from graphconvgeo_amd.dropout import draw_seed

    rs = np.random.RandomState(77)
    want = np.random.RandomState(77).randint(1, 2147462579)
    assert draw_seed(rs) == want
    np.random.seed(77)
    assert draw_seed() == want


A16, B16, W16, S16, I16 = (C.c_void_p(x) for x in (0x10000, 0x20000, 0x40000, 0x50000, 0x60000))
THR, SCALE, SEED = C.c_uint32(1 << 31), C.c_float(2.0), C.c_uint64(77)


def test_dropout_abi_without_gpu(native_lib):
    f = native_lib.gcg_dropout_f32
    tail = (THR, SCALE, SEED, S16, 1, 0, None, None)
    assert f(8, 4, None, 4, B16, 4, *tail) == 1                       # null X
    assert f(8, 4, A16, 4, None, 4, *tail) == 1                       # null Y
    assert f(8, 4, A16, 4, B16, 4, THR, SCALE, SEED, None, 1, 0, None, None) == 1  # null step
    assert f(8, 4, A16, 3, B16, 4, *tail) == 1                        # ldx < K
    assert f(8, 4, A16, 4, B16, 3, *tail) == 1                        # ldy < K
    assert f(-1, 4, A16, 4, B16, 4, *tail) == 1                       # negative M
    assert f(8, -1, A16, 4, B16, 4, *tail) == 1                       # negative K
    assert f(8, 4, A16, 4, B16, 4, THR, SCALE, SEED, S16, 1, -1, None, None) == 1  # row0 < 0
    assert f(8, 4, C.c_void_p(0x10002), 4, B16, 4, *tail) == 2        # misaligned
    assert f(0, 4, None, 4, None, 4, *tail) == 0                      # M == 0
    assert f(8, 0, None, 0, None, 0, *tail) == 0                      # K == 0


def test_dropout_relu_backward_abi_without_gpu(native_lib):
    f = native_lib.gcg_dropout_relu_backward_f32
    tail = (THR, SCALE, SEED, S16, 1, 0, None)
    ws = (W16, 1 << 20)
    assert f(8, 4, None, 4, None, 0, B16, 4, None, *ws, *tail) == 1           # null gY
    assert f(8, 4, A16, 4, None, 0, None, 4, None, *ws, *tail) == 1           # null g_out
    assert f(8, 4, A16, 4, None, 0, B16, 4, None, *ws, THR, SCALE, SEED, None, 1, 0, None) == 1
    assert f(8, 4, A16, 3, None, 0, B16, 4, None, *ws, *tail) == 1            # ldg < K
    assert f(8, 4, A16, 4, None, 0, B16, 3, None, *ws, *tail) == 1            # ldo < K
    assert f(8, 1025, A16, 1028, None, 0, B16, 1028, None, W16, 1 << 22, *tail) == 1  # K cap
    assert f(-1, 4, A16, 4, None, 0, B16, 4, None, *ws, *tail) == 1           # negative M
    assert f(8, -2, A16, 4, None, 0, B16, 4, None, *ws, *tail) == 1           # negative K
    assert f(8, 4, A16, 4, None, 0, B16, 4, None, None, 0, *tail) == 6        # no workspace
    assert f(8, 4, A16, 4, None, 0, B16, 4, None, W16, 4, *tail) == 6         # short workspace
    assert f(8, 4, A16, 4, I16, 3, B16, 4, None, *ws, *tail) == 2             # ldgate < K
    assert f(8, 300, A16, 301, None, 0, B16, 304, None, *ws, *tail) == 2      # wide: 16-B rows
    assert f(0, 4, None, 4, None, 0, None, 4, None, None, 0, *tail) == 0      # M == 0
    assert f(8, 0, None, 0, None, 0, None, 0, None, None, 0, *tail) == 0      # K == 0


def test_csr_dropout_abi_without_gpu(native_lib):
    f = native_lib.gcg_csr_dropout_f32
    tail = (THR, SCALE, SEED, S16, 1, None)
    assert f(4, 4, 8, None, I16, A16, B16, 0, *tail) == 1      # null indptr
    assert f(4, 4, 8, S16, None, A16, B16, 0, *tail) == 1      # null indices
    assert f(4, 4, 8, S16, I16, None, B16, 0, *tail) == 1      # null vals
    assert f(4, 4, 8, S16, I16, A16, None, 0, *tail) == 1      # null vals_out
    assert f(4, 4, 8, S16, I16, A16, B16, 0, THR, SCALE, SEED, None, 1, None) == 1  # null step
    assert f(-1, 4, 8, S16, I16, A16, B16, 0, *tail) == 1      # negative sizes
    assert f(4, -1, 8, S16, I16, A16, B16, 0, *tail) == 1
    assert f(4, 4, -1, S16, I16, A16, B16, 0, *tail) == 1
    assert f(4, 4, 8, S16, I16, A16, B16, 2, *tail) == 1       # transposed is 0 or 1
    assert f(0, 4, 8, S16, I16, A16, B16, 0, *tail) == 1       # entries without rows
    assert f(4, 4, 0, None, None, None, None, 0, *tail) == 0   # nnz == 0
    assert f(0, 0, 0, None, None, None, None, 1, *tail) == 0
