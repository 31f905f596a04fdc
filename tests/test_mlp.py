"""CPU tests of the mini-batch MLP trainer (graphconvgeo_amd.mlp, reference mlp.py:96-311): batch
iteration, size rules, every refusal, and host-side argument validation of the new C-ABI
entries (no GPU compute here)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import mlp_reference as R
from graphconvgeo_amd import mlp as M


@pytest.mark.parametrize("n,B", [(1300, 400), (1200, 400), (400, 400), (257, 64), (5, 1)])
def test_batch_count_and_dropped_tail(n, B):
    np.random.seed(11)
    batches = M.iterate_minibatch_indices(n, B)
    assert len(batches) == (n - B) // B + 1 == M.n_batches(n, B)
    assert all(len(b) == B for b in batches)
    used = np.concatenate(batches)
    assert used.size == len(set(used.tolist())) == (n // B) * B  # the tail is dropped
    order = np.arange(n)
    np.random.RandomState(11).shuffle(order)
    assert np.array_equal(used, order[:used.size])  # the global stream's shuffle
    assert [b.tolist() for b in R.batches_of(order, B)] == [b.tolist() for b in batches]


def test_epoch_orders_follow_the_global_stream():
    """Successive epochs draw successive shuffles of arange(n) from np.random (mlp.py:84-85)."""
    np.random.seed(5)
    got = [np.concatenate(M.iterate_minibatch_indices(10, 5)) for _ in range(3)]
    rs = np.random.RandomState(5)
    for g in got:
        o = np.arange(10)
        rs.shuffle(o)
        assert np.array_equal(g, o)


def test_fewer_rows_than_a_batch_raises():
    with pytest.raises(ValueError, match="fewer than one batch"):
        M.n_batches(399, 400)
    with pytest.raises(ValueError):
        M.n_batches(10, 0)


def test_out_size_is_the_number_of_distinct_labels():
    assert M.output_size(np.array([0, 5, 5, 2])) == 3  # len(set(.)), not max + 1 (mlp.py:132)
    assert M.output_size(np.array([3, 3, 3])) == 1


def test_hidden_size_rule():
    assert M.default_hidden_size(9, 300) == 15       # in_size // 20
    assert M.default_hidden_size(9, 10_000) == 45    # 5 * out_size
    assert M.default_hidden_size(129, 9_467) == 473  # int(9467 / 20)


def test_constructor_defaults_are_the_references():
    clf = M.MLP()
    assert (clf.n_epochs, clf.batch_size, clf.add_hidden, clf.regul_coefs) == \
        (10, 1000, True, [5e-5, 5e-5])
    assert clf.drop_out_coefs == [0.5, 0.5] and clf.early_stopping_max_down == 100000
    assert clf.hidden_layer_size is None and clf.init_parameters is None


@pytest.mark.parametrize("kw", [{"complete_prob": True}, {"drop_out": True},
                                {"loss_name": "hinge"}])
def test_unbuilt_options_raise(kw):
    with pytest.raises(NotImplementedError):
        M.MLP(**kw)


def _xy(n=12, f=40):
    X = sps.random(n, f, density=0.2, format="csr", dtype=np.float32, random_state=0)
    return X, np.arange(n) % 3


def test_dense_input_raises():
    X, Y = _xy()
    with pytest.raises(ValueError, match="Input for this layer must be sparse"):
        M.MLP(batch_size=4, device="cpu").fit(X.toarray(), Y, X, Y)
    with pytest.raises(ValueError, match="Input for this layer must be sparse"):
        M.MLP(batch_size=4, device="cpu").fit(X, Y, X.toarray(), Y)
    with pytest.raises(ValueError, match="Input for this layer must be sparse"):
        M.input_convolution(np.eye(3), np.eye(3), device="cpu")


def test_label_beyond_out_size_raises():
    X, Y = _xy()
    bad = Y.copy()
    bad[0] = 7  # 4 distinct labels {0, 1, 2, 7}: out_size 4, label 7 has no output unit
    with pytest.raises(ValueError, match="outside"):
        M.MLP(batch_size=4, device="cpu").fit(X, bad, X, Y)
    dev = Y.copy()
    dev[1] = 3  # a dev label the training set never had
    with pytest.raises(ValueError, match="Y_dev"):
        M.MLP(batch_size=4, device="cpu").fit(X, Y, X, dev)


def test_training_set_smaller_than_a_batch_raises():
    X, Y = _xy()
    with pytest.raises(ValueError, match="fewer than one batch"):
        M.MLP(batch_size=13, device="cpu").fit(X, Y, X, Y)


def test_package_exports():
    import graphconvgeo_amd as g
    assert g.MLP is M.MLP and g.input_convolution is M.input_convolution
    assert hasattr(g.DeviceCSR, "row_slice")


# -- C-ABI: host-side validation -------------------------------------------------------------
OK, INVAL, MISALIGNED, WORKSPACE = 0, 1, 2, 6


def test_segment_sizes_and_argument_validation_without_gpu(native_lib):
    lib = native_lib
    cap = C.c_int64()
    # seg_capacity is host arithmetic: min(nnz_sel, n_batches * n_cols) + 1
    assert lib.gcg_minibatch_segment_sizes(256, 64, 97, 1500, C.byref(cap), None) == OK
    assert cap.value == 4 * 97 + 1
    assert lib.gcg_minibatch_segment_sizes(256, 64, 97, 100, C.byref(cap), None) == OK
    assert cap.value == 101
    assert lib.gcg_minibatch_segment_sizes(0, 64, 97, 0, C.byref(cap), None) == OK
    assert cap.value == 1
    sizes = lib.gcg_minibatch_segment_sizes
    assert sizes(-64, 64, 97, 10, C.byref(cap), None) == INVAL
    assert sizes(255, 64, 97, 10, C.byref(cap), None) == INVAL      # not whole batches
    assert sizes(256, 0, 97, 10, C.byref(cap), None) == INVAL
    assert sizes(256, 64, 0, 10, C.byref(cap), None) == INVAL
    assert sizes(256, 64, 97, -1, C.byref(cap), None) == INVAL
    # 100,000 batches x 97,000 columns: the (batch, column) key does not fit 32 bits
    assert sizes(64 * 100_000, 64, 97_000, 10, C.byref(cap), None) == INVAL
    assert "32-bit" in lib.gcg_last_error().decode()
    assert sizes(64 * 1000, 64, 97_000, 10, C.byref(cap), None) == OK  # 9.7e7 keys fit

    a = C.c_void_p(0x10000)
    seg = lib.gcg_minibatch_segment
    args = (256, 64, 1500, a, a, a, a, a)  # n_sel, batch, nnz_sel, the five outputs
    assert seg(300, 97, a, a, a, a, *args, None, 0, None) == WORKSPACE
    assert seg(300, 97, a, a, a, a, *args, a, 64, None) == WORKSPACE          # short
    assert seg(300, 97, None, a, a, a, *args, a, 1 << 30, None) == INVAL      # NULL indptr
    assert seg(300, 97, a, a, a, None, *args, a, 1 << 30, None) == INVAL      # NULL perm
    assert seg(300, 97, a, a, a, a, 256, 64, 1500, None, a, a, a, a, a, 1 << 30, None) == INVAL
    assert seg(-1, 97, a, a, a, a, *args, a, 1 << 30, None) == INVAL
    assert seg(300, 97, a, a, a, a, 255, 64, 1500, a, a, a, a, a, a, 1 << 30, None) == INVAL
    assert seg(300, 97, a, a, a, a, *args, C.c_void_p(0x10004), 1 << 30, None) == MISALIGNED


def test_w1_step_argument_validation_without_gpu(native_lib):
    step = native_lib.gcg_minibatch_w1_step_f32
    a = C.c_void_p(0x10000)
    tail = (a, a, a, a, a, 0.0, 0.0, a, 0.9, 0.999, 1e-8, None)
    assert step(-1, 4, a, a, a, a, 4, 8, *tail) == INVAL
    assert step(10, -4, a, a, a, a, 4, 8, *tail) == INVAL
    assert step(10, 4, a, a, a, a, 3, 8, *tail) == INVAL                       # ldg < K
    assert step(10, 4, None, a, a, a, 4, 8, *tail) == INVAL                    # NULL W
    assert step(10, 4, a, a, a, None, 4, 8, *tail) == INVAL                    # NULL G
    assert step(10, 4, a, a, a, a, 4, 8, a, a, a, a, a, 0.0, 0.0, None, 0.9, 0.999, 1e-8,
                None) == INVAL                                                 # NULL step size
    assert "gcg_minibatch_w1_step_f32" in native_lib.gcg_last_error().decode()
    assert step(10, 4, C.c_void_p(0x10002), a, a, a, 4, 8, *tail) == MISALIGNED
    assert step(0, 4, None, None, None, None, 4, 8, None, None, None, None, None, 0.0, 0.0, None,
                0.9, 0.999, 1e-8, None) == OK                                  # empty: no launch
    assert step(10, 0, None, None, None, None, 0, 8, None, None, None, None, None, 0.0, 0.0, None,
                0.9, 0.999, 1e-8, None) == OK
