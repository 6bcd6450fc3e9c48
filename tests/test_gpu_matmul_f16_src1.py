"""MUL_MAT with an F16 src1 on an F16 src0 (the second node of ggml_conv_1d / _2d: im2col . kernel) on the device, against the reference's own CPU backend
(ref_conv.mul_mat_f16), 0 differing words.  The reference reads such a src1 in place: tinyBLAS when it is contiguous and ne11 >= 2, K % 8 == 0, ne01 % 4 == 0, else
ggml_vec_dot_f16 through its strides; tests/test_conv_model.py shows that the two give different words for the same values, so the contiguous / padded pairs below pin
the route.  The lane-group kernels take every column count and every prefill mode: an F16 src1 never reaches the tolerance tier."""
import ctypes as C

import numpy as np
import pytest

import ref_conv as RC
import ref_norm as N
from conftest import prefill_mode
from ref_ggml import GGML_TYPE_F16

pytestmark = pytest.mark.gpu

CLLM_E_INVALID, CLLM_E_UNSUPPORTED = -1, -2
KS = [8, 24, 32, 40, 72, 260]
ROWS0 = [1, 3, 4, 5, 33]
ROWS1 = [1, 2, 5]
_cache = {}


def shared(key, make):
    if key not in _cache:
        v = make()
        for a in v:
            a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def device(gpu, buf, view):
    return gpu.Tensor.from_strided(np.ascontiguousarray(buf).view(np.uint8), gpu.F16, view.ne, view.nb)


def product(gpu, w, x, pad):
    """(device words, reference words) of w [.., M, K] and x [.., Ncol, K] (uint16 words), x's rows `pad` halves apart beyond K"""
    wb, wv = w.reshape(-1), RC.dense_view(w)
    xb, xv = RC.padded_rows(x, pad) if pad else (x.reshape(-1), RC.dense_view(x))
    want = RC.mul_mat_f16(wb, wv, xb, xv)
    got = gpu.ops.mul_mat(device(gpu, wb, wv), device(gpu, xb, xv)).numpy().reshape(want.shape)
    return got, want


def same(got, want, what):
    """0 differing words; a NaN where the reference gives one (the edge values alone produce any)"""
    N.assert_same_words_nan_for_nan(got, want, what)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("K", KS)
def test_every_row_count_on_both_layouts(gpu, K, pad):
    """src0 rows 1, 3, 4, 5, 33 x src1 rows 1, 2, 5, contiguous (tinyBLAS where it takes the product) and behind padded rows (vec_dot always)"""
    for M in ROWS0:
        for Ncol in ROWS1:
            w, x = shared(("ops", K, M, Ncol), lambda: (RC.halves((M, K), K + M, 3.0), RC.halves((Ncol, K), K + Ncol + 100, 3.0)))
            got, want = product(gpu, w, x, pad)
            same(got, want, f"K {K} M {M} N {Ncol} pad {pad}")


def test_the_contiguous_and_the_padded_product_differ_where_the_routes_do(gpu):
    """the same values: tinyBLAS words for the contiguous src1, vec_dot words behind padded rows -- and the device has each"""
    w, x = shared(("route",), lambda: (RC.halves((8, 72), 3, 3.0), RC.halves((2, 72), 4, 3.0)))
    g0, w0 = product(gpu, w, x, 0)
    g1, w1 = product(gpu, w, x, 8)
    assert np.count_nonzero(w0.view(np.uint32) != w1.view(np.uint32)) > 0
    same(g0, w0, "contiguous")
    same(g1, w1, "padded")


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("K,M", [(72, 8), (40, 5), (260, 4)])
def test_batches_and_broadcast(gpu, K, M, pad):
    """ne[2] = 2 on both; then src1 ne[2] = 4 over src0 ne[2] = 2 (r2 = 2)"""
    for b1 in (2, 4):
        w, x = shared(("batch", K, M, b1), lambda: (RC.halves((2, M, K), K + 7, 3.0), RC.halves((b1, 3, K), K + 8, 3.0)))
        got, want = product(gpu, w, x, pad)
        same(got, want, f"K {K} M {M} batches 2 x {b1} pad {pad}")


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("K,M,Ncol", [(72, 8, 2), (40, 5, 2), (260, 4, 1)])
def test_edge_values(gpu, K, M, Ncol, pad):
    """+-0, subnormals, the largest finite halves, +-inf and NaNs in both operands: the reference's words, a NaN where it gives one"""
    w, x = shared(("edge", K, M, Ncol), lambda: (RC.edge_halves((M, K), K), RC.edge_halves((Ncol, K), K + 50)))
    with np.errstate(all="ignore"):
        got, want = product(gpu, w, x, pad)
    same(got, want, "edge values")


@pytest.mark.parametrize("mode", [0, 1])
def test_many_columns_stay_on_the_exact_kernels_in_every_prefill_mode(gpu, mode):
    """40 columns (past every column threshold of the F32-src1 routes), in the fast and in the exact prefill mode: the reference's words"""
    w, x = shared(("cols",), lambda: (RC.halves((8, 72), 30, 3.0), RC.halves((40, 72), 31, 3.0)))
    with prefill_mode(gpu, mode):
        got, want = product(gpu, w, x, 0)
    same(got, want, f"40 columns, prefill mode {mode}")


# ---- what is declined -----------------------------------------------------------------------------------------------------------------------
def test_an_f16_src1_with_another_src0_is_declined(gpu):
    x = gpu.Tensor.from_numpy(np.ones((2, 32), np.float16))
    for w in (gpu.Tensor.from_numpy(np.ones((4, 32), np.float32)), gpu.Tensor(gpu.Q8_0, [32, 4]), gpu.Tensor(gpu.Q4_K, [256, 4])):
        xx = x if w.ne[0] == 32 else gpu.Tensor.from_numpy(np.ones((2, 256), np.float16))
        dst = gpu.Tensor.from_numpy(np.full((2, 4), 7.0, np.float32))
        with pytest.raises(gpu.lib.CllmError) as e:
            gpu.ops.mul_mat(w, xx, dst=dst)
        assert e.value.rc == CLLM_E_UNSUPPORTED and "F16" in str(e.value), str(e.value)
        assert np.all(dst.numpy() == 7.0)


def test_strides_that_are_no_multiple_of_2_and_rows_that_are_not_dense_are_declined(gpu):
    w = gpu.Tensor.from_numpy(np.ones((4, 32), np.float16))
    raw = gpu.Tensor.from_numpy(np.ones(1024, np.float16))
    dst = gpu.Tensor.from_numpy(np.full((2, 4), 7.0, np.float32))
    for view, word in ((raw.view([32, 2], [2, 65]), "aligned"), (raw.view([32, 2], [2, 64], 1), "aligned"), (raw.view([32, 2], [4, 128]), "dense")):
        with pytest.raises(gpu.lib.CllmError) as e:
            gpu.ops.mul_mat(w, view, dst=dst)
        assert e.value.rc == CLLM_E_UNSUPPORTED and word in str(e.value), str(e.value)
        assert np.all(dst.numpy() == 7.0)


def test_a_k_mismatch_is_declined(gpu):
    w = gpu.Tensor.from_numpy(np.ones((4, 32), np.float16))
    x = gpu.Tensor.from_numpy(np.ones((2, 40), np.float16))
    dst = gpu.Tensor.from_numpy(np.full((2, 4), 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.mul_mat(w, x, dst=dst)
    assert e.value.rc == CLLM_E_INVALID and "K mismatch" in str(e.value)
    assert np.all(dst.numpy() == 7.0)


def test_the_scratch_size_is_unaffected(gpu):
    w, x = gpu.Tensor.from_numpy(np.ones((4, 32), np.float16)), gpu.Tensor.from_numpy(np.ones((2, 32), np.float16))
    cw, cx = w.c(), x.c()
    assert gpu.lib.get().cllm_mul_mat_wsize(C.byref(cw), C.byref(cx)) == 0
