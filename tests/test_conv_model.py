"""CPU-only: what the convolution nodes' GPU tests stand on.  The header declares cllm_op_im2col / cllm_op_pool_1d / cllm_op_pool_2d and the library exports them; the
numpy restatements of the three index rules (tests/ref_conv.py) equal the reference's own CPU backend on the GPU files' case lists, F16 rounding and edge values
included; the reference's MUL_MAT with an F16 src1 on an F16 src0 gives DIFFERENT words on its tinyBLAS route and its vec_dot route for the same values, and a
padded-row src1 takes the vec_dot words -- without which the route cases of tests/test_gpu_matmul_f16_src1.py would prove nothing."""
import os
import subprocess

import numpy as np
import pytest

import ref_conv as RC
import ref_ggml as R
from ref_ggml import GGML_TYPE_F16, GGML_TYPE_F32, View
from test_abi import header_symbols

NEW = ("cllm_op_im2col", "cllm_op_pool_1d", "cllm_op_pool_2d")
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built")


def test_the_header_declares_and_the_library_exports_the_three_entries(pkg):
    syms = header_symbols()
    for s in NEW:
        assert s in syms, s
        assert s in pkg.lib.SIGNATURES, s
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib.SO_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [s for s in NEW if s not in exported]
    txt = open(os.path.join(os.path.dirname(pkg.lib.SO_PATH), "..", "include", "chatllm_hip.h")).read()
    for cite in ("ggml_compute_forward_im2col_f16", "ggml_compute_forward_pool_1d", "ggml_compute_forward_pool_2d"):
        assert cite in txt, cite


def _view_1d(IC, IW, N):
    return View(GGML_TYPE_F32, [IW, IC, N, 1])


@needs_ref
@pytest.mark.parametrize("dst_type", [GGML_TYPE_F16, GGML_TYPE_F32])
@pytest.mark.parametrize("case", RC.IM2COL_1D)
def test_im2col_1d_restated(case, dst_type):
    IC, IW, KW, s0, p0, d0, N = case
    for x in (RC.random_image((N, IC, IW), 11 + IW), RC.edge_image((N, IC, IW))):
        want = RC.im2col(x, _view_1d(IC, IW, N), [KW, IC, 2], GGML_TYPE_F16, s0, 0, p0, 0, d0, 0, False, dst_type)
        got = RC.im2col_np(x, 1, KW, s0, 0, p0, 0, d0, 0, False, dst_type)
        assert got.dtype == want.dtype and np.array_equal(got, want), case


@needs_ref
@pytest.mark.parametrize("dst_type", [GGML_TYPE_F16, GGML_TYPE_F32])
@pytest.mark.parametrize("case", RC.IM2COL_2D)
def test_im2col_2d_restated(case, dst_type):
    IC, IH, IW, KH, KW, s0, s1, p0, p1, d0, d1, N = case
    for x in (RC.random_image((N, IC, IH, IW), 13 + IW), RC.edge_image((N, IC, IH, IW))):
        want = RC.im2col(x, View(GGML_TYPE_F32, [IW, IH, IC, N]), [KW, KH, IC, 2], GGML_TYPE_F16, s0, s1, p0, p1, d0, d1, True, dst_type)
        got = RC.im2col_np(x, KH, KW, s0, s1, p0, p1, d0, d1, True, dst_type)
        assert got.dtype == want.dtype and np.array_equal(got, want), case


@needs_ref
def test_im2col_honours_padded_channel_and_batch_strides():
    """the reference reads the channel and batch strides as given (ops.cpp:6151-6152): a view with poison between channels and batches gathers the same words"""
    IC, IH, IW, N = 3, 5, 6, 2
    x = RC.random_image((N, IC, IH, IW), 5)
    buf = np.full((N, IC + 1, IH * IW + 7), 1e30, np.float32)
    buf[:, :IC, :IH * IW] = x.reshape(N, IC, -1)
    v = View(GGML_TYPE_F32, [IW, IH, IC, N], [4, IW * 4, buf.shape[2] * 4, buf.shape[1] * buf.shape[2] * 4])
    want = RC.im2col(buf, v, [3, 2, IC, 1], GGML_TYPE_F16, 1, 2, 1, 0, 1, 1, True, GGML_TYPE_F16)
    assert np.array_equal(want, RC.im2col_np(x, 2, 3, 1, 2, 1, 0, 1, 1, True, GGML_TYPE_F16))


@needs_ref
def test_the_half_rounding_on_the_edge_values():
    """GGML_CPU_FP32_TO_FP16 of this build: round to nearest even, overflow to inf, subnormal results, every NaN -> sign | 0x7e00"""
    f = lambda bits: np.array(bits, np.uint32).view(np.float32)
    got = R.fp32_to_fp16(np.concatenate([np.array([65504.0, 65519.996, 65520.0, -65520.0, 1e5, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 0.0, -0.0], np.float32),
                                         f([0x7fc00000, 0xffc00001, 0x7f800001, 0xffa55aa5, 0x7f800000, 0xff800000])]))
    assert list(got) == [0x7bff, 0x7bff, 0x7c00, 0xfc00, 0x7c00, 0x0001, 0x0000, 0x0001, 0x3c00, 0x3c02, 0x0000, 0x8000, 0x7e00, 0xfe00, 0x7e00, 0xfe00, 0x7c00, 0xfc00]


@needs_ref
@pytest.mark.parametrize("op", [RC.POOL_AVG, RC.POOL_MAX])
@pytest.mark.parametrize("case", RC.POOL_1D)
def test_pool_1d_restated(case, op):
    IW, k0, s0, p0 = case
    x = RC.pool_input((2, 3, 2, IW), 100 + IW + k0)
    assert np.array_equal(RC.pool_1d(x, op, k0, s0, p0).view(np.uint32), RC.pool_1d_np(x, op, k0, s0, p0).view(np.uint32)), case


@needs_ref
@pytest.mark.parametrize("op", [RC.POOL_AVG, RC.POOL_MAX])
@pytest.mark.parametrize("case", RC.POOL_2D)
def test_pool_2d_restated(case, op):
    IH, IW, k0, k1, s0, s1, p0, p1 = case
    x = RC.pool_input((2, 3, IH, IW), 200 + IW + k0)
    assert np.array_equal(RC.pool_2d(x, op, k0, k1, s0, s1, p0, p1).view(np.uint32), RC.pool_2d_np(x, op, k0, k1, s0, s1, p0, p1).view(np.uint32)), case


@needs_ref
def test_the_pooling_quirks_of_the_reference():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    # 1-D AVG divides by the positions inside; a window wholly in the padding is 0.0f -- (IW 1, k 1, s 1, p 1): windows at -1, 0, 1
    x = np.array([[3.0]], np.float32)
    assert list(RC.pool_1d(x, RC.POOL_AVG, 1, 1, 1)[0]) == [0.0, 3.0, 0.0]
    assert list(RC.pool_1d(x, RC.POOL_MAX, 1, 1, 1)[0]) == [-RC.FLT_MAX, 3.0, -RC.FLT_MAX]
    assert list(RC.pool_1d(np.array([[1.0, 2.0, 4.0]], np.float32), RC.POOL_AVG, 2, 2, 1)[0]) == [1.0, 3.0]            # [pad, 1] / 1, [2, 4] / 2
    # 2-D AVG divides by k0 * k1 always
    y = np.array([[[1.0, 2.0], [4.0, 8.0]]], np.float32)
    assert RC.pool_2d(y, RC.POOL_AVG, 2, 2, 2, 2, 1, 1).tolist() == [[[0.25, 0.5], [1.0, 2.0]]]
    # MAX: a NaN stays only while nothing follows it; -inf alone gives -FLT_MAX
    z = np.array([[nan, 1.0, 2.0, nan, -inf, -inf]], np.float32)
    got = RC.pool_1d(z, RC.POOL_MAX, 2, 2, 0)[0]
    assert got[0] == 1.0 and np.isnan(got[1]) and got[2] == -RC.FLT_MAX
    for fn, a in ((RC.pool_1d_np, (z, RC.POOL_MAX, 2, 2, 0)), (RC.pool_1d_np, (x, RC.POOL_AVG, 1, 1, 1))):
        w = RC.pool_1d(*a)
        assert np.array_equal(np.isnan(fn(*a)), np.isnan(w)) and np.array_equal(fn(*a)[~np.isnan(w)], w[~np.isnan(w)])


def _mm_operands(K, M, Ncol, seed):
    """values on which the two accumulation orders round differently"""
    return RC.halves((M, K), seed, 3.0), RC.halves((Ncol, K), seed + 1, 3.0)


@needs_ref
def test_the_two_routes_of_an_f16_src1_give_different_words():
    """K % 8 == 0, ne01 % 4 == 0, 2 columns: the contiguous src1 takes tinyBLAS (one 8-lane accumulator), the same values behind padded rows take ggml_vec_dot_f16
    (32 accumulators and their tree).  Column by column (ne11 = 1: vec_dot on any layout) gives the padded product's words"""
    K, M, Ncol = 72, 8, 2
    w, x = _mm_operands(K, M, Ncol, 3)
    cont = RC.mul_mat_f16(w, RC.dense_view(w), x, RC.dense_view(x))
    xb, xv = RC.padded_rows(x, 8)
    padded = RC.mul_mat_f16(w, RC.dense_view(w), xb, xv)
    assert np.count_nonzero(cont.view(np.uint32) != padded.view(np.uint32)) > 0
    single = np.stack([RC.mul_mat_f16(w, RC.dense_view(w), x[c:c + 1], RC.dense_view(x[c:c + 1])).reshape(M) for c in range(Ncol)])
    assert np.array_equal(single.view(np.uint32), padded.reshape(Ncol, M).view(np.uint32))
    assert np.allclose(cont, padded, rtol=1e-4, atol=1e-3)


@needs_ref
@pytest.mark.parametrize("K,M,Ncol", [(72, 5, 2), (260, 8, 2), (72, 8, 1)])
def test_where_tinyblas_declines_a_contiguous_f16_src1_has_the_vec_dot_words(K, M, Ncol):
    """ne01 % 4 != 0, K % 8 != 0, one column: the contiguous and the padded src1 agree word for word (both vec_dot)"""
    w, x = _mm_operands(K, M, Ncol, 7)
    cont = RC.mul_mat_f16(w, RC.dense_view(w), x, RC.dense_view(x))
    xb, xv = RC.padded_rows(x, 8)
    assert np.array_equal(cont.view(np.uint32), RC.mul_mat_f16(w, RC.dense_view(w), xb, xv).view(np.uint32))
