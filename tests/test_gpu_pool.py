"""GGML_OP_POOL_1D / POOL_2D on the device, through the C ABI (cllm_op_pool_1d / _2d) via the Python mirror (ops.pool_1d / pool_2d), against the reference's own CPU
backend: the numpy restatements of tests/ref_conv.py, which tests/test_conv_model.py shows equal to ggml_pool_1d / _2d on these case lists.  0 differing words through a
uint32 view; a NaN where the reference gives one.  The destination lies inside a sentinel-filled buffer.
What the lists catch (predicted with the restatement): dividing the 2-D average by the positions inside fails every 2-D case with padding (4 of 5) and the quirk
test; dividing the 1-D one by k fails every 1-D case with padding or a cut last window; swapping s0 / s1, k0 / k1 or p0 / p1 fails the first, second and fifth 2-D case;
walking kx outside ky, or summing in another order, fails the AVG cases through the alternating large magnitudes; fmaxf in place of std::max fails the NaN quirk."""
import ctypes as C

import numpy as np
import pytest

import ref_conv as RC
import ref_norm as N

pytestmark = pytest.mark.gpu

CLLM_E_INVALID, CLLM_E_UNSUPPORTED = -1, -2
SENT = np.float32(-7.25)
_cache = {}


def shared(key, make):
    if key not in _cache:
        v = make()
        for a in v:
            a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def run(gpu, x, call, out_shape):
    """call(src, dst) on a destination inside a sentinel-filled buffer; the sentinel must survive on both sides"""
    n = int(np.prod(out_shape))
    buf = gpu.Tensor.from_numpy(np.full(n + 8, SENT, np.float32))
    ne = list(reversed(out_shape)) + [1] * (4 - len(out_shape))
    dst = buf.view(ne, [4, 4 * ne[0], 4 * ne[0] * ne[1], 4 * ne[0] * ne[1] * ne[2]], 16)
    src = gpu.Tensor.from_numpy(np.concatenate([x.reshape(-1), np.full(16, 1e30, np.float32)])).view(
        list(reversed(x.shape)) + [1] * (4 - x.ndim), [4] + [4 * int(np.prod(x.shape[x.ndim - i:])) for i in range(1, 4)])
    call(src, dst)
    words = buf.numpy()
    assert np.all(words[:4] == SENT) and np.all(words[4 + n:] == SENT), "written outside the destination"
    return words[4:4 + n].reshape(out_shape)


@pytest.mark.parametrize("op", [RC.POOL_AVG, RC.POOL_MAX])
@pytest.mark.parametrize("case", RC.POOL_1D)
def test_pool_1d(gpu, case, op):
    IW, k0, s0, p0 = case
    x, want = shared(("1d", case, op), lambda: (lambda x: (x, RC.pool_1d_np(x, op, k0, s0, p0)))(RC.pool_input((2, 3, 2, IW), 100 + IW + k0)))
    got = run(gpu, x, lambda s, d: gpu.ops.pool_1d(s, op, k0, s0, p0, dst=d), want.shape)
    N.assert_same_words(got, want, f"pool_1d {case} op {op}")


@pytest.mark.parametrize("op", [RC.POOL_AVG, RC.POOL_MAX])
@pytest.mark.parametrize("case", RC.POOL_2D)
def test_pool_2d(gpu, case, op):
    IH, IW, k0, k1, s0, s1, p0, p1 = case
    x, want = shared(("2d", case, op), lambda: (lambda x: (x, RC.pool_2d_np(x, op, k0, k1, s0, s1, p0, p1)))(RC.pool_input((2, 3, IH, IW), 200 + IW + k0)))
    got = run(gpu, x, lambda s, d: gpu.ops.pool_2d(s, op, k0, k1, s0, s1, p0, p1, dst=d), want.shape)
    N.assert_same_words(got, want, f"pool_2d {case} op {op}")


def test_more_than_one_workgroup(gpu):
    """[65, 9, 5, 3] -> 3 * 5 * 9 * 32 outputs: 17 workgroups of 256"""
    x, want = shared(("big",), lambda: (lambda x: (x, RC.pool_1d_np(x, RC.POOL_AVG, 3, 2, 0)))(RC.pool_input((3, 5, 9, 65), 9)))
    got = run(gpu, x, lambda s, d: gpu.ops.pool_1d(s, RC.POOL_AVG, 3, 2, 0, dst=d), want.shape)
    N.assert_same_words(got, want, "pool_1d, several workgroups")


def test_the_1d_average_divides_by_the_positions_inside(gpu):
    """[pad, 1] / 1 and [2, 4] / 2; a window wholly in the padding is 0.0f"""
    got = run(gpu, np.array([[1.0, 2.0, 4.0]], np.float32), lambda s, d: gpu.ops.pool_1d(s, RC.POOL_AVG, 2, 2, 1, dst=d), (1, 2))
    assert got.tolist() == [[1.0, 3.0]]
    got = run(gpu, np.array([[3.0]], np.float32), lambda s, d: gpu.ops.pool_1d(s, RC.POOL_AVG, 1, 1, 1, dst=d), (1, 3))
    assert got.view(np.uint32).tolist() == [[0, np.float32(3.0).view(np.uint32), 0]]


def test_the_2d_average_divides_by_the_window_always(gpu):
    y = np.array([[[1.0, 2.0], [4.0, 8.0]]], np.float32)
    got = run(gpu, y, lambda s, d: gpu.ops.pool_2d(s, RC.POOL_AVG, 2, 2, 2, 2, 1, 1, dst=d), (1, 2, 2))
    assert got.tolist() == [[[0.25, 0.5], [1.0, 2.0]]]


def test_the_division_is_ieee(gpu):
    """sums whose quotient by 3 needs correct rounding"""
    x = shared(("div",), lambda: (np.random.default_rng(3).standard_normal((4, 3 * 257)).astype(np.float32) * np.float32(1e-3),))[0]
    want = RC.pool_1d_np(x, RC.POOL_AVG, 3, 3, 0)
    got = run(gpu, x, lambda s, d: gpu.ops.pool_1d(s, RC.POOL_AVG, 3, 3, 0, dst=d), want.shape)
    N.assert_same_words(got, want, "avg / 3")


def test_max_keeps_a_nan_only_while_nothing_follows_it(gpu):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    z = np.array([[nan, 1.0, 2.0, nan, -inf, -inf, nan, nan]], np.float32)
    got = run(gpu, z, lambda s, d: gpu.ops.pool_1d(s, RC.POOL_MAX, 2, 2, 0, dst=d), (1, 4))[0]
    assert got[0] == 1.0 and np.isnan(got[1]) and got[2] == -RC.FLT_MAX and np.isnan(got[3])
    N.assert_same_words_nan_for_nan(got, RC.pool_1d_np(z, RC.POOL_MAX, 2, 2, 0)[0], "max with NaNs")


def test_max_over_the_padding_alone_is_minus_flt_max(gpu):
    got = run(gpu, np.array([[3.0]], np.float32), lambda s, d: gpu.ops.pool_1d(s, RC.POOL_MAX, 1, 1, 1, dst=d), (1, 3))
    assert got.tolist() == [[-RC.FLT_MAX, 3.0, -RC.FLT_MAX]]
    y = np.full((1, 2, 2), -np.inf, np.float32)
    got = run(gpu, y, lambda s, d: gpu.ops.pool_2d(s, RC.POOL_MAX, 1, 1, 1, 1, 1, 1, dst=d), (1, 4, 4))
    assert np.all(got == -RC.FLT_MAX)


def test_an_empty_tensor_is_no_launch(gpu):
    assert gpu.ops.pool_1d(gpu.Tensor(gpu.F32, [8, 0]), RC.POOL_AVG, 2, 2, 0).ne[:2] == [4, 0]


# ---- what is declined -----------------------------------------------------------------------------------------------------------------------
def declined(gpu, rc, word, call, dst_host):
    dst = gpu.Tensor.from_numpy(dst_host)
    with pytest.raises(gpu.lib.CllmError) as e:
        call(dst)
    assert e.value.rc == rc and word in str(e.value), str(e.value)
    assert np.array_equal(dst.numpy(), dst_host)


def test_declines(gpu):
    a = gpu.Tensor.from_numpy(np.ones((2, 6, 8), np.float32))
    d1, d2 = np.full((2, 6, 4), SENT, np.float32), np.full((2, 3, 4), SENT, np.float32)
    h = gpu.Tensor.from_numpy(np.ones((2, 6, 8), np.float16))
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda d: gpu.ops.pool_1d(h, RC.POOL_AVG, 2, 2, 0, dst=d), d1)                   # an F16 source
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda d: gpu.ops.pool_2d(h, RC.POOL_AVG, 2, 2, 2, 2, 0, 0, dst=d), d2)
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda d: gpu.ops.pool_1d(a, RC.POOL_AVG, 2, 2, 0, dst=d), d1.astype(np.float16))  # an F16 destination
    declined(gpu, CLLM_E_INVALID, "op", lambda d: gpu.ops.pool_1d(a, 2, 2, 2, 0, dst=d), d1)                                    # GGML_OP_POOL_COUNT
    declined(gpu, CLLM_E_INVALID, "op", lambda d: gpu.ops.pool_2d(a, -1, 2, 2, 2, 2, 0, 0, dst=d), d2)
    for k, s, p in [(0, 2, 0), (2, 0, 0), (2, 2, -1)]:
        declined(gpu, CLLM_E_INVALID, "kernel, stride or padding", lambda d: gpu.ops.pool_1d(a, RC.POOL_AVG, k, s, p, dst=d), d1)
    for q in [(2, 0, 2, 2, 0, 0), (2, 2, 2, 0, 0, 0), (2, 2, 2, 2, 0, -1)]:
        declined(gpu, CLLM_E_INVALID, "kernel, stride or padding", lambda d: gpu.ops.pool_2d(a, RC.POOL_AVG, *q, dst=d), d2)
    declined(gpu, CLLM_E_INVALID, "shape", lambda d: gpu.ops.pool_1d(a, RC.POOL_AVG, 2, 2, 0, dst=d), d2)                        # dst ne is not the rule's
    declined(gpu, CLLM_E_INVALID, "shape", lambda d: gpu.ops.pool_2d(a, RC.POOL_AVG, 2, 2, 2, 2, 0, 0, dst=d), d1)
    declined(gpu, CLLM_E_INVALID, "shape", lambda d: gpu.ops.pool_1d(a, RC.POOL_AVG, 9, 1, 0, dst=d), d1)                        # the window is wider than the row
    wide = gpu.Tensor.from_numpy(np.ones(4096, np.float32))
    declined(gpu, CLLM_E_UNSUPPORTED, "contiguous", lambda d: gpu.ops.pool_1d(wide.view([8, 6, 2], [4, 40, 240]), RC.POOL_AVG, 2, 2, 0, dst=d), d1)      # a view as source
    declined(gpu, CLLM_E_UNSUPPORTED, "contiguous", lambda d: gpu.ops.pool_2d(wide.view([8, 6, 2], [8, 64, 384]), RC.POOL_MAX, 2, 2, 2, 2, 0, 0, dst=d), d2)
    back = gpu.Tensor.from_numpy(np.full(4096, SENT, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.pool_1d(a, RC.POOL_AVG, 2, 2, 0, dst=back.view([4, 6, 2], [4, 24, 144]))                                        # a view as destination
    assert e.value.rc == CLLM_E_UNSUPPORTED and "contiguous" in str(e.value)
    assert np.all(back.numpy() == SENT)


def test_a_null_tensor_is_declined(gpu):
    a = gpu.Tensor.from_numpy(np.ones((2, 8), np.float32))
    L = gpu.lib.get()
    ca = a.c()
    assert L.cllm_op_pool_1d(None, 1, None, C.byref(ca), 2, 2, 0) == CLLM_E_INVALID and b"null" in L.cllm_last_error()
    assert L.cllm_op_pool_1d(None, 1, C.byref(ca), None, 2, 2, 0) == CLLM_E_INVALID
    assert L.cllm_op_pool_2d(None, 1, None, C.byref(ca), 2, 2, 2, 2, 0, 0) == CLLM_E_INVALID and b"null" in L.cllm_last_error()
    assert L.cllm_op_pool_2d(None, 1, C.byref(ca), None, 2, 2, 2, 2, 0, 0) == CLLM_E_INVALID
    assert np.array_equal(a.numpy(), np.ones((2, 8), np.float32))
