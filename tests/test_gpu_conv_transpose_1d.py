"""GGML_OP_CONV_TRANSPOSE_1D on the device, through the C ABI (cllm_op_conv_transpose_1d) via the Python mirror (ops.conv_transpose_1d), with an F16 and an F32 kernel,
against the reference's own CPU backend: the numpy restatement of tests/ref_resample.py, which tests/test_resample_model.py shows equal to ggml_conv_transpose_1d on
this case list -- and shows that adding the taps in descending order, or a plain sequential dot product, gives other words on it.  0 differing words; a NaN where the
reference gives one.  The operands put large and small magnitudes side by side, so the 32-accumulator order, its tree, the leftovers' arithmetic (F16: in double; F32: a
group of four rounded products, then fmas) and the ascending order of the taps each decide words.  The destination lies inside a sentinel-filled buffer."""
import ctypes as C

import numpy as np
import pytest

import ref_norm as N
import ref_resample as RR

pytestmark = pytest.mark.gpu

CLLM_E_INVALID, CLLM_E_UNSUPPORTED = RR.CLLM_E_INVALID, RR.CLLM_E_UNSUPPORTED
SENT = RR.SENT
TYPES = pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
shared, declined = RR.shared, RR.declined


def run(gpu, k, x, s0, layout="dense"):
    (kr, kv), (xr, xv) = RR.conv_t_views(k, x, layout)
    kt, xt = RR.device_view(gpu, kr, kv), RR.device_view(gpu, xr, xv)
    shape = (k.shape[1], (x.shape[1] - 1) * s0 + k.shape[2])
    return RR.run_in_sentinel(gpu, lambda d: gpu.ops.conv_transpose_1d(kt, xt, s0, dst=d), shape)


@TYPES
@pytest.mark.parametrize("case", RR.CONV_T)
def test_conv_transpose_1d(gpu, case, f16):
    k, x = RR.conv_t_operands(case, f16)
    want = shared((case, f16), lambda: RR.conv_transpose_1d_np(k, x, case[4]))
    N.assert_same_words(run(gpu, k, x, case[4]), want, f"conv_transpose_1d {case} f16 {f16}")


@TYPES
@pytest.mark.parametrize("layout", ["padded data", "padded kernel"])
def test_the_strides_are_read_as_given(gpu, layout, f16):
    """a data matrix with nb11 > 4 L and a kernel with padded nb01 and nb02, poison in the gaps"""
    case = (5, 2, 70, 4, 2)
    k, x = RR.conv_t_operands(case, f16, 1)
    want = shared(("strides", f16), lambda: RR.conv_transpose_1d_np(k, x, case[4]))
    N.assert_same_words(run(gpu, k, x, case[4], layout), want, layout)


@TYPES
def test_products_of_minus_zero_and_untouched_outputs_give_plus_zero(gpu, f16):
    k = np.full((8, 3, 2), 1.5, np.float32)
    k = k.astype(np.float16).view(np.uint16) if f16 else k
    got = run(gpu, k, np.full((8, 5), -0.0, np.float32), 4)
    assert got.shape == (3, 18) and np.all(got.view(np.uint32) == 0)


@TYPES
def test_data_beyond_the_fp16_range(gpu, f16):
    """1e5 rounds to the fp16 infinity under an F16 kernel (inf - inf: a NaN where the reference has one) and stays finite under an F32 kernel"""
    case = (4, 3, 40, 6, 2)
    k, x = RR.conv_t_operands(case, f16, 2)
    x = x.copy()
    x[::3, ::2] = np.float32(1e5)
    x[1, 1] = np.float32(-7e4)
    want = shared(("beyond", f16), lambda: RR.conv_transpose_1d_np(k, x, case[4]))
    assert bool(np.any(np.isnan(want))) == f16
    N.assert_same_words_nan_for_nan(run(gpu, k, x, case[4]), want, "data beyond 65504")


def test_an_empty_tensor_is_no_launch(gpu):
    k = gpu.Tensor(gpu.F16, [4, 0, 8])
    assert gpu.ops.conv_transpose_1d(k, gpu.Tensor(gpu.F32, [5, 8]), 2).ne == [12, 0, 1, 1]


# ---- what is declined -----------------------------------------------------------------------------------------------------------------------
def test_declines(gpu):
    ct = gpu.ops.conv_transpose_1d
    k = gpu.Tensor.from_numpy(np.ones((8, 3, 4), np.float16))          # [K 4, Cout 3, Cin 8]
    kf = gpu.Tensor.from_numpy(np.ones((8, 3, 4), np.float32))
    x = gpu.Tensor.from_numpy(np.ones((8, 5), np.float32))             # [L 5, Cin 8]
    d = np.full((3, 12), SENT, np.float32)                             # (5 - 1) * 2 + 4
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda t: ct(gpu.Tensor.from_numpy(np.ones((8, 3, 4), np.int32)), x, 2, dst=t), d)
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda t: ct(k, gpu.Tensor.from_numpy(np.ones((8, 5), np.float16)), 2, dst=t), d)
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda t: ct(k, x, 2, dst=t), d.astype(np.float16))
    for s0 in (0, -2):
        declined(gpu, CLLM_E_INVALID, "stride", lambda t: ct(k, x, s0, dst=t), d)
    wide16, wide32 = gpu.Tensor.from_numpy(np.ones(4096, np.float16)), gpu.Tensor.from_numpy(np.ones(4096, np.float32))
    declined(gpu, CLLM_E_UNSUPPORTED, "dense", lambda t: ct(wide16.view([4, 3, 8], [4, 16, 48]), x, 2, dst=t), d)      # kernel nb00 != 2
    declined(gpu, CLLM_E_UNSUPPORTED, "dense", lambda t: ct(wide32.view([4, 3, 8], [8, 32, 96]), x, 2, dst=t), d)      # kernel nb00 != 4
    declined(gpu, CLLM_E_UNSUPPORTED, "dense", lambda t: ct(k, wide32.view([5, 8], [8, 40]), 2, dst=t), d)             # data nb10 != 4
    declined(gpu, CLLM_E_INVALID, "shape", lambda t: ct(k, gpu.Tensor.from_numpy(np.ones((7, 5), np.float32)), 2, dst=t), d)          # Cin of the kernel and of the data
    declined(gpu, CLLM_E_INVALID, "shape", lambda t: ct(k, gpu.Tensor.from_numpy(np.ones((2, 8, 5), np.float32)), 2, dst=t), d)       # the data is no matrix
    declined(gpu, CLLM_E_INVALID, "shape", lambda t: ct(gpu.Tensor.from_numpy(np.ones((2, 8, 3, 4), np.float16)), x, 2, dst=t), d)    # kernel ne[3] != 1
    declined(gpu, CLLM_E_INVALID, "shape", lambda t: ct(k, x, 3, dst=t), d)                                                            # dst ne[0] is not (L - 1) s0 + K
    declined(gpu, CLLM_E_INVALID, "shape", lambda t: ct(kf, x, 2, dst=t), np.full((4, 12), SENT, np.float32))                          # dst ne[1] is not Cout
    declined(gpu, CLLM_E_UNSUPPORTED, "alignment", lambda t: ct(wide32.view([4, 3, 8], [4, 18, 54]), x, 2, dst=t), d)                 # kernel rows that do not start on an element
    back = gpu.Tensor.from_numpy(np.full(4096, SENT, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        ct(k, x, 2, dst=back.view([12, 3], [4, 64]))                                                                                   # a view as destination
    assert e.value.rc == CLLM_E_UNSUPPORTED and "contiguous" in str(e.value)
    # operands that do not start on an element, data rows that are no whole floats apart, a destination that does not start on a float
    declined(gpu, CLLM_E_UNSUPPORTED, "alignment", lambda t: ct(wide16.view([4, 3, 8], [2, 8, 24], 1), x, 2, dst=t), d)
    declined(gpu, CLLM_E_UNSUPPORTED, "alignment", lambda t: ct(k, wide32.view([5, 8], [4, 20], 2), 2, dst=t), d)
    declined(gpu, CLLM_E_UNSUPPORTED, "alignment", lambda t: ct(k, wide32.view([5, 8], [4, 22]), 2, dst=t), d)
    with pytest.raises(gpu.lib.CllmError) as e:
        ct(k, x, 2, dst=back.view([12, 3], [4, 48], 2))
    assert e.value.rc == CLLM_E_UNSUPPORTED and "alignment" in str(e.value)
    assert np.all(back.numpy() == SENT)


def test_a_null_tensor_is_declined(gpu):
    a = gpu.Tensor.from_numpy(np.ones((2, 8), np.float32))
    L = gpu.lib.get()
    ca = a.c()
    for args in ((None, C.byref(ca), C.byref(ca)), (C.byref(ca), None, C.byref(ca)), (C.byref(ca), C.byref(ca), None)):
        assert L.cllm_op_conv_transpose_1d(None, *args, 1) == CLLM_E_INVALID and b"null" in L.cllm_last_error()
    assert np.array_equal(a.numpy(), np.ones((2, 8), np.float32))
