"""GGML_OP_UPSCALE on the device (NEAREST and plain BILINEAR: what ggml::interpolate emits), through the C ABI (cllm_op_upscale) via the Python mirror (ops.upscale),
against the reference's own CPU backend: the numpy restatement of tests/ref_resample.py, which tests/test_resample_model.py shows equal to ggml_interpolate on this case
list -- and shows that of the twelve possible fma contractions of the bilinear expression only the one restated matches.  0 differing words.  Inputs alternate between
1e4 and 1e-4 per element, so a product rounded where the reference fuses it (or the reverse), a reciprocal in place of the IEEE division, or dx taken from the
unclamped index changes words.  The destination lies inside a sentinel-filled buffer."""
import ctypes as C

import numpy as np
import pytest

import ref_norm as N
import ref_resample as RR

pytestmark = pytest.mark.gpu

CLLM_E_INVALID, CLLM_E_UNSUPPORTED = RR.CLLM_E_INVALID, RR.CLLM_E_UNSUPPORTED
SENT = RR.SENT
SOURCES = RR.upscale_sources()
shared, declined = RR.shared, RR.declined


@pytest.mark.parametrize("mode", [RR.NEAREST, RR.BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("i", range(len(SOURCES)), ids=[s[0] for s in SOURCES])
def test_upscale(gpu, i, mode):
    name, raw, view, ne = SOURCES[i]
    want = shared((i, mode), lambda: RR.upscale_np(RR.gather(raw, view), ne, mode))
    src = RR.device_view(gpu, raw, view)
    got = RR.run_in_sentinel(gpu, lambda d: gpu.ops.upscale(src, mode, dst=d), want.shape)
    N.assert_same_words(got, want, f"upscale {name} mode {mode}")


def test_nearest_moves_words(gpu):
    """NaN payloads, -0.0, infinities and subnormals pass through NEAREST as they are"""
    x = RR.edge_mix((2, 3, 5), 7)
    want = RR.upscale_np(x, [9, 7, 2, 1], RR.NEAREST)
    got = RR.run_in_sentinel(gpu, lambda d: gpu.ops.upscale(gpu.Tensor.from_numpy(x), RR.NEAREST, dst=d), want.shape)
    N.assert_same_words(got, want, "nearest over edge values")


def test_the_scale_factor_form_is_the_hosts(gpu):
    """ggml::interpolate(a, mode, scale_factor): [int64(ne0 * f), int64(ne1 * f), ne2, ne3]"""
    x = RR.upscale_input((2, 3, 4), 5)
    got = gpu.ops.upscale(gpu.Tensor.from_numpy(x), RR.BILINEAR, scale_factor=2.5)
    assert got.ne == [10, 7, 2, 1]
    N.assert_same_words(got.numpy(), RR.upscale_np(x, [10, 7, 2, 1], RR.BILINEAR)[0], "scale_factor 2.5")
    assert gpu.ops.upscale(gpu.Tensor.from_numpy(x), RR.NEAREST, ne=[8, 6, 2]).ne == [8, 6, 2, 1]


def test_an_empty_tensor_is_no_launch(gpu):
    assert gpu.ops.upscale(gpu.Tensor(gpu.F32, [4, 0]), RR.NEAREST, ne=[8, 0]).ne[:2] == [8, 0]


# ---- what is declined -----------------------------------------------------------------------------------------------------------------------
def test_declines(gpu):
    a = gpu.Tensor.from_numpy(np.ones((2, 3, 4), np.float32))
    h = gpu.Tensor.from_numpy(np.ones((2, 3, 4), np.float16))
    d = np.full((2, 6, 8), SENT, np.float32)
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda t: gpu.ops.upscale(h, RR.NEAREST, dst=t), d)
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda t: gpu.ops.upscale(a, RR.NEAREST, dst=t), d.astype(np.float16))
    # GGML_SCALE_MODE_BICUBIC, GGML_SCALE_FLAG_ALIGN_CORNERS and GGML_SCALE_FLAG_ANTIALIAS on either mode, a mode beyond the enum, a negative word
    for mode in (2, 0 | 1 << 8, 1 | 1 << 8, 1 | 1 << 9, 1 | 1 << 8 | 1 << 9, 3, 1 << 16, -1):
        declined(gpu, CLLM_E_UNSUPPORTED, "mode", lambda t: gpu.ops.upscale(a, mode, dst=t), d)
    wide = gpu.Tensor.from_numpy(np.ones(4096, np.float32))
    declined(gpu, CLLM_E_UNSUPPORTED, "alignment", lambda t: gpu.ops.upscale(wide.view([4, 3, 2], [6, 64, 512]), RR.BILINEAR, dst=t), d)
    declined(gpu, CLLM_E_INVALID, "shape", lambda t: gpu.ops.upscale(gpu.Tensor(gpu.F32, [4, 0, 2]), RR.NEAREST, dst=t), d)             # nothing to read from
    back = gpu.Tensor.from_numpy(np.full(4096, SENT, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.upscale(a, RR.BILINEAR, dst=back.view([8, 6, 2], [4, 48, 480]))                                                            # a view as destination
    assert e.value.rc == CLLM_E_UNSUPPORTED and "contiguous" in str(e.value)
    # a source or a destination that does not start on a float
    declined(gpu, CLLM_E_UNSUPPORTED, "alignment", lambda t: gpu.ops.upscale(wide.view([4, 3, 2], [4, 16, 48], 2), RR.NEAREST, dst=t), d)
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.upscale(a, RR.BILINEAR, dst=back.view([8, 6, 2], [4, 32, 192], 2))
    assert e.value.rc == CLLM_E_UNSUPPORTED and "alignment" in str(e.value)
    assert np.all(back.numpy() == SENT)


def test_a_null_tensor_is_declined(gpu):
    a = gpu.Tensor.from_numpy(np.ones((2, 8), np.float32))
    L = gpu.lib.get()
    ca = a.c()
    assert L.cllm_op_upscale(None, None, C.byref(ca), 0) == CLLM_E_INVALID and b"null" in L.cllm_last_error()
    assert L.cllm_op_upscale(None, C.byref(ca), None, 1) == CLLM_E_INVALID
    assert np.array_equal(a.numpy(), np.ones((2, 8), np.float32))
