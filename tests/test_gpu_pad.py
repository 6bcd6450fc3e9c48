"""GGML_OP_PAD and GGML_OP_PAD_REFLECT_1D on the device, through the C ABI (cllm_op_pad / cllm_op_pad_reflect_1d) via the Python mirror (ops.pad / ops.pad_reflect_1d),
against the reference's own CPU backend: the numpy restatements of tests/ref_resample.py, which tests/test_resample_model.py shows equal to ggml_pad_ext /
ggml_pad_reflect_1d on these case lists.  0 differing words through a uint32 view -- NaN payloads, -0.0, infinities and subnormals are moved as words.  Every case runs with
the destination 4 and 5 floats into a sentinel-filled buffer: rows that may start on 16 bytes (the 16-byte stores and the scalar tail) and rows that never do (the
word-by-word path)."""
import ctypes as C

import numpy as np
import pytest

import ref_norm as N
import ref_resample as RR

pytestmark = pytest.mark.gpu

CLLM_E_INVALID, CLLM_E_UNSUPPORTED = RR.CLLM_E_INVALID, RR.CLLM_E_UNSUPPORTED
SENT = RR.SENT
PAD_SOURCES = RR.pad_sources()
shared, declined = RR.shared, RR.declined


@pytest.mark.parametrize("at", [4, 5])
@pytest.mark.parametrize("i", range(len(PAD_SOURCES)), ids=[s[0] for s in PAD_SOURCES])
def test_pad(gpu, i, at):
    name, raw, view, p = PAD_SOURCES[i]
    want = shared(("pad", i), lambda: RR.pad_np(RR.gather(raw, view), p))
    src = RR.device_view(gpu, raw, view)
    got = RR.run_in_sentinel(gpu, lambda d: gpu.ops.pad(src, *p, dst=d), want.shape, at)
    N.assert_same_words(got, want, f"pad {name} at {at}")


@pytest.mark.parametrize("at", [4, 5])
@pytest.mark.parametrize("case", RR.REFLECT)
def test_pad_reflect_1d(gpu, case, at):
    x = RR.reflect_input(case)
    want = shared(("reflect", case), lambda: RR.pad_reflect_1d_np(x, case[1], case[2]))
    src = gpu.Tensor.from_numpy(x)
    got = RR.run_in_sentinel(gpu, lambda d: gpu.ops.pad_reflect_1d(src, case[1], case[2], dst=d), want.shape, at)
    N.assert_same_words(got, want, f"pad_reflect_1d {case} at {at}")


def test_the_mirrors_allocate_the_constructors_shapes(gpu):
    a = gpu.Tensor.from_numpy(np.arange(24, dtype=np.float32).reshape(2, 3, 4))
    assert gpu.ops.pad(a, 1, 2, 0, 1).ne == [7, 4, 2, 1]
    got = gpu.ops.pad_reflect_1d(a, 2, 1)
    assert got.ne == [7, 3, 2, 1] and got.numpy()[0, 0].tolist() == [2.0, 1.0, 0.0, 1.0, 2.0, 3.0, 2.0]


def test_an_empty_tensor_is_no_launch(gpu):
    assert gpu.ops.pad(gpu.Tensor(gpu.F32, [8, 0]), 1, 1).ne[:2] == [10, 0]
    assert gpu.ops.pad_reflect_1d(gpu.Tensor(gpu.F32, [8, 0]), 2, 2).ne[:2] == [12, 0]


# ---- what is declined -----------------------------------------------------------------------------------------------------------------------
def test_declines(gpu):
    """every refusal of the two entries, with its error word and an untouched destination.  (The circular form of PAD has no entry: the module's supports_op declines
    op_params[8] != 0.)"""
    a = gpu.Tensor.from_numpy(np.ones((2, 6, 8), np.float32))
    h = gpu.Tensor.from_numpy(np.ones((2, 6, 8), np.float16))
    d = np.full((2, 7, 11), SENT, np.float32)            # pads (1, 2, 0, 1)
    p = (1, 2, 0, 1, 0, 0, 0, 0)
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda t: gpu.ops.pad(h, *p, dst=t), d)
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda t: gpu.ops.pad(a, *p, dst=t), d.astype(np.float16))
    for k in range(8):
        q = list(p)
        q[k] = -1
        declined(gpu, CLLM_E_INVALID, "negative padding", lambda t: gpu.ops.pad(a, *q, dst=t), d)
    declined(gpu, CLLM_E_INVALID, "shape", lambda t: gpu.ops.pad(a, 1, 1, 0, 1, dst=t), d)
    declined(gpu, CLLM_E_INVALID, "shape", lambda t: gpu.ops.pad(a, 1, 2, 0, 1, 0, 1, dst=t), d)
    wide = gpu.Tensor.from_numpy(np.ones(4096, np.float32))
    declined(gpu, CLLM_E_UNSUPPORTED, "alignment", lambda t: gpu.ops.pad(wide.view([8, 6, 2], [6, 64, 512]), *p, dst=t), d)          # strides that are no whole floats
    back = gpu.Tensor.from_numpy(np.full(4096, SENT, np.float32))
    for call in (lambda: gpu.ops.pad(a, *p, dst=back.view([11, 7, 2], [4, 48, 480])),                    # a view with padded rows as destination
                 lambda: gpu.ops.pad_reflect_1d(a, 1, 2, dst=back.view([11, 6, 2], [4, 48, 480]))):
        with pytest.raises(gpu.lib.CllmError) as e:
            call()
        assert e.value.rc == CLLM_E_UNSUPPORTED and "contiguous" in str(e.value), str(e.value)
    # a source or a destination that does not start on a float
    odd = wide.view([8, 6, 2], [4, 32, 192], 2)
    declined(gpu, CLLM_E_UNSUPPORTED, "alignment", lambda t: gpu.ops.pad(odd, *p, dst=t), d)
    declined(gpu, CLLM_E_UNSUPPORTED, "alignment", lambda t: gpu.ops.pad_reflect_1d(odd, 1, 2, dst=t), np.full((2, 6, 11), SENT, np.float32))
    for call in (lambda: gpu.ops.pad(a, *p, dst=back.view([11, 7, 2], [4, 44, 308], 2)),
                 lambda: gpu.ops.pad_reflect_1d(a, 1, 2, dst=back.view([11, 6, 2], [4, 44, 264], 2))):
        with pytest.raises(gpu.lib.CllmError) as e:
            call()
        assert e.value.rc == CLLM_E_UNSUPPORTED and "alignment" in str(e.value), str(e.value)
    assert np.all(back.numpy() == SENT)

    r = np.full((2, 6, 11), SENT, np.float32)            # p0 1, p1 2
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda t: gpu.ops.pad_reflect_1d(h, 1, 2, dst=t), r)
    declined(gpu, CLLM_E_UNSUPPORTED, "type", lambda t: gpu.ops.pad_reflect_1d(a, 1, 2, dst=t), r.astype(np.float16))
    declined(gpu, CLLM_E_INVALID, "negative padding", lambda t: gpu.ops.pad_reflect_1d(a, -1, 2, dst=t), r)
    declined(gpu, CLLM_E_INVALID, "negative padding", lambda t: gpu.ops.pad_reflect_1d(a, 1, -2, dst=t), r)
    declined(gpu, CLLM_E_INVALID, "smaller than the row", lambda t: gpu.ops.pad_reflect_1d(a, 8, 0, dst=t), np.full((2, 6, 16), SENT, np.float32))
    declined(gpu, CLLM_E_INVALID, "smaller than the row", lambda t: gpu.ops.pad_reflect_1d(a, 0, 8, dst=t), np.full((2, 6, 16), SENT, np.float32))
    declined(gpu, CLLM_E_INVALID, "shape", lambda t: gpu.ops.pad_reflect_1d(a, 2, 2, dst=t), r)
    declined(gpu, CLLM_E_UNSUPPORTED, "contiguous", lambda t: gpu.ops.pad_reflect_1d(wide.view([8, 6, 2], [4, 40, 240]), 1, 2, dst=t), r)      # a view as source


def test_a_null_tensor_is_declined(gpu):
    a = gpu.Tensor.from_numpy(np.ones((2, 8), np.float32))
    L = gpu.lib.get()
    ca = a.c()
    assert L.cllm_op_pad(None, None, C.byref(ca), 0, 0, 0, 0, 0, 0, 0, 0) == CLLM_E_INVALID and b"null" in L.cllm_last_error()
    assert L.cllm_op_pad(None, C.byref(ca), None, 0, 0, 0, 0, 0, 0, 0, 0) == CLLM_E_INVALID
    assert L.cllm_op_pad_reflect_1d(None, None, C.byref(ca), 0, 0) == CLLM_E_INVALID and b"null" in L.cllm_last_error()
    assert L.cllm_op_pad_reflect_1d(None, C.byref(ca), None, 0, 0) == CLLM_E_INVALID
    assert np.array_equal(a.numpy(), np.ones((2, 8), np.float32))
