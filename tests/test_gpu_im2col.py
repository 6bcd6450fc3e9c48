"""GGML_OP_IM2COL on the device, through the C ABI (cllm_op_im2col) via the Python mirror (ops.im2col), against the reference's own CPU backend: the numpy restatement
of tests/ref_conv.py, which tests/test_conv_model.py shows equal to ggml_im2col on these very case lists.  Words are compared through a uint16 / uint32 view and 0
differing words are allowed (F16 NaNs included: the reference's rounding makes every NaN sign | 0x7e00, and so does the kernel).  The source buffer is poisoned beyond
its logical extent; the destination lies inside a buffer filled with a sentinel, which shows that every element is written, zeros included, and nothing around it.
What each list catches (predicted with the restatement): swapping s0 / s1, p0 / p1 or d0 / d1 fails the two asymmetric 2-D cases (the stems and the patch embedding
are symmetric and pass it: they are there for their shapes); in 1-D, dropping the dilation fails the six d0 = 2 cases, dropping the padding the ten p0 > 0 cases,
a stride of 1 the six s0 = 2 cases with OW > 1; reading N / IC from ne13 / ne12 in 1-D fails every 1-D case with IC or N > 1; a tail or an unaligned row stored as a
vector shows in the sentinel behind rows of 1, 3, 9 and 12 halves."""
import ctypes as C

import numpy as np
import pytest

import ref_conv as RC
import ref_ggml as R
from ref_ggml import GGML_TYPE_F16, GGML_TYPE_F32

pytestmark = pytest.mark.gpu

CLLM_E_INVALID, CLLM_E_UNSUPPORTED = -1, -2
SENT16, SENT32 = 0x5bcd, 0x5bcd1234
GUARD = 16                                # bytes of sentinel in front of the destination (keeps its 16-byte alignment) and behind it
_cache = {}


def shared(key, make):
    if key not in _cache:
        v = make()
        for a in v:
            a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


class KernelShape:
    """the kernel operand: read for its shape and type only -- its data pointer is null"""

    def __init__(self, gpu, type_, ne):
        self.gpu, self.type, self.ne = gpu, type_, [int(v) for v in ne] + [1] * (4 - len(ne))

    def c(self):
        t = self.gpu.lib.CTensor()
        es = 2 if self.type == GGML_TYPE_F16 else 4
        t.type = self.type
        t.ne[:] = self.ne
        t.nb[:] = [es, es * self.ne[0], es * self.ne[0] * self.ne[1], es * self.ne[0] * self.ne[1] * self.ne[2]]
        t.data = None
        return t


def source(gpu, x, ne):
    """x dense in a buffer with poison behind it"""
    flat = np.concatenate([np.ascontiguousarray(x, np.float32).reshape(-1), np.full(64, 1e30, np.float32)])
    return gpu.Tensor.from_numpy(flat).view(ne, [4, 4 * ne[0], 4 * ne[0] * ne[1], 4 * ne[0] * ne[1] * ne[2]])


def destination(gpu, dst_type, ne, shift=0):
    """a contiguous destination of shape ne inside a sentinel-filled buffer, `shift` bytes past the 16-byte aligned position; returns (tensor, read) where read()
    checks the sentinel on both sides and returns the words [ne3, ne2, ne1, ne0]"""
    dt, sent = (np.uint16, SENT16) if dst_type == GGML_TYPE_F16 else (np.uint32, SENT32)
    es = np.dtype(dt).itemsize
    n = int(np.prod(ne))
    assert shift % es == 0
    total = (2 * GUARD + shift) // es + n
    buf = gpu.Tensor.from_numpy(np.full(total, sent, dt).view(np.float16 if es == 2 else np.float32))
    dst = buf.view(ne, [es, es * ne[0], es * ne[0] * ne[1], es * ne[0] * ne[1] * ne[2]], GUARD + shift)

    def read():
        words = buf.numpy().view(dt)
        lo = (GUARD + shift) // es
        assert np.all(words[:lo] == sent) and np.all(words[lo + n:] == sent), "written outside the destination"
        return words[lo:lo + n].reshape(tuple(reversed(ne)))
    return dst, read


def check(gpu, x, sne, kne, p, is_2d, dst_type, want, src=None, shift=0):
    s0, s1, p0, p1, d0, d1 = p
    ne = RC.im2col_ne(kne + [1] * (4 - len(kne)), sne, s0, s1, p0, p1, d0, d1, is_2d)
    dst, read = destination(gpu, dst_type, ne, shift)
    kernel = KernelShape(gpu, GGML_TYPE_F16, kne)
    gpu.ops.im2col(kernel, src if src is not None else source(gpu, x, sne), s0, s1, p0, p1, d0, d1, is_2d, dst=dst)
    got = read()
    assert not np.any(got == (SENT16 if dst_type == GGML_TYPE_F16 else SENT32)), "an element was left unwritten"
    bad = int(np.count_nonzero(got != want.reshape(got.shape)))
    assert bad == 0, f"{bad} of {got.size} words differ"


def want_1d(case, dst_type, kind):
    IC, IW, KW, s0, p0, d0, N = case

    def make():
        x = RC.random_image((N, IC, IW), 11 + IW) if kind == "random" else RC.edge_image((N, IC, IW))
        return x, RC.im2col_np(x, 1, KW, s0, 0, p0, 0, d0, 0, False, dst_type)
    return shared(("1d", case, dst_type, kind), make)


def want_2d(case, dst_type, kind):
    IC, IH, IW, KH, KW, s0, s1, p0, p1, d0, d1, N = case

    def make():
        x = RC.random_image((N, IC, IH, IW), 13 + IW) if kind == "random" else RC.edge_image((N, IC, IH, IW))
        return x, RC.im2col_np(x, KH, KW, s0, s1, p0, p1, d0, d1, True, dst_type)
    return shared(("2d", case, dst_type, kind), make)


@pytest.mark.parametrize("dst_type", [GGML_TYPE_F16, GGML_TYPE_F32])
@pytest.mark.parametrize("case", RC.IM2COL_1D)
def test_im2col_1d(gpu, case, dst_type):
    IC, IW, KW, s0, p0, d0, N = case
    for kind in ("random", "edge"):
        x, want = want_1d(case, dst_type, kind)
        check(gpu, x, [IW, IC, N, 1], [KW, IC, 2], (s0, 0, p0, 0, d0, 0), False, dst_type, want)


@pytest.mark.parametrize("dst_type", [GGML_TYPE_F16, GGML_TYPE_F32])
@pytest.mark.parametrize("case", RC.IM2COL_2D)
def test_im2col_2d(gpu, case, dst_type):
    IC, IH, IW, KH, KW, s0, s1, p0, p1, d0, d1, N = case
    for kind in ("random", "edge"):
        x, want = want_2d(case, dst_type, kind)
        check(gpu, x, [IW, IH, IC, N], [KW, KH, IC, 2], (s0, s1, p0, p1, d0, d1), True, dst_type, want)


@pytest.mark.parametrize("dst_type,shift", [(GGML_TYPE_F16, 2), (GGML_TYPE_F16, 8), (GGML_TYPE_F32, 4)])
@pytest.mark.parametrize("case", [RC.IM2COL_1D[7], RC.IM2COL_2D[3]])
def test_a_destination_that_is_not_16_byte_aligned(gpu, case, dst_type, shift):
    """rows of 12 (1-D) and 27 (2-D) elements starting 2, 4 or 8 bytes off: no row may be stored as a vector where it does not start on 16 bytes"""
    if len(case) == 7:
        IC, IW, KW, s0, p0, d0, N = case
        x, want = want_1d(case, dst_type, "random")
        check(gpu, x, [IW, IC, N, 1], [KW, IC, 2], (s0, 0, p0, 0, d0, 0), False, dst_type, want, shift=shift)
    else:
        IC, IH, IW, KH, KW, s0, s1, p0, p1, d0, d1, N = case
        x, want = want_2d(case, dst_type, "random")
        check(gpu, x, [IW, IH, IC, N], [KW, KH, IC, 2], (s0, s1, p0, p1, d0, d1), True, dst_type, want, shift=shift)


@pytest.mark.parametrize("dst_type", [GGML_TYPE_F16, GGML_TYPE_F32])
def test_padded_channel_and_batch_strides(gpu, dst_type):
    """channels and batches apart by more than a plane, poison in between (1-D: nb[1] / nb[2]; 2-D: nb[2] / nb[3]): honoured as the reference honours them"""
    IC, IH, IW, N = 3, 5, 6, 2
    x = RC.random_image((N, IC, IH, IW), 5)
    buf = np.full((N, IC + 1, IH * IW + 7), 1e30, np.float32)
    buf[:, :IC, :IH * IW] = x.reshape(N, IC, -1)
    whole = gpu.Tensor.from_numpy(buf.reshape(-1))
    cs, bs = buf.shape[2] * 4, buf.shape[1] * buf.shape[2] * 4
    want = RC.im2col_np(x, 2, 3, 1, 2, 1, 0, 1, 1, True, dst_type)
    check(gpu, None, [IW, IH, IC, N], [3, 2, IC, 1], (1, 2, 1, 0, 1, 1), True, dst_type, want, src=whole.view([IW, IH, IC, N], [4, IW * 4, cs, bs]))
    x1 = x.reshape(N, IC, IH * IW)
    want = RC.im2col_np(x1, 1, 4, 2, 0, 3, 0, 2, 0, False, dst_type)
    check(gpu, None, [IH * IW, IC, N, 1], [4, IC, 1], (2, 0, 3, 0, 2, 0), False, dst_type, want, src=whole.view([IH * IW, IC, N, 1], [4, cs, bs, bs * N]))


def test_an_f32_kernel_with_an_f32_destination(gpu):
    """ggml_conv_2d with an F32 kernel: the F32 form needs no F16 kernel"""
    case = RC.IM2COL_2D[0]
    IC, IH, IW, KH, KW, s0, s1, p0, p1, d0, d1, N = case
    x, want = want_2d(case, GGML_TYPE_F32, "random")
    dst, read = destination(gpu, GGML_TYPE_F32, RC.im2col_ne([KW, KH, IC, 1], [IW, IH, IC, N], s0, s1, p0, p1, d0, d1, True))
    gpu.ops.im2col(KernelShape(gpu, GGML_TYPE_F32, [KW, KH, IC, 1]), source(gpu, x, [IW, IH, IC, N]), s0, s1, p0, p1, d0, d1, True, dst=dst)
    assert np.array_equal(read(), want)


def test_an_empty_tensor_is_no_launch(gpu):
    src = gpu.Tensor(gpu.F32, [7, 3, 0, 1])
    out = gpu.ops.im2col(KernelShape(gpu, GGML_TYPE_F16, [3, 3, 2]), src, 1, 0, 1, 0, 1, 0, False)
    assert out.ne == [9, 7, 0, 1]


# ---- what is declined: the code, a message, and the destination keeps the sentinel ------------------------------------------------------------
def declined(gpu, rc, word, kernel, src, dst, read, p, is_2d):
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.im2col(kernel, src, *p, is_2d, dst=dst)
    assert e.value.rc == rc and word in str(e.value), str(e.value)
    w = read()
    assert np.all(w == (SENT16 if w.dtype == np.uint16 else SENT32))


def _setup(gpu, dst_type=GGML_TYPE_F16, ne=None):
    x = RC.random_image((2, 3, 5, 6), 1)
    src = source(gpu, x, [6, 5, 3, 2])
    dst, read = destination(gpu, dst_type, ne or RC.im2col_ne([3, 2, 3, 1], [6, 5, 3, 2], 1, 1, 0, 0, 1, 1, True))
    return src, dst, read


def test_types_are_declined(gpu):
    src, dst, read = _setup(gpu)
    k16, k32 = KernelShape(gpu, GGML_TYPE_F16, [3, 2, 3, 1]), KernelShape(gpu, GGML_TYPE_F32, [3, 2, 3, 1])
    p = (1, 1, 0, 0, 1, 1)
    declined(gpu, CLLM_E_UNSUPPORTED, "type", k32, src, dst, read, p, True)                       # an F16 dst needs an F16 kernel (the reference's assert)
    h = gpu.Tensor.from_numpy(np.ones((2, 3, 5, 6), np.float16))
    declined(gpu, CLLM_E_UNSUPPORTED, "type", k16, h, dst, read, p, True)                         # an F16 source
    idst = gpu.Tensor(gpu.I32, dst.ne)
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.im2col(k16, src, *p, True, dst=idst)
    assert e.value.rc == CLLM_E_UNSUPPORTED and "type" in str(e.value)


def test_parameters_are_declined(gpu):
    src, dst, read = _setup(gpu)
    k = KernelShape(gpu, GGML_TYPE_F16, [3, 2, 3, 1])
    for p in [(0, 1, 0, 0, 1, 1), (1, 0, 0, 0, 1, 1), (1, 1, -1, 0, 1, 1), (1, 1, 0, -1, 1, 1), (1, 1, 0, 0, 0, 1), (1, 1, 0, 0, 1, 0)]:
        declined(gpu, CLLM_E_INVALID, "stride, padding or dilation", k, src, dst, read, p, True)


def test_shapes_are_declined(gpu):
    src, dst, read = _setup(gpu)
    p = (1, 1, 0, 0, 1, 1)
    declined(gpu, CLLM_E_INVALID, "shape", KernelShape(gpu, GGML_TYPE_F16, [3, 2, 4, 1]), src, dst, read, p, True)       # kernel->ne[2] != src->ne[2]
    declined(gpu, CLLM_E_INVALID, "shape", KernelShape(gpu, GGML_TYPE_F16, [3, 2, 3, 1]), src, dst, read, (2, 1, 0, 0, 1, 1), True)      # dst ne is not the rule's
    declined(gpu, CLLM_E_INVALID, "shape", KernelShape(gpu, GGML_TYPE_F16, [7, 2, 3, 1]), src, dst, read, p, True)       # the kernel is wider than the image
    # 1-D: kernel->ne[1] != src->ne[1]; src->ne[3] != 1
    declined(gpu, CLLM_E_INVALID, "shape", KernelShape(gpu, GGML_TYPE_F16, [3, 4, 1]), src, dst, read, (1, 0, 0, 0, 1, 0), False)
    declined(gpu, CLLM_E_INVALID, "shape", KernelShape(gpu, GGML_TYPE_F16, [3, 5, 1]), src, dst, read, (1, 0, 0, 0, 1, 0), False)


def test_views_are_declined(gpu):
    src, dst, read = _setup(gpu)
    k = KernelShape(gpu, GGML_TYPE_F16, [3, 2, 3, 1])
    p = (1, 1, 0, 0, 1, 1)
    x = gpu.Tensor.from_numpy(np.zeros(4096, np.float32))
    declined(gpu, CLLM_E_UNSUPPORTED, "dense", k, x.view([6, 5, 3, 2], [8, 48, 240, 720]), dst, read, p, True)           # nb[0] != 4
    declined(gpu, CLLM_E_UNSUPPORTED, "dense", k, x.view([6, 5, 3, 2], [4, 32, 160, 480]), dst, read, p, True)           # 2-D: nb[1] != IW * 4
    wide = gpu.Tensor.from_numpy(np.full(8192, 7.0, np.float16))
    ne = dst.ne
    padded = wide.view(ne, [2, 2 * ne[0] + 16, (2 * ne[0] + 16) * ne[1], (2 * ne[0] + 16) * ne[1] * ne[2]])
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.im2col(k, src, *p, True, dst=padded)
    assert e.value.rc == CLLM_E_UNSUPPORTED and "contiguous" in str(e.value)
    assert np.all(wide.numpy() == np.float16(7.0))


def test_a_null_tensor_is_declined(gpu):
    src, dst, read = _setup(gpu)
    L = gpu.lib.get()
    ck, cs, cd = KernelShape(gpu, GGML_TYPE_F16, [3, 2, 3, 1]).c(), src.c(), dst.c()
    for args in ((None, C.byref(cs), C.byref(cd)), (C.byref(ck), None, C.byref(cd)), (C.byref(ck), C.byref(cs), None)):
        assert L.cllm_op_im2col(None, *args, 1, 1, 0, 0, 1, 1, 1) == CLLM_E_INVALID
        assert b"null" in L.cllm_last_error()
    assert np.all(read() == SENT16)
