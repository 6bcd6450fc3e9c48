"""The reference's own CPU backend (ref_ggml.libs()) for the convolution nodes: ggml_im2col, ggml_pool_1d / _2d, ggml_mul_mat with an F16 src1, and the whole
ggml_conv_1d / ggml_conv_2d graphs followed by the bias ADD of Conv1D::forward / Conv2D::forward (src/layers.cpp:1864-1928).  Next to each: a numpy restatement of
the three index rules (im2col_np, pool_1d_np, pool_2d_np), which tests/test_conv_model.py shows equal to the reference on the case lists below, so that the GPU files
share one settled expectation; and those case lists.  Arrays are in numpy order (the reversed ne)."""
import ctypes as C

import numpy as np

import ref_ggml as R
from ref_ggml import GGML_TYPE_F16, GGML_TYPE_F32, View, _bytes, _graph, _new, _parent, _view

POOL_MAX, POOL_AVG = 0, 1
FLT_MAX = np.float32(3.4028234663852886e38)
_ready = False


def libs():
    global _ready
    base, cpu = R.libs()
    if not _ready:
        P, I = C.c_void_p, C.c_int
        base.ggml_im2col.restype, base.ggml_im2col.argtypes = P, [P, P, P, I, I, I, I, I, I, C.c_bool, I]
        base.ggml_pool_1d.restype, base.ggml_pool_1d.argtypes = P, [P, P, I, I, I, I]
        base.ggml_pool_2d.restype, base.ggml_pool_2d.argtypes = P, [P, P, I, I, I, I, I, C.c_float, C.c_float]
        base.ggml_conv_1d.restype, base.ggml_conv_1d.argtypes = P, [P, P, P, I, I, I]
        base.ggml_conv_2d.restype, base.ggml_conv_2d.argtypes = P, [P, P, P, I, I, I, I, I, I]
        base.ggml_add.restype, base.ggml_add.argtypes = P, [P, P, P]
        _ready = True
    return base, cpu


def conv_out(ins, ks, s, p, d):
    """ggml_calc_conv_output_size"""
    return (ins + 2 * p - d * (ks - 1) - 1) // s + 1


def pool_out(ins, ks, s, p):
    """ggml_calc_pool_output_size for an integer padding"""
    return (ins + 2 * p - ks) // s + 1


# ---- IM2COL -------------------------------------------------------------------------------------------------------------------------------
def im2col_ne(kne, sne, s0, s1, p0, p1, d0, d1, is_2d):
    """ggml_im2col's result ne"""
    ow = conv_out(sne[0], kne[0], s0, p0, d0)
    if is_2d:
        return [kne[2] * kne[1] * kne[0], ow, conv_out(sne[1], kne[1], s1, p1, d1), sne[3]]
    return [kne[1] * kne[0], ow, sne[2], 1]


def im2col(x_raw, x_view, kne, ktype, s0, s1, p0, p1, d0, d1, is_2d, dst_type):
    """ggml_im2col(kernel of shape kne and type ktype, the F32 view x_view of the float32 buffer x_raw, ...) -> the words of the result (uint16 for an F16 dst, uint32
    for F32), shaped [ne3, ne2, ne1, ne0]"""
    libs()
    x_raw = np.ascontiguousarray(x_raw, np.float32).reshape(-1)
    kne = [int(v) for v in kne] + [1] * (4 - len(kne))
    ne = im2col_ne(kne, x_view.ne, s0, s1, p0, p1, d0, d1, is_2d)
    dt = np.uint16 if dst_type == GGML_TYPE_F16 else np.uint32

    def build(base, ctx):
        k = base.ggml_new_tensor_4d(ctx, ktype, *kne)
        x = _view(base, ctx, _parent(base, ctx, GGML_TYPE_F32, _bytes(x_raw)), x_view)
        d = base.ggml_im2col(ctx, k, x, s0, s1, p0, p1, d0, d1, bool(is_2d), dst_type)
        return d, [(d, tuple(reversed(ne)), dt)]
    return _graph(x_raw.nbytes + 4 * int(np.prod(kne)) + 4 * int(np.prod(ne)) + (1 << 16), build)[0]


def half_words(x):
    """GGML_CPU_FP32_TO_FP16 of the reference's x86 build per element (ref_ggml.fp32_to_fp16), the shape of x"""
    x = np.ascontiguousarray(x, np.float32)
    return R.fp32_to_fp16(x).reshape(x.shape)


def im2col_np(x, kh, kw, s0, s1, p0, p1, d0, d1, is_2d, dst_type):
    """the index rule restated: x float32 [N, IC, IH, IW] (1-D: [N, IC, IW]) -> words [N, OH, OW, IC*KH*KW] (1-D: [1, N, OW, IC*KW])"""
    x = np.ascontiguousarray(x, np.float32)
    if not is_2d:
        x = x[:, :, None, :]
        kh, s1, p1, d1 = 1, 1, 0, 1
    N, IC, IH, IW = x.shape
    OW, OH = conv_out(IW, kw, s0, p0, d0), (conv_out(IH, kh, s1, p1, d1) if is_2d else 1)
    src = x.view(np.uint32)
    out = np.zeros((N, OH, OW, IC, kh, kw), np.uint32)
    for ikh in range(kh):
        for ikw in range(kw):
            ih = np.arange(OH) * s1 + ikh * d1 - p1
            iw = np.arange(OW) * s0 + ikw * d0 - p0
            oh, ow = np.nonzero((ih >= 0) & (ih < IH))[0], np.nonzero((iw >= 0) & (iw < IW))[0]
            if len(oh) and len(ow):
                out[..., ikh, ikw][np.ix_(np.arange(N), oh, ow, np.arange(IC))] = src[:, :, ih[oh]][:, :, :, iw[ow]].transpose(0, 2, 3, 1)
    out = out.reshape(N, OH, OW, IC * kh * kw)
    if dst_type == GGML_TYPE_F16:
        out = half_words(out.view(np.float32))
    return out if is_2d else out.reshape(1, N, OW, IC * kw)


# (IC, IW, KW, s0, p0, d0, N): IC 1 / 3, IW 1 / 7 / 64 / 65, KW 1 / 3 / 4, s0 1 / 2, p0 0 / 1 / KW - 1, d0 1 / 2, N 1 / 2; row lengths IC*KW of 1, 3, 4, 9, 12 (either side of 8,
# multiples of 4 and not); OW == 1 (the first and the last two)
IM2COL_1D = [
    (1, 1, 1, 1, 0, 1, 1), (1, 7, 3, 1, 0, 1, 1), (3, 7, 3, 1, 1, 1, 2), (3, 7, 3, 2, 2, 1, 1), (1, 7, 4, 2, 3, 2, 2), (3, 7, 4, 1, 1, 2, 1),
    (1, 64, 3, 1, 1, 1, 2), (3, 64, 4, 2, 0, 1, 1), (3, 64, 1, 1, 0, 1, 2), (1, 65, 4, 1, 3, 2, 1), (3, 65, 3, 2, 1, 2, 2), (3, 65, 4, 2, 3, 1, 2),
    (3, 1, 3, 1, 1, 1, 1), (3, 7, 4, 2, 0, 2, 2),
]
# (IC, IH, IW, KH, KW, s0, s1, p0, p1, d0, d1, N): everything asymmetric; the patch embedding (K == S == 14, 28x42, no overlap, no padding); the stems K3 s1 p1 and K3 s2 p1
IM2COL_2D = [
    (2, 9, 13, 2, 3, 2, 1, 1, 2, 1, 2, 2),
    (1, 6, 5, 3, 2, 1, 2, 0, 1, 2, 1, 1),
    (3, 28, 42, 14, 14, 14, 14, 0, 0, 1, 1, 1),
    (3, 10, 11, 3, 3, 1, 1, 1, 1, 1, 1, 2),
    (3, 10, 11, 3, 3, 2, 2, 1, 1, 1, 1, 1),
]


def random_image(shape, seed):
    return (np.random.default_rng(seed).standard_normal(shape) * 3.0).astype(np.float32)


def edge_image(shape):
    """+-0, subnormals, values that overflow F16, values on F16 rounding ties, NaNs with payloads, +-inf (ref_ggml.special_values), repeated over the image"""
    v = R.special_values()
    return np.resize(v, int(np.prod(shape))).reshape(shape).astype(np.float32)


# ---- POOL ---------------------------------------------------------------------------------------------------------------------------------
def pool_1d(x, op, k0, s0, p0):
    """ggml_pool_1d over a dense float32 x [ne3, ne2, ne1, IW] -> float32 [.., OW]"""
    libs()
    x = np.ascontiguousarray(x, np.float32)
    shape = x.shape[:-1] + (pool_out(x.shape[-1], k0, s0, p0),)

    def build(base, ctx):
        d = base.ggml_pool_1d(ctx, _new(base, ctx, x), op, k0, s0, p0)
        return d, [(d, shape, np.float32)]
    return _graph(2 * x.nbytes + 4 * int(np.prod(shape)) + (1 << 16), build)[0]


def pool_2d(x, op, k0, k1, s0, s1, p0, p1):
    """ggml_pool_2d over a dense float32 x [ne3, ne2, IH, IW] -> float32 [.., OH, OW]"""
    libs()
    x = np.ascontiguousarray(x, np.float32)
    shape = x.shape[:-2] + (pool_out(x.shape[-2], k1, s1, p1), pool_out(x.shape[-1], k0, s0, p0))

    def build(base, ctx):
        d = base.ggml_pool_2d(ctx, _new(base, ctx, x), op, k0, k1, s0, s1, C.c_float(p0), C.c_float(p1))
        return d, [(d, shape, np.float32)]
    return _graph(2 * x.nbytes + 4 * int(np.prod(shape)) + (1 << 16), build)[0]


def _pool_np(x, op, k0, k1, s0, s1, p0, p1, by_count):
    x = np.ascontiguousarray(x, np.float32)
    IH, IW = x.shape[-2:]
    OH, OW = pool_out(IH, k1, s1, p1), pool_out(IW, k0, s0, p0)
    planes = x.reshape(-1, IH, IW)
    out = np.empty((planes.shape[0], OH, OW), np.float32)
    with np.errstate(all="ignore"):
        for oy in range(OH):
            for ox in range(OW):
                res = np.full(planes.shape[0], 0.0 if op == POOL_AVG else -FLT_MAX, np.float32)
                count = 0
                for ky in range(k1):
                    iy = oy * s1 - p1 + ky
                    if iy < 0 or iy >= IH:
                        continue
                    for kx in range(k0):
                        ix = ox * s0 - p0 + kx
                        if ix < 0 or ix >= IW:
                            continue
                        v = planes[:, iy, ix]
                        res = (res + v).astype(np.float32) if op == POOL_AVG else np.where(v < res, res, v)      # std::max(v, res)
                        count += 1
                if op == POOL_AVG:
                    res = (res / np.float32(count) if count else np.zeros_like(res)) if by_count else res / np.float32(k0 * k1)
                out[:, oy, ox] = res
    return out.reshape(x.shape[:-2] + (OH, OW))


def pool_1d_np(x, op, k0, s0, p0):
    x = np.ascontiguousarray(x, np.float32)
    return _pool_np(x[..., None, :], op, k0, 1, s0, 1, p0, 0, True)[..., 0, :]


def pool_2d_np(x, op, k0, k1, s0, s1, p0, p1):
    return _pool_np(x, op, k0, k1, s0, s1, p0, p1, False)


# (IW, k0, s0, p0): k 1 / 2 / 3, s != k, p 0 / 1, a last window partly outside ((7, 3, 2, 1): base 5, positions 5, 6, 7; (8, 3, 3, 1): base 5 .. 7 inside, first window starts at -1)
POOL_1D = [(7, 1, 2, 0), (7, 2, 1, 0), (7, 2, 3, 1), (7, 3, 2, 1), (8, 3, 3, 1), (65, 3, 2, 0), (6, 2, 2, 1)]
# (IH, IW, k0, k1, s0, s1, p0, p1)
POOL_2D = [(5, 7, 2, 3, 1, 2, 1, 0), (6, 9, 3, 2, 2, 1, 0, 1), (4, 4, 2, 2, 2, 2, 0, 0), (5, 5, 3, 3, 2, 2, 1, 1), (7, 6, 3, 2, 3, 1, 1, 0)]


def pool_input(shape, seed):
    """values on which the order of the sum decides a float: large magnitudes of alternating sign next to small ones"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    big = (rng.integers(0, 2, size=shape) * 2 - 1) * np.float32(2.0 ** 24) * rng.integers(1, 4, size=shape)
    return np.where(rng.random(shape) < 0.5, big.astype(np.float32) + x, x).astype(np.float32)


# ---- MUL_MAT with an F16 src1 -------------------------------------------------------------------------------------------------------------
def mul_mat_f16(w_raw, w_view, x_raw, x_view):
    """ggml_mul_mat(w, x) of an F16 view of the uint16 buffer w_raw and an F16 view of the uint16 buffer x_raw -> float32 [x.ne[3], x.ne[2], x.ne[1], w.ne[1]]"""
    libs()
    assert w_view.type == GGML_TYPE_F16 and x_view.type == GGML_TYPE_F16
    w_raw, x_raw = _bytes(np.ascontiguousarray(w_raw, np.uint16)), _bytes(np.ascontiguousarray(x_raw, np.uint16))
    shape = (x_view.ne[3], x_view.ne[2], x_view.ne[1], w_view.ne[1])

    def build(base, ctx):
        w = _view(base, ctx, _parent(base, ctx, GGML_TYPE_F16, w_raw), w_view)
        x = _view(base, ctx, _parent(base, ctx, GGML_TYPE_F16, x_raw), x_view)
        out = base.ggml_mul_mat(ctx, w, x)
        return out, [(out, shape, np.float32)]
    return _graph(w_raw.nbytes + 3 * x_raw.nbytes + 4 * int(np.prod(shape)) + (1 << 20), build)[0]


def padded_rows(a, pad, poison=0x7bff):
    """a uint16 [.., rows, K] -> (buffer uint16 with `pad` poison halves behind every row, the F16 View of the rows in it)"""
    a = np.ascontiguousarray(a, np.uint16)
    a4 = a.reshape((1,) * (4 - a.ndim) + a.shape)
    buf = np.full(a4.shape[:-1] + (a4.shape[-1] + pad,), poison, np.uint16)
    buf[..., :a4.shape[-1]] = a4
    K, rs = a4.shape[-1], (a4.shape[-1] + pad) * 2
    ne = [K, a4.shape[2], a4.shape[1], a4.shape[0]]
    return buf.reshape(-1), View(GGML_TYPE_F16, ne, [2, rs, rs * ne[1], rs * ne[1] * ne[2]])


def dense_view(a, type_=GGML_TYPE_F16):
    a4 = a.reshape((1,) * (4 - a.ndim) + a.shape)
    return View(type_, list(reversed(a4.shape)))


def halves(shape, seed, scale=1.0):
    """random fp16 values as uint16 words"""
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float16).view(np.uint16)


def edge_halves(shape, seed):
    """fp16 operands [rows, K] with edge values among ordinary ones: +-0, subnormals and the largest finite values anywhere; +-inf and NaNs in row 0 alone, so that the
    other rows' products stay finite"""
    h = halves(shape, seed).copy()
    edge = np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x0400, 0x7bff, 0xfbff, 0x3c00, 0xbc00], np.uint16)
    flat = h.reshape(-1)
    idx = np.random.default_rng(seed + 1).choice(flat.size, size=flat.size // 3 + 1, replace=False)
    flat[idx] = np.resize(edge, idx.size)
    h[0, :4] = [0x7c00, 0xfc00, 0x7e00, 0xfe01]
    return h


# ---- the whole convolutions ----------------------------------------------------------------------------------------------------------------
def conv_1d_bias(kernel, ktype, x, bias, s, p, d):
    """ggml_conv_1d(kernel [OC, IC, K] (float16 words as uint16), x float32 [N, IC, IW], s, p, d) + the bias as a [1, OC] tensor -> float32 [N, OC, OL]"""
    libs()
    assert ktype == GGML_TYPE_F16
    x, bias = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(bias, np.float32)
    OC, IC, K = kernel.shape
    shape = (x.shape[0], OC, conv_out(x.shape[2], K, s, p, d))

    def build(base, ctx):
        k = _new(base, ctx, np.ascontiguousarray(kernel), ktype)
        out = base.ggml_conv_1d(ctx, k, _new(base, ctx, x), s, p, d)
        out = base.ggml_add(ctx, out, _new(base, ctx, bias.reshape(OC, 1)))
        return out, [(out, shape, np.float32)]
    return _graph(8 * (kernel.nbytes + x.nbytes + 4 * int(np.prod(shape)) * IC * K) + (1 << 20), build)[0]


def conv_2d_bias(kernel, ktype, x, bias, s0, s1, p0, p1, d0, d1):
    """ggml_conv_2d(kernel [OC, IC, KH, KW] (uint16 words of F16, or float32), x float32 [N, IC, IH, IW], ...) + the bias as a [1, 1, OC] tensor -> float32 [N, OC, OH, OW]"""
    libs()
    x, bias = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(bias, np.float32)
    OC, IC, KH, KW = kernel.shape
    shape = (x.shape[0], OC, conv_out(x.shape[2], KH, s1, p1, d1), conv_out(x.shape[3], KW, s0, p0, d0))

    def build(base, ctx):
        k = _new(base, ctx, np.ascontiguousarray(kernel), ktype)
        out = base.ggml_conv_2d(ctx, k, _new(base, ctx, x), s0, s1, p0, p1, d0, d1)
        out = base.ggml_add(ctx, out, _new(base, ctx, bias.reshape(OC, 1, 1)))
        return out, [(out, shape, np.float32)]
    return _graph(8 * (kernel.nbytes + x.nbytes + 4 * int(np.prod(shape)) * IC * KH * KW) + (1 << 20), build)[0]
