"""The reference's own CPU backend (oracle/_ref/libggml-cpu.so over libggml-base.so, built from the reference by oracle/Makefile) driven
through its public ggml C API with ctypes: ggml_init, ggml_new_tensor_4d, the op constructor, ggml_build_forward_expand,
ggml_graph_compute_with_ctx.  The oracle of the element-wise ops that oracle/ref_ops.c does not expose (TANH, RELU, SIGMOID, GELU,
GELU_QUICK, SQR), of SCALE with a bias, broadcast ADD / MUL / DIV, DIAG_MASK_INF and of ROPE over a view (ggml_view_4d), out of place and
in place; of SET_ROWS, CPY / CONT, GET_ROWS between views (ggml_view_4d, ggml_permute, ggml_transpose), of SOFT_MAX with a mask tensor and of
MUL_MAT between views of a weight buffer and of a src1 buffer.
Also: the input sets the CPU and the GPU tests of the unary ops share."""
import ctypes as C
import os

import numpy as np

from conftest import load_package

_tensor = load_package().tensor

REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref")
GGML_TYPE_F32 = 0
# the codes of cllm_unary (== enum ggml_unary_op); SQR is an op of its own (GGML_OP_SQR)
TANH, RELU, SIGMOID, GELU, GELU_QUICK, SQR = 4, 6, 7, 8, 9, -1
OPS = {"tanh": TANH, "relu": RELU, "sigmoid": SIGMOID, "gelu": GELU, "gelu_quick": GELU_QUICK, "sqr": SQR}
_CTOR = {TANH: "ggml_tanh", RELU: "ggml_relu", SIGMOID: "ggml_sigmoid", GELU: "ggml_gelu", GELU_QUICK: "ggml_gelu_quick", SQR: "ggml_sqr"}
_BINARY = {"add": "ggml_add", "mul": "ggml_mul", "div": "ggml_div"}
GGML_TYPE_I32 = 26
GGML_TYPE_F16, GGML_TYPE_Q8_0, GGML_TYPE_I64 = 1, 8, 27
# (bytes of a block, elements of a block) of the types the data-movement entry points take: ggml.c type_traits
_BLOCK = {t: (_tensor.TYPE_SIZE[t], _tensor.BLCK[t]) for t in _tensor.TYPE_SIZE}


class _InitParams(C.Structure):
    _fields_ = [("mem_size", C.c_size_t), ("mem_buffer", C.c_void_p), ("no_alloc", C.c_bool)]


_libs = None


def available():
    return os.path.exists(os.path.join(REF, "libggml-base.so")) and os.path.exists(os.path.join(REF, "libggml-cpu.so"))


def libs():
    """(libggml-base, libggml-cpu) with the prototypes this file uses"""
    global _libs
    if _libs is None:
        if not available():
            raise RuntimeError(f"{REF}/libggml-cpu.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` where the reference lies")
        base = C.CDLL(os.path.join(REF, "libggml-base.so"), mode=C.RTLD_GLOBAL)
        cpu = C.CDLL(os.path.join(REF, "libggml-cpu.so"), mode=C.RTLD_GLOBAL)
        P = C.c_void_p
        base.ggml_init.restype, base.ggml_init.argtypes = P, [_InitParams]
        base.ggml_free.restype, base.ggml_free.argtypes = None, [P]
        base.ggml_new_tensor_4d.restype, base.ggml_new_tensor_4d.argtypes = P, [P, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64]
        base.ggml_get_data.restype, base.ggml_get_data.argtypes = P, [P]
        base.ggml_new_graph.restype, base.ggml_new_graph.argtypes = P, [P]
        base.ggml_build_forward_expand.restype, base.ggml_build_forward_expand.argtypes = None, [P, P]
        base.ggml_tensor_overhead.restype, base.ggml_graph_overhead.restype = C.c_size_t, C.c_size_t
        for name in _CTOR.values():
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P]
        for name in _BINARY.values():
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P, P]
        base.ggml_scale_bias.restype, base.ggml_scale_bias.argtypes = P, [P, P, C.c_float, C.c_float]
        base.ggml_diag_mask_inf.restype, base.ggml_diag_mask_inf.argtypes = P, [P, P, C.c_int]
        base.ggml_view_4d.restype, base.ggml_view_4d.argtypes = P, [P, P] + [C.c_int64] * 4 + [C.c_size_t] * 4
        base.ggml_permute.restype, base.ggml_permute.argtypes = P, [P, P] + [C.c_int] * 4
        base.ggml_transpose.restype, base.ggml_transpose.argtypes = P, [P, P]
        base.ggml_new_tensor_1d.restype, base.ggml_new_tensor_1d.argtypes = P, [P, C.c_int, C.c_int64]
        for name in ("ggml_set_rows",):
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P, P, P]
        for name in ("ggml_cpy", "ggml_get_rows", "ggml_mul_mat"):
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P, P]
        base.ggml_cont.restype, base.ggml_cont.argtypes = P, [P, P]
        for name in ("ggml_soft_max_ext", "ggml_soft_max_ext_inplace"):
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P, P, C.c_float, C.c_float]
        for name in ("ggml_rope_ext", "ggml_rope_ext_inplace"):
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P, P, P, C.c_int, C.c_int, C.c_int] + [C.c_float] * 6
        cpu.ggml_cpu_init.restype, cpu.ggml_cpu_init.argtypes = None, []
        cpu.ggml_graph_compute_with_ctx.restype, cpu.ggml_graph_compute_with_ctx.argtypes = C.c_int, [P, P, C.c_int]
        base.ggml_fp32_to_fp16_row.restype, base.ggml_fp32_to_fp16_row.argtypes = None, [P, P, C.c_int64]
        base.ggml_fp16_to_fp32_row.restype, base.ggml_fp16_to_fp32_row.argtypes = None, [P, P, C.c_int64]
        cpu.ggml_cpu_init()                 # fills ggml_table_gelu_f16 / ggml_table_gelu_quick_f16 (ggml-cpu.c:3694-3703)
        _libs = (base, cpu)
    return _libs


def unary(op, x):
    """the reference's result of one op node over x (float32, up to 4 dimensions, numpy order = reversed ne), same shape"""
    base, cpu = libs()
    x = np.ascontiguousarray(x, np.float32)
    ne = list(reversed(x.shape)) + [1] * (4 - x.ndim)
    mem = 2 * x.nbytes + 8 * base.ggml_tensor_overhead() + base.ggml_graph_overhead() + (1 << 16)
    ctx = base.ggml_init(_InitParams(mem, None, False))
    assert ctx
    try:
        a = base.ggml_new_tensor_4d(ctx, GGML_TYPE_F32, *ne)
        C.memmove(base.ggml_get_data(a), x.ctypes.data, x.nbytes)
        d = getattr(base, _CTOR[op])(ctx, a)
        g = base.ggml_new_graph(ctx)
        base.ggml_build_forward_expand(g, d)
        assert cpu.ggml_graph_compute_with_ctx(ctx, g, 1) == 0
        out = np.empty_like(x)
        C.memmove(out.ctypes.data, base.ggml_get_data(d), x.nbytes)
        return out
    finally:
        base.ggml_free(ctx)


def _ne(x):
    """ne[4] of a numpy array of up to 4 dimensions (numpy order = reversed ne)"""
    return list(reversed(x.shape)) + [1] * (4 - x.ndim)


def _new(base, ctx, x, type_=GGML_TYPE_F32):
    """a dense tensor of the context holding x"""
    t = base.ggml_new_tensor_4d(ctx, type_, *_ne(x))
    C.memmove(base.ggml_get_data(t), x.ctypes.data, x.nbytes)
    return t


def _graph(nbytes, build):
    """one context, one graph of the node build(base, ctx) returns, one thread; build's second result says what to read back (a list of
    (tensor, shape, dtype)); returns those arrays"""
    base, cpu = libs()
    mem = nbytes + 32 * base.ggml_tensor_overhead() + base.ggml_graph_overhead() + (1 << 16)
    ctx = base.ggml_init(_InitParams(mem, None, False))
    assert ctx
    try:
        d, reads = build(base, ctx)
        g = base.ggml_new_graph(ctx)
        base.ggml_build_forward_expand(g, d)
        assert cpu.ggml_graph_compute_with_ctx(ctx, g, 1) == 0
        outs = []
        for t, shape, dtype in reads:
            out = np.empty(shape, dtype)
            C.memmove(out.ctypes.data, base.ggml_get_data(t), out.nbytes)
            outs.append(out)
        return outs
    finally:
        base.ggml_free(ctx)


def scale_bias(x, s, b):
    """ggml_scale_bias(x, s, b): x * s + b as the reference's SCALE node computes it (ggml_vec_scale_f32 when b == 0, ggml_vec_mad1_f32 per row
    otherwise), same shape"""
    x = np.ascontiguousarray(x, np.float32)

    def build(base, ctx):
        d = base.ggml_scale_bias(ctx, _new(base, ctx, x), C.c_float(s), C.c_float(b))
        return d, [(d, x.shape, np.float32)]
    return _graph(2 * x.nbytes, build)[0]


def binary(op, a, b):
    """ggml_add / ggml_mul / ggml_div (op: "add", "mul", "div") of a and a b that repeats into a (ggml_can_repeat: every ne of a is a multiple
    of b's); both dense; the shape of a"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)

    def build(base, ctx):
        d = getattr(base, _BINARY[op])(ctx, _new(base, ctx, a), _new(base, ctx, b))
        return d, [(d, a.shape, np.float32)]
    return _graph(2 * a.nbytes + b.nbytes, build)[0]


def diag_mask_inf(x, n_past):
    """ggml_diag_mask_inf(x, n_past): -inf where i0 > n_past + i1"""
    x = np.ascontiguousarray(x, np.float32)

    def build(base, ctx):
        d = base.ggml_diag_mask_inf(ctx, _new(base, ctx, x), n_past)
        return d, [(d, x.shape, np.float32)]
    return _graph(2 * x.nbytes, build)[0]


ROPE_DEFAULTS = dict(n_ctx_orig=0, freq_base=10000.0, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=0.0, beta_slow=0.0)


def rope(parent, view_ne, view_nb, view_offset, pos, ff, params, inplace):
    """ggml_rope_ext (or ggml_rope_ext_inplace) over ggml_view_4d(parent, view_ne, view_nb[1..3], view_offset) of a dense float32 parent.
    pos: int32 [view_ne[2]]; ff: the frequency factors, float32 [>= n_dims / 2], or None; params: n_dims, mode and any of ROPE_DEFAULTS.
    Returns (the result as a dense array of shape reversed(view_ne), the parent's buffer after the run); in place the result is the view's
    content read out of that buffer"""
    parent = np.ascontiguousarray(parent, np.float32)
    pos = np.ascontiguousarray(pos, np.int32)
    ff = None if ff is None else np.ascontiguousarray(ff, np.float32)
    ne = [int(v) for v in view_ne] + [1] * (4 - len(view_ne))
    nb = [int(v) for v in view_nb]
    p = dict(ROPE_DEFAULTS, **params)
    shape = tuple(reversed(ne))

    def build(base, ctx):
        par = _new(base, ctx, parent)
        v = base.ggml_view_4d(ctx, par, ne[0], ne[1], ne[2], ne[3], nb[1], nb[2], nb[3], view_offset)
        tp = _new(base, ctx, pos, GGML_TYPE_I32)
        tf = _new(base, ctx, ff) if ff is not None else None
        ctor = base.ggml_rope_ext_inplace if inplace else base.ggml_rope_ext
        d = ctor(ctx, v, tp, tf, p["n_dims"], p["mode"], p["n_ctx_orig"], p["freq_base"], p["freq_scale"], p["ext_factor"], p["attn_factor"],
                 p["beta_fast"], p["beta_slow"])
        return d, [(par, parent.shape, np.float32)] + ([] if inplace else [(d, shape, np.float32)])
    outs = _graph(2 * parent.nbytes + pos.nbytes + (ff.nbytes if ff is not None else 0) + 4 * (ne[0] + 64), build)
    after = outs[0]
    if inplace:
        result = np.lib.stride_tricks.as_strided(after.reshape(-1)[view_offset // 4:], shape, (nb[3], nb[2], nb[1], nb[0])).copy()
    else:
        result = outs[1]
    return result, after


# ---- SET_ROWS, CPY / CONT, GET_ROWS, SOFT_MAX with a mask ----------------------------------------------------------------------------
def row_bytes(type_, ne0):
    """ggml_row_size"""
    size, blck = _BLOCK[type_]
    assert ne0 % blck == 0, (type_, ne0)
    return size * (ne0 // blck)


class View:
    """ggml_view_4d(parent, ne, nb[1..3], offset), then ggml_permute(axes) when axes is given (ggml_transpose for "transpose"): the description the
    reference, the oracle and the device tensors are all built from.  nb defaults to dense rows of `ne`"""

    def __init__(self, type_, ne, nb=None, offset=0, axes=None):
        self.type = type_
        self.ne = [int(v) for v in ne] + [1] * (4 - len(ne))
        if nb is None:
            nb = [_BLOCK[type_][0], row_bytes(type_, self.ne[0])]
            nb += [nb[1] * self.ne[1], nb[1] * self.ne[1] * self.ne[2]]
        self.nb = [int(v) for v in nb]
        assert len(self.nb) == 4 and self.nb[0] == _BLOCK[type_][0]
        self.offset, self.axes = int(offset), axes

    def final(self):
        """(ne, nb) after the permutation: dimension i of the view becomes dimension axes[i] of the result (ggml_permute)"""
        axes = (1, 0, 2, 3) if self.axes == "transpose" else self.axes
        if axes is None:
            return list(self.ne), list(self.nb)
        ne, nb = [0] * 4, [0] * 4
        for i, a in enumerate(axes):
            ne[a], nb[a] = self.ne[i], self.nb[i]
        return ne, nb

    def nelements(self):
        return int(np.prod(self.ne))

    def __repr__(self):
        return f"View({self.type}, {self.ne}, {self.nb}, {self.offset}, {self.axes})"


def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _parent(base, ctx, type_, raw):
    """a 1-D tensor of `type_` over a copy of the bytes `raw`: the buffer the views are cut from"""
    size, blck = _BLOCK[type_]
    assert raw.nbytes % size == 0, (type_, raw.nbytes)
    t = base.ggml_new_tensor_1d(ctx, type_, raw.nbytes // size * blck)
    C.memmove(base.ggml_get_data(t), raw.ctypes.data, raw.nbytes)
    return t


def _view(base, ctx, parent, v):
    t = base.ggml_view_4d(ctx, parent, v.ne[0], v.ne[1], v.ne[2], v.ne[3], v.nb[1], v.nb[2], v.nb[3], v.offset)
    if v.axes == "transpose":
        t = base.ggml_transpose(ctx, t)
    elif v.axes is not None:
        t = base.ggml_permute(ctx, t, *v.axes)
    return t


def set_rows(dst0, dst_view, src, src_view, idx):
    """ggml_set_rows(dst, src, idx).  dst0: the bytes of the destination's whole buffer; dst_view: the destination inside it (F32, F16 or Q8_0; a
    view at an offset with padded rows, or the whole buffer); src: the float32 buffer the source is a ggml_view_4d of (src_view; rows may be
    padded: nb[1] > ne0 * 4); idx: a dense int32 or int64 array of 1 to 3 dimensions (numpy order), which broadcasts over ne[2] and ne[3].
    Returns the whole destination buffer afterwards, as bytes"""
    dst0, src = _bytes(dst0), np.ascontiguousarray(src, np.float32).reshape(-1)
    assert idx.dtype in (np.int32, np.int64) and 1 <= idx.ndim <= 3
    idx = np.ascontiguousarray(idx)
    it = GGML_TYPE_I64 if idx.dtype == np.int64 else GGML_TYPE_I32

    def build(base, ctx):
        d = _parent(base, ctx, dst_view.type, dst0)
        s = _parent(base, ctx, GGML_TYPE_F32, _bytes(src))
        out = base.ggml_set_rows(ctx, _view(base, ctx, d, dst_view), _view(base, ctx, s, src_view), _new(base, ctx, idx, it))
        return out, [(d, dst0.shape, np.uint8)]
    return _graph(dst0.nbytes + src.nbytes + idx.nbytes + (1 << 16), build)[0]


def cpy(src0, src_view, dst0, dst_view):
    """ggml_cpy(src, dst) between two views of two buffers given as bytes; dst0 None: ggml_cont(src), a dense tensor of the permuted view's shape.
    Returns the destination's whole buffer afterwards, as bytes"""
    src0 = _bytes(src0)
    dst0 = None if dst0 is None else _bytes(dst0)
    ne, _ = src_view.final()
    n_out = row_bytes(src_view.type, ne[0]) * ne[1] * ne[2] * ne[3] if dst0 is None else dst0.nbytes

    def build(base, ctx):
        s = _view(base, ctx, _parent(base, ctx, src_view.type, src0), src_view)
        if dst0 is None:
            out = base.ggml_cont(ctx, s)
            return out, [(out, (n_out,), np.uint8)]
        d = _parent(base, ctx, dst_view.type, dst0)
        out = base.ggml_cpy(ctx, s, _view(base, ctx, d, dst_view))
        return out, [(d, dst0.shape, np.uint8)]
    return _graph(src0.nbytes + n_out + (1 << 20), build)[0]


def get_rows(table, type_, ne, idx0, idx_view):
    """ggml_get_rows(table, idx): table: the bytes of a dense tensor of `type_` and shape ne [ne0, rows, ne2, ne3]; idx: an I32 view (1 to 3
    dimensions, idx.ne[1] == ne2, idx.ne[2] == ne3: the batched form) of the int32 buffer idx0.  Returns float32 [idx.ne[2], idx.ne[1], idx.ne[0], ne0]"""
    table, idx0 = _bytes(table), np.ascontiguousarray(idx0, np.int32).reshape(-1)
    ne = [int(v) for v in ne] + [1] * (4 - len(ne))
    ine, _ = idx_view.final()
    shape = (ine[2], ine[1], ine[0], ne[0])

    def build(base, ctx):
        t = base.ggml_new_tensor_4d(ctx, type_, *ne)
        assert row_bytes(type_, ne[0]) * ne[1] * ne[2] * ne[3] == table.nbytes
        C.memmove(base.ggml_get_data(t), table.ctypes.data, table.nbytes)
        out = base.ggml_get_rows(ctx, t, _view(base, ctx, _parent(base, ctx, GGML_TYPE_I32, _bytes(idx0)), idx_view))
        return out, [(out, shape, np.float32)]
    return _graph(table.nbytes + idx0.nbytes + 4 * int(np.prod(shape)) + (1 << 16), build)[0]


def mul_mat(w_raw, w_view, x_raw, x_view):
    """ggml_mul_mat(w, x) of two views of two buffers given as bytes: w_view any weight type (rows nb[1] apart, matrices nb[2] / nb[3] apart, at an offset), x_view F32.
    A buffer that is no whole number of blocks of its type is lengthened with 0x7f bytes.  Returns the node's dense result, float32 [x.ne[3], x.ne[2], x.ne[1], w.ne[1]]"""
    def whole(raw, type_):
        raw, size = _bytes(raw), _BLOCK[type_][0]
        return raw if raw.nbytes % size == 0 else np.concatenate([raw, np.full(size - raw.nbytes % size, 0x7f, np.uint8)])
    w_raw, x_raw = whole(w_raw, w_view.type), whole(x_raw, GGML_TYPE_F32)
    assert x_view.type == GGML_TYPE_F32 and w_view.axes is None
    xne, _ = x_view.final()
    shape = (xne[3], xne[2], xne[1], w_view.ne[1])

    def build(base, ctx):
        w = _view(base, ctx, _parent(base, ctx, w_view.type, w_raw), w_view)
        x = _view(base, ctx, _parent(base, ctx, GGML_TYPE_F32, x_raw), x_view)
        out = base.ggml_mul_mat(ctx, w, x)
        return out, [(out, shape, np.float32)]
    # the work buffer holds src1 in the weight's vec_dot_type: never more than src1 itself plus a block header per 32 values
    return _graph(w_raw.nbytes + 3 * x_raw.nbytes + 4 * int(np.prod(shape)) + (1 << 20), build)[0]


def soft_max_ext(x, mask, scale, inplace=False):
    """ggml_soft_max_ext(x, mask, scale, max_bias = 0) (or its _inplace form): x float32 [ne3, ne2, ne1, ne0]; mask float32 or float16, dense, with
    mask.ne[0] == ne0, mask.ne[1] >= ne1 and ne[2], ne[3] dividing x's.  The shape of x"""
    x = np.ascontiguousarray(x, np.float32)
    assert mask.dtype in (np.float32, np.float16)
    mask = np.ascontiguousarray(mask)
    mt = GGML_TYPE_F16 if mask.dtype == np.float16 else GGML_TYPE_F32

    def build(base, ctx):
        a = _new(base, ctx, x)
        ctor = base.ggml_soft_max_ext_inplace if inplace else base.ggml_soft_max_ext
        d = ctor(ctx, a, _new(base, ctx, mask, mt), C.c_float(scale), C.c_float(0.0))
        return d, [(d, x.shape, np.float32)]
    return _graph(2 * x.nbytes + mask.nbytes + 4 * (x.shape[-1] + 64) + (1 << 16), build)[0]


def gelu_tables():
    """(ggml_table_gelu_f16, ggml_table_gelu_quick_f16) as the reference's ggml_cpu_init filled them: uint16 [65536] each"""
    _, cpu = libs()
    return tuple(np.ctypeslib.as_array((C.c_uint16 * 65536).in_dll(cpu, name)).copy() for name in ("ggml_table_gelu_f16", "ggml_table_gelu_quick_f16"))


def fp32_to_fp16(x):
    """ggml_fp32_to_fp16_row: the portable ggml_compute_fp32_to_fp16 (ggml-impl.h:401-425) per element -- what GGML_CPU_FP32_TO_FP16 is in the
    x86-64-v3 build (simd-mappings.h:143-145) -- as uint16"""
    base, _ = libs()
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty(x.size, np.uint16)
    base.ggml_fp32_to_fp16_row(x.ctypes.data, y.ctypes.data, x.size)
    return y


def fp16_to_fp32(h):
    """ggml_fp16_to_fp32_row: ggml_compute_fp16_to_fp32 (ggml-impl.h:378-399), which also fills ggml_table_f32_f16"""
    base, _ = libs()
    h = np.ascontiguousarray(h, np.uint16)
    y = np.empty(h.size, np.float32)
    base.ggml_fp16_to_fp32_row(h.ctypes.data, y.ctypes.data, h.size)
    return y


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _f(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def special_values():
    """+-0, +-inf, NaNs (quiet and signalling, either sign, payloads in the high and in the low mantissa bits), the smallest and largest
    subnormals, +-FLT_MIN, +-FLT_MAX, the GELU clamp at +-10 and the fp16 range's edges: 65504, the tie at 65520, 2^-24, the tie at 2^-25"""
    b = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fa00000, 0xffa55aa5, 0x7fffffff, 0xffffffff,
         0x7fc02000, 0x7f802000, 0x7fc01fff,
         0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x7f7fffff, 0xff7fffff]
    v = [10.0, -10.0, 65504.0, 65519.996, 65520.0, -65520.0, 2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -14, 1.0, -1.0, 22.0, -22.0, 0.5, 88.0, -88.0, -104.0]
    f = np.array(v, np.float32)
    near = np.concatenate([np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))])
    return np.concatenate([_f(b), f, near])


def threshold_neighbours():
    """the neighbours (-2 .. +2 ulp, both signs) of every branch threshold of glibc's tanhf (s_tanhf.c: inf, 22, 1, 2^-55), of the expm1f it
    calls on 2|x| and -2|x| (s_expm1f.c: 27 ln2, 88.72, 0.5 ln2, 1.5 ln2, 2^-25, and k = 23, 56 / 57 through x = k ln2; the thresholds
    themselves and their halves, which is where tanhf's argument puts them) and of expf (e_expf.c: |x| >= 88, overflow, underflow,
    may-underflow), which SIGMOID and GELU_QUICK call"""
    t = [0x7f800000, 0x41b00000, 0x3f800000, 0x24000000,
         0x4195b844, 0x42b17218, 0x42b17180, 0x3eb17218, 0x3f851592, 0x33000000]
    t += [int(np.float32(k * np.log(2.0)).view(np.uint32)) for k in (2, 22, 23, 24, 56, 57, 58)]
    t += [int(np.float32(k * np.log(2.0) + 0.5 * np.log(2.0)).view(np.uint32)) for k in (1, 2, 22, 23, 56, 57)]      # where k = (int)(x / ln2 + 0.5) steps
    t += [b - 0x00800000 for b in list(t) if 0x00800000 < b < 0x7f800000]                    # halved: tanhf hands expm1f 2|x|
    t += [0x42b00000] + [int(np.float32(float.fromhex(h)).view(np.uint32)) for h in ("0x1.62e42ep6", "0x1.9fe368p6", "0x1.9d1d9ep6")]      # expf: 88 and its three range tests
    t += [int(np.float32(float.fromhex(h) / 1.702).view(np.uint32)) for h in ("0x1.62e42ep6", "0x1.9fe368p6", "0x1.9d1d9ep6")]             # the same, reached through GELU_QUICK's -1.702 x
    bits = []
    for b in t:
        for d in range(-2, 3):
            v = b + d
            if 0 <= v <= 0x7fffffff:
                bits += [v, v | 0x80000000]
    return _f(bits)


def all_fp16_values():
    """every fp16-representable value as float32 (NaNs included): all 65 536 indices of the two GELU tables"""
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)


def random_bits(n=1 << 20, seed=20250607):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)


def full_input_set():
    return np.concatenate([all_fp16_values(), special_values(), threshold_neighbours(), random_bits()])
