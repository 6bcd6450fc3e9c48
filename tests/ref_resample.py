"""The reference's own CPU backend (ref_ggml.libs()) for the nodes the front ends put around their convolutions: ggml_pad_ext, ggml_pad_reflect_1d, ggml_interpolate
(NEAREST and BILINEAR) and ggml_conv_transpose_1d.  Next to each runner: a numpy restatement (pad_np, pad_reflect_1d_np, upscale_np, conv_transpose_1d_np), which
tests/test_resample_model.py shows equal to the reference word for word on the case lists below, so that the GPU files share one settled expectation; and those case
lists.  Arrays are in numpy order (the reversed ne).  A source is (raw, View): the buffer and the view of it the node reads; `gather` is the dense array of that view."""
import ctypes as C

import numpy as np

import ref_ggml as R
from ref_ggml import GGML_TYPE_F16, GGML_TYPE_F32, View, _bytes, _graph, _parent, _view

f32 = np.float32
NEAREST, BILINEAR = 0, 1
SENT = f32(-7.25)
_ready = False


def libs():
    global _ready
    base, cpu = R.libs()
    if not _ready:
        P, I = C.c_void_p, C.c_int
        base.ggml_pad_ext.restype, base.ggml_pad_ext.argtypes = P, [P, P] + [I] * 8
        base.ggml_pad_reflect_1d.restype, base.ggml_pad_reflect_1d.argtypes = P, [P, P, I, I]
        base.ggml_interpolate.restype, base.ggml_interpolate.argtypes = P, [P, P] + [C.c_int64] * 4 + [C.c_uint32]
        base.ggml_conv_transpose_1d.restype, base.ggml_conv_transpose_1d.argtypes = P, [P, P, P, I, I, I]
        _ready = True
    return base, cpu


# ---- sources: dense, padded with poison, permuted ------------------------------------------------------------------------------------------
def _np_dtype(type_):
    return np.uint16 if type_ == GGML_TYPE_F16 else np.float32


def dense(a, type_=GGML_TYPE_F32):
    """(raw, View) of a dense array of up to 4 dimensions"""
    a = np.ascontiguousarray(a)
    return a.reshape(-1), View(type_, R._ne(a))


def padded(a, extra, poison, type_=GGML_TYPE_F32):
    """a [n3, n2, n1, n0] (fewer dimensions allowed) inside a buffer with extra = (e0, e1, e2) poison elements behind every row, rows behind every plane, planes behind
    every cube: (raw, View with those strides)"""
    a = np.ascontiguousarray(a)
    a4 = a.reshape((1,) * (4 - a.ndim) + a.shape)
    n3, n2, n1, n0 = a4.shape
    buf = np.full((n3, n2 + extra[2], n1 + extra[1], n0 + extra[0]), poison, a.dtype)
    buf[:, :n2, :n1, :n0] = a4
    es = a.dtype.itemsize
    nb = [es, buf.shape[3] * es, buf.shape[3] * buf.shape[2] * es, buf.shape[3] * buf.shape[2] * buf.shape[1] * es]
    return buf.reshape(-1), View(type_, [n0, n1, n2, n3], nb)


def permuted(a, axes, type_=GGML_TYPE_F32):
    """ggml_permute(axes) (or "transpose") of the dense array a: (raw, View)"""
    a = np.ascontiguousarray(a)
    return a.reshape(-1), View(type_, R._ne(a), None, 0, axes)


def gather(raw, view):
    """the dense array [ne3, ne2, ne1, ne0] of what the view shows of raw"""
    ne, nb = view.final()
    raw = np.ascontiguousarray(raw).reshape(-1)
    return np.lib.stride_tricks.as_strided(raw[view.offset // raw.dtype.itemsize:], tuple(reversed(ne)), tuple(reversed(nb))).copy()


def device_view(gpu, raw, view):
    """the device tensor of (raw, view)"""
    raw = np.ascontiguousarray(raw).reshape(-1)
    ne, nb = view.final()
    return gpu.Tensor.from_numpy(raw.view(np.float16) if raw.dtype == np.uint16 else raw).view(ne, nb, view.offset)


def run_in_sentinel(gpu, call, out_shape, at=4):
    """call(dst) on a contiguous F32 destination `at` floats into a sentinel-filled buffer (at 4: the rows may start on 16 bytes; at 5: they never do); the sentinel
    must survive on both sides.  Returns the destination's words as float32 of out_shape"""
    n = int(np.prod(out_shape))
    buf = gpu.Tensor.from_numpy(np.full(n + at + 7, SENT, f32))
    ne = list(reversed(out_shape)) + [1] * (4 - len(out_shape))
    dst = buf.view(ne, [4, 4 * ne[0], 4 * ne[0] * ne[1], 4 * ne[0] * ne[1] * ne[2]], 4 * at)
    call(dst)
    words = buf.numpy()
    assert np.all(words[:at] == SENT) and np.all(words[at + n:] == SENT), "written outside the destination"
    return words[at:at + n].reshape(out_shape)


CLLM_E_INVALID, CLLM_E_UNSUPPORTED = -1, -2
_cache = {}


def shared(key, make):
    """make() once per key, read-only afterwards: a reference shared among the tests that need it"""
    if key not in _cache:
        v = make()
        v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def declined(gpu, rc, word, call, dst_host):
    """call(dst) raises CllmError with the code rc and `word` in its message, and leaves the destination (a device copy of dst_host) untouched"""
    import pytest
    dst = gpu.Tensor.from_numpy(dst_host)
    with pytest.raises(gpu.lib.CllmError) as e:
        call(dst)
    assert e.value.rc == rc and word in str(e.value), str(e.value)
    assert np.array_equal(dst.numpy(), dst_host)


def edge_mix(shape, seed):
    """ordinary values with NaNs of every payload, +-0, +-inf, subnormals and the other special values (ref_ggml.special_values) on a third of the positions"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(f32)
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=flat.size // 3 + 1, replace=False)
    flat[idx] = np.resize(R.special_values(), idx.size)
    return x


# ---- PAD ----------------------------------------------------------------------------------------------------------------------------------
def pad(raw, view, p):
    """ggml_pad_ext(the F32 view of raw, lp0, rp0, .., lp3, rp3) -> float32 [ne3, ne2, ne1, ne0]"""
    libs()
    raw = np.ascontiguousarray(raw, f32).reshape(-1)
    ne, _ = view.final()
    out = tuple(reversed([ne[i] + p[2 * i] + p[2 * i + 1] for i in range(4)]))

    def build(base, ctx):
        d = base.ggml_pad_ext(ctx, _view(base, ctx, _parent(base, ctx, GGML_TYPE_F32, _bytes(raw)), view), *p)
        return d, [(d, out, f32)]
    return _graph(raw.nbytes + 4 * int(np.prod(out)) + (1 << 16), build)[0]


def pad_np(x, p):
    """x [ne3, ne2, ne1, ne0]: the source words inside, +0.0f around"""
    x = np.asarray(x, f32)
    x = x.reshape((1,) * (4 - x.ndim) + x.shape)
    n = x.shape
    out = np.zeros((n[0] + p[6] + p[7], n[1] + p[4] + p[5], n[2] + p[2] + p[3], n[3] + p[0] + p[1]), np.uint32)
    out[p[6]:p[6] + n[0], p[4]:p[4] + n[1], p[2]:p[2] + n[2], p[0]:p[0] + n[3]] = x.view(np.uint32)
    return out.view(f32)


def pad_sources():
    """(name, raw, View, (lp0, rp0, lp1, rp1, lp2, rp2, lp3, rp3)): the smallest shapes at which the kernel can go wrong -- pads on every axis; the causal left pad; an
    outer axis alone; no pad at all; a single word; rows of 34 words over several workgroups (a 16-byte unit and a tail of 2); a transposed source (nb00 != 4); a source
    with poison between rows, planes and cubes"""
    Z = (0,) * 6
    dense_cases = [((5, 3, 2, 2), (1, 2, 2, 1, 1, 1, 1, 2)), ((7, 4, 1, 1), (3, 0) + Z), ((8, 3, 5, 1), (0, 0, 0, 0, 2, 4, 0, 0)), ((6, 2, 2, 1), (0, 0) + Z),
                   ((1, 1, 1, 1), (0, 3) + Z), ((33, 9, 5, 3), (0, 1) + Z)]
    out = []
    for i, (ne, p) in enumerate(dense_cases):
        out.append((f"{list(ne)} {p}", *dense(edge_mix(tuple(reversed(ne)), 40 + i)), p))
    out.append(("transposed [4, 6]", *permuted(edge_mix((4, 6), 50), "transpose"), (1, 2, 1, 0, 0, 0, 0, 0)))
    out.append(("poison between rows and planes", *padded(edge_mix((2, 2, 3, 5), 51), (3, 1, 2), f32(1e30)), (2, 1, 1, 1, 0, 1, 1, 0)))
    return out


# ---- PAD_REFLECT_1D -------------------------------------------------------------------------------------------------------------------------
def pad_reflect_1d(x, p0, p1):
    """ggml_pad_reflect_1d over a dense float32 x [ne3, ne2, ne1, ne00] -> [.., p0 + ne00 + p1]"""
    libs()
    x = np.ascontiguousarray(x, f32)
    out = x.shape[:-1] + (x.shape[-1] + p0 + p1,)

    def build(base, ctx):
        d = base.ggml_pad_reflect_1d(ctx, R._new(base, ctx, x), p0, p1)
        return d, [(d, out, f32)]
    return _graph(2 * x.nbytes + 4 * int(np.prod(out)) + (1 << 16), build)[0]


def pad_reflect_1d_np(x, p0, p1):
    """src[p0], .., src[1], src[0 .. ne00 - 1], src[ne00 - 2], .., src[ne00 - 1 - p1], as words"""
    w = np.ascontiguousarray(x, f32).view(np.uint32)
    n = w.shape[-1]
    idx = np.concatenate([np.arange(p0, 0, -1), np.arange(n), np.arange(n - 2, n - 2 - p1, -1)]).astype(np.int64)
    return np.ascontiguousarray(w[..., idx]).view(f32)


# (ne00, p0, p1, the other ne): both pads; the shortest row that can be padded; one side only; the longest pads (ne00 - 1); none; a row beyond 64 words; 135 rows of 137
# words (35 units each): 19 workgroups
REFLECT = [(5, 2, 3, (3, 2, 2)), (2, 1, 1, (3, 2, 2)), (9, 0, 4, (3, 2, 2)), (9, 8, 0, (3, 2, 2)), (7, 0, 0, (3, 2, 2)), (65, 3, 2, (3, 2, 2)), (130, 4, 3, (9, 5, 3))]


def reflect_input(case):
    ne00, p0, p1, rest = case
    return edge_mix(tuple(reversed(rest)) + (ne00,), 60 + ne00 + p0)


# ---- UPSCALE --------------------------------------------------------------------------------------------------------------------------------
def upscale(raw, view, ne, mode):
    """ggml_interpolate(the F32 view of raw, ne0 .. ne3, mode) -> float32 [ne3, ne2, ne1, ne0]"""
    libs()
    raw = np.ascontiguousarray(raw, f32).reshape(-1)
    ne = [int(v) for v in ne] + [1] * (4 - len(ne))
    out = tuple(reversed(ne))

    def build(base, ctx):
        d = base.ggml_interpolate(ctx, _view(base, ctx, _parent(base, ctx, GGML_TYPE_F32, _bytes(raw)), view), *ne, mode)
        return d, [(d, out, f32)]
    return _graph(raw.nbytes + 4 * int(np.prod(out)) + (1 << 16), build)[0]


def fma32(a, b, c):
    """fmaf over float32 arrays: the product is exact in double; the sum is rounded to odd in double first (TwoSum's residual decides), so that the rounding to
    float32 is the one rounding of an fma"""
    p = np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, f32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = (err != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(f32)


def _fused_or_not(fuse):
    """term + acc with the term's last multiply fused into the add (an fma) or rounded first"""
    return (lambda p, w, acc: fma32(p, w, acc)) if fuse else (lambda p, w, acc: (p * w + acc).astype(f32))


def bilinear_patterns():
    """every way gcc may contract  a*(1-dx)*(1-dy) + b*dx*(1-dy) + c*(1-dx)*dy + d*dx*dy  (left to right; each term is (p * q) * r, and only a term's LAST multiply can
    fuse with an add): the first sum fuses a's multiply, b's, or neither; the second and third add fuse theirs or not.  name -> f(A, B, C, D, dy, my) over the rounded
    products A = a*(1-dx), B = b*dx, C = c*(1-dx), D = d*dx.  "plain/plain/plain" is the un-contracted form"""
    pats = {}
    for first in ("a", "b", "plain"):
        for fc in (True, False):
            for fd in (True, False):
                def f(A, B, C, D, dy, my, first=first, fc=fc, fd=fd):
                    if first == "a":
                        v = fma32(A, my, (B * my).astype(f32))
                    elif first == "b":
                        v = fma32(B, my, (A * my).astype(f32))
                    else:
                        v = ((A * my).astype(f32) + (B * my).astype(f32)).astype(f32)
                    v = _fused_or_not(fc)(C, dy, v)
                    return _fused_or_not(fd)(D, dy, v)
                pats[f"{first}/{'fma' if fc else 'plain'}/{'fma' if fd else 'plain'}"] = f
    return pats


# what the x86-64-v3 build of ggml_compute_forward_upscale_f32 does (read from libggml-cpu.so; tests/test_resample_model.py shows it is the only one that matches):
# b's term is rounded, a's, c's and d's last multiplies are fused
BILINEAR_PATTERN = "a/fma/fma"


def _axis_nearest(n_dst, n_src):
    sf = f32(n_dst) / f32(n_src)
    return (np.arange(n_dst).astype(f32) / sf).astype(np.int64)


def _axis_linear(n_dst, n_src):
    sf = f32(n_dst) / f32(n_src)
    x = (np.arange(n_dst).astype(f32) + f32(0.5)) / sf - f32(0.5)
    k0 = np.floor(x).astype(np.int64)
    k1 = k0 + 1
    k0, k1 = np.clip(k0, 0, n_src - 1), np.clip(k1, 0, n_src - 1)
    dk = x - k0.astype(f32)
    dk = np.where(f32(1.0) < dk, f32(1.0), dk)
    dk = np.where(f32(0.0) < dk, dk, f32(0.0))
    return k0, k1, dk.astype(f32)


def upscale_np(x, ne, mode, pattern=BILINEAR_PATTERN):
    """x [ne03, ne02, ne01, ne00] -> [ne3, ne2, ne1, ne0]; sf_k = (float) ne_k / ne0k; NEAREST: the source word at (int64)(i_k / sf_k) on every axis; BILINEAR: that on
    axes 2 and 3, the four neighbours on axes 0 and 1 combined by the named contraction pattern"""
    x = np.asarray(x, f32)
    x = x.reshape((1,) * (4 - x.ndim) + x.shape)
    ne = [int(v) for v in ne] + [1] * (4 - len(ne))
    i3, i2 = _axis_nearest(ne[3], x.shape[0]), _axis_nearest(ne[2], x.shape[1])
    planes = x[i3][:, i2]
    if mode == NEAREST:
        i1, i0 = _axis_nearest(ne[1], x.shape[2]), _axis_nearest(ne[0], x.shape[3])
        return np.ascontiguousarray(planes.view(np.uint32)[:, :, i1][:, :, :, i0]).view(f32)
    y0, y1, dy = _axis_linear(ne[1], x.shape[2])
    x0, x1, dx = _axis_linear(ne[0], x.shape[3])
    a, b = planes[:, :, y0][:, :, :, x0], planes[:, :, y0][:, :, :, x1]
    c, d = planes[:, :, y1][:, :, :, x0], planes[:, :, y1][:, :, :, x1]
    dy, my = dy[:, None], (f32(1.0) - dy)[:, None]
    mx = f32(1.0) - dx
    A, B, Cc, D = (a * mx).astype(f32), (b * dx).astype(f32), (c * mx).astype(f32), (d * dx).astype(f32)
    return bilinear_patterns()[pattern](A, B, Cc, D, np.broadcast_to(dy, A.shape), np.broadcast_to(my, A.shape))


def upscale_input(shape, seed):
    """standard_normal scaled by 1e4 / 1e-4 alternating per element, so that a misplaced rounding shows"""
    x = np.random.default_rng(seed).standard_normal(shape)
    scale = np.where(np.arange(x.size).reshape(shape) % 2 == 0, 1e4, 1e-4)
    return (x * scale).astype(f32)


# (source ne, destination ne): up by 2; up by odd factors; down; one source pixel; nearest on axes 2 and 3; the identity; odd factors over several workgroups
UPSCALE = [([4, 3, 2, 1], [8, 6, 2, 1]), ([5, 4, 3, 1], [7, 9, 3, 1]), ([7, 5, 2, 1], [3, 2, 2, 1]), ([1, 1, 2, 1], [4, 3, 2, 1]), ([3, 3, 2, 2], [3, 3, 4, 6]),
           ([6, 6, 3, 1], [6, 6, 3, 1]), ([16, 16, 8, 1], [37, 29, 8, 1])]


def upscale_sources():
    """(name, raw, View, destination ne): the list above on dense sources, and step.cpp's source -- the position embedding [hidden, g, g] seen through permute(2, 0, 1) as
    [g, g, hidden] (nb[0] = hidden * 4, nb[2] = 4), resized to another grid"""
    out = [(f"{s} -> {d}", *dense(upscale_input(tuple(reversed(s)), 70 + i)), d) for i, (s, d) in enumerate(UPSCALE)]
    out.append(("permute(2, 0, 1) of [6, 5, 5] -> [7, 4, 6, 1]", *permuted(upscale_input((5, 5, 6), 79), (2, 0, 1, 3)), [7, 4, 6, 1]))
    return out


# ---- CONV_TRANSPOSE_1D ------------------------------------------------------------------------------------------------------------------------
def conv_transpose_1d(k_raw, k_view, x_raw, x_view, s0):
    """ggml_conv_transpose_1d(kernel view [K, Cout, Cin] (F16 words as uint16, or float32), data view [L, Cin] F32, s0, 0, 1) -> float32 [Cout, (L - 1) * s0 + K]"""
    libs()
    kdt = _np_dtype(k_view.type)
    k_raw, x_raw = np.ascontiguousarray(k_raw, kdt).reshape(-1), np.ascontiguousarray(x_raw, f32).reshape(-1)
    K, Cout, Cin = k_view.ne[:3]
    L = x_view.ne[0]
    out = (Cout, (L - 1) * s0 + K)

    def build(base, ctx):
        k = _view(base, ctx, _parent(base, ctx, k_view.type, _bytes(k_raw)), k_view)
        x = _view(base, ctx, _parent(base, ctx, GGML_TYPE_F32, _bytes(x_raw)), x_view)
        d = base.ggml_conv_transpose_1d(ctx, k, x, s0, 0, 1)
        return d, [(d, out, f32)]
    # the work buffer holds the repacked kernel and data
    return _graph(k_raw.nbytes + x_raw.nbytes + 8 * (K * Cout * Cin + L * Cin) + 4 * int(np.prod(out)) + (1 << 20), build)[0]


def _vec_dot(x, y, f16, sequential=False):
    """ggml_vec_dot_f16 / _f32 of the x86-64-v3 build over the first axis of the float32 arrays x and y (broadcast against each other behind it): 32 accumulators,
    accumulator a takes elements a, a + 32, .. with one fma each; GGML_F32x8_REDUCE; the n mod 32 leftovers -- F16: float products added in double and rounded once;
    F32: whole groups of four as rounded products added in order, the scalar rest as fmas.  sequential: acc = acc + x[i] * y[i] in float, for showing that the order matters"""
    n = x.shape[0]
    shape = np.broadcast_shapes(x.shape[1:], y.shape[1:])
    with np.errstate(all="ignore"):
        if sequential:
            u = np.zeros(shape, f32)
            for i in range(n):
                u = (u + (x[i] * y[i]).astype(f32)).astype(f32)
            return u
        acc = [np.zeros(shape, f32) for _ in range(32)]
        np_ = n & ~31
        for i in range(np_):
            acc[i % 32] = fma32(x[i], y[i], acc[i % 32])
        s = [((acc[l] + acc[16 + l]) + (acc[8 + l] + acc[24 + l])).astype(f32) for l in range(8)]
        t = [(s[l] + s[l + 4]).astype(f32) for l in range(4)]
        u = ((t[0] + t[1]) + (t[2] + t[3])).astype(f32)
        if f16:
            sd = u.astype(np.float64)
            for i in range(np_, n):
                sd = sd + (x[i] * y[i]).astype(f32).astype(np.float64)
            return sd.astype(f32)
        i = np_
        while i + 4 <= n:
            for l in range(4):
                u = (u + (x[i + l] * y[i + l]).astype(f32)).astype(f32)
            i += 4
        for i in range(i, n):
            u = fma32(x[i], y[i], u)
        return u


def conv_transpose_1d_np(kernel, data, s0, descending=False, sequential=False):
    """kernel [Cin, Cout, K] (uint16: F16 words; float32), data [Cin, L] float32 -> [Cout, (L - 1) * s0 + K].  From +0.0f; for i10 ascending and every tap i00:
    dst[oc][i10 * s0 + i00] += v(oc, i10, i00), v the reference's dot product over Cin (an F16 kernel: the data rounded to fp16 first).  descending / sequential: the
    wrong orders, for showing that the case lists tell them apart"""
    f16 = kernel.dtype == np.uint16
    data = np.asarray(data, f32)
    with np.errstate(all="ignore"):
        kf = kernel.view(np.float16).astype(f32) if f16 else np.asarray(kernel, f32)
        xf = data.astype(np.float16).astype(f32) if f16 else data
        Cin, Cout, K = kf.shape
        L = xf.shape[1]
        v = _vec_dot(xf[:, None, :, None], kf[:, :, None, :], f16, sequential)          # [Cout, L, K]
        out = np.zeros((Cout, (L - 1) * s0 + K), f32)
        for i10 in (range(L - 1, -1, -1) if descending else range(L)):
            out[:, i10 * s0:i10 * s0 + K] = (out[:, i10 * s0:i10 * s0 + K] + v[:, i10, :]).astype(f32)
    return out


# (K, Cout, Cin, L, s0): leftovers only; whole chunks only; two or three taps per output with F32 leftovers of a group of four and two scalars; no overlap; untouched
# outputs between the taps; one position; up to seven taps; vocoder-like, several workgroups
CONV_T = [(4, 3, 5, 6, 2), (4, 3, 32, 5, 2), (5, 2, 70, 4, 2), (3, 2, 33, 4, 3), (2, 3, 8, 5, 4), (3, 4, 64, 1, 1), (7, 5, 40, 9, 1), (16, 40, 96, 33, 8)]


def conv_t_operands(case, f16, seed=0):
    """(kernel [Cin, Cout, K] as uint16 words or float32, data [Cin, L] float32): large and small magnitudes side by side, so that the order of the dot product and the
    order of the taps both decide a float"""
    K, Cout, Cin, L, s0 = case
    rng = np.random.default_rng([K, Cout, Cin, L, s0, seed])
    k = rng.standard_normal((Cin, Cout, K)) * np.where(rng.random((Cin, Cout, K)) < 0.5, 8.0, 0.125)
    x = rng.standard_normal((Cin, L)) * np.where(rng.random((Cin, L)) < 0.5, 64.0, 1.0 / 64.0)
    k = k.astype(np.float16).view(np.uint16) if f16 else k.astype(f32)
    return k, x.astype(f32)


def conv_t_views(k, x, layout):
    """((k_raw, k_view), (x_raw, x_view)) for layout "dense", "padded data" (nb11 > 4 L, poison between) or "padded kernel" (nb01 and nb02 padded)"""
    kt = GGML_TYPE_F16 if k.dtype == np.uint16 else GGML_TYPE_F32
    kpoison = np.uint16(0x7bff) if k.dtype == np.uint16 else f32(1e30)
    kk = padded(k, (3, 2, 0), kpoison, kt) if layout == "padded kernel" else dense(k, kt)
    xx = padded(x, (5, 0, 0), f32(1e30)) if layout == "padded data" else dense(x)
    return kk, xx
