"""MUL_MAT over every operand layout the C ABI accepts: the cases tests/test_matmul_layout_model.py (CPU: the oracle over the views against the oracle over dense
copies and against the reference's CPU backend) and tests/test_gpu_matmul_layouts.py (the kernels against the oracle) share.  Plain numpy, no GPU.

A case is a weight type, a shape [K, N, ne02, ne03] x [K, M, ne12, ne13] and a LAYOUT: a view (ne, nb, offset) of a raw weight buffer, of a raw src1 buffer and of a
raw dst buffer.  build(case) makes the three buffers and the dense copies of the operands.  Every byte of a source buffer that its view does not cover is POISON
(0x7f: 3.39e38 as F32, a NaN as an fp16 scale, a saturated block as quants); every byte of the dst buffer starts as moe_model.SENTINEL.

Layout parts (a layout is a tuple of them; LAYOUTS_2D / LAYOUTS_3D name the tuples):
  w_row_pad    nb01 = row_size + p, p the smallest positive multiple of both 16 and the type's row_align (csrc/types.def)
  w_col_slice  the second half of the columns of a [2K, N] matrix: nb01 = row_size(2K), offset row_size(K)
  w_3d         ne02 = ne03 = 2 with nb02 and nb03 padded by p (src1 ne12 = 4, ne13 = 2: r2 = 2, r3 = 1; ne12 = 2, ne13 = 4: r2 = 1, r3 = 2)
  x_row_pad    nb11 = 4K + 16, nb12 and nb13 padded by 32 and 48 more
  x_permuted   src1 is permute(0, 2, 1, 3) of a [K, ne12, M] buffer: nb11 = 4K ne12, nb12 = 4K
  d_row_pad    nb1 = 4N + 12 (a multiple of 4 and not of 16), nb2 and nb3 padded by 20 and 8 more
  offset       src1 and dst start 16 bytes into their buffers, the weight row_align bytes (the smallest its launchers take) into its own

A case whose layout changes nothing that can be observed at its shape (x_row_pad or d_row_pad with one column and one slice) is not generated: alterations(case) lists
the strides and offsets that differ from the dense ones in a dimension of more than one entry, and test_matmul_layout_model.py shows for each of them that computing
with the dense value instead gives another result -- a case that could not tell a stride bug from correct code fails there.

route_of(case, thresholds, ...) restates csrc/capi.hip's and csrc/matmul_f.hip's choice of kernel from the thresholds the library reports, not from device state."""
import collections
import ctypes as C
import functools
import os
import re
import zlib

import numpy as np

import moe_model
import weight_edge_cases as W
from conftest import ROOT, load_package
from synth_helpers import BLCK, TYPE_SIZE, rand_blocks

POISON, SENTINEL = 0x7f, moe_model.SENTINEL
F32, F16 = 0, 1
TUNED, KQ_TYPES, FLOAT_TYPES = W.TUNED, W.ALL_TYPES[4:], (F16, F32)
TYPE_NAME = {**W.TYPE_NAME, F32: "f32"}
View = collections.namedtuple("View", "ne nb offset")


def _row_align():
    """type id -> row_align, from csrc/types.def"""
    text = open(os.path.join(ROOT, "chatllm.cpp_amd", "csrc", "types.def")).read()
    out = {int(m.group(1)): int(m.group(2)) for m in re.finditer(r"^CLLM_WTYPE\(\s*\w+,\s*(\d+),\s*\d+,\s*\d+,\s*\w+,\s*\w+,\s*(\d+),", text, re.M)}
    assert len(out) >= 26 and out[12] == 16 and out[3] == 4 and out[2] == 2, out
    return out


ROW_ALIGN = _row_align()


def row_size(t, ne0):
    assert ne0 % BLCK[t] == 0
    return TYPE_SIZE[t] * (ne0 // BLCK[t])


def w_pad(t):
    """the smallest positive multiple of both 16 and the type's row_align"""
    return int(np.lcm(16, ROW_ALIGN[t]))


def dense_view(t, ne):
    rs = row_size(t, ne[0])
    return View(list(ne), [TYPE_SIZE[t], rs, rs * ne[1], rs * ne[1] * ne[2]], 0)


def extent(t, v):
    """one past the last byte of the view"""
    return v.offset + sum((v.ne[i] - 1) * v.nb[i] for i in (1, 2, 3)) + row_size(t, v.ne[0])


def _up(n, m):
    return (n + m - 1) // m * m


LAYOUTS_2D = {"dense": (), "w_row_pad": ("w_row_pad",), "w_col_slice": ("w_col_slice",), "x_row_pad": ("x_row_pad",), "d_row_pad": ("d_row_pad",), "offset": ("offset",),
              "combined": ("w_row_pad", "x_row_pad", "d_row_pad", "offset")}
# name -> (parts, ne02, ne03, ne12, ne13)
LAYOUTS_3D = {"w_3d_r2": (("w_3d",), 2, 2, 4, 2), "w_3d_r3": (("w_3d",), 2, 2, 2, 4), "x_permuted": (("x_permuted",), 1, 1, 3, 1),
              "combined_3d": (("w_row_pad", "w_3d", "x_row_pad", "d_row_pad", "offset"), 2, 2, 4, 2)}


def layout_views(t, K, N, M, ne02, ne03, ne12, ne13, parts):
    """-> (weight view, src1 view, dst view) of the layout `parts`"""
    rs, p = row_size(t, K), w_pad(t)
    nb01, woff = rs, 0
    if "w_row_pad" in parts:
        nb01 = rs + p
    if "w_col_slice" in parts:
        assert "w_row_pad" not in parts
        nb01, woff = row_size(t, 2 * K), rs
        assert woff % ROW_ALIGN[t] == 0, "this slice breaks the type's row_align: it belongs to the declines"
    nb02 = nb01 * N + (p if "w_3d" in parts else 0)
    nb03 = nb02 * ne02 + (p if "w_3d" in parts else 0)
    if "offset" in parts:
        woff += ROW_ALIGN[t]
    wv = View([K, N, ne02, ne03], [TYPE_SIZE[t], nb01, nb02, nb03], woff)
    if "x_permuted" in parts:
        assert "x_row_pad" not in parts
        xnb = [4, 4 * K * ne12, 4 * K, 4 * K * ne12 * M]
    elif "x_row_pad" in parts:
        nb11 = 4 * K + 16
        nb12 = nb11 * M + 32
        xnb = [4, nb11, nb12, nb12 * ne12 + 48]
    else:
        xnb = dense_view(F32, [K, M, ne12, ne13]).nb
    xv = View([K, M, ne12, ne13], xnb, 16 if "offset" in parts else 0)
    if "d_row_pad" in parts:
        nb1 = 4 * N + 12
        nb2 = nb1 * M + 20
        dnb = [4, nb1, nb2, nb2 * ne12 + 8]
    else:
        dnb = dense_view(F32, [N, M, ne12, ne13]).nb
    dv = View([N, M, ne12, ne13], dnb, 16 if "offset" in parts else 0)
    return wv, xv, dv


class Case:
    """one product: family (tuned / kq / float), type, shape, layout name and the three views; wbytes / xbytes / dbytes: the sizes of the raw buffers"""

    def __init__(self, family, t, layout, wv, xv, dv, wbytes=None, tag=""):
        self.family, self.t, self.layout, self.wv, self.xv, self.dv = family, t, layout, wv, xv, dv
        self.K, self.N, self.M = wv.ne[0], wv.ne[1], xv.ne[1]
        self.ne02, self.ne03, self.ne12, self.ne13 = wv.ne[2], wv.ne[3], xv.ne[2], xv.ne[3]
        assert dv.ne == [self.N, self.M, self.ne12, self.ne13] and xv.ne[0] == self.K and self.ne12 % self.ne02 == 0 and self.ne13 % self.ne03 == 0
        self.wbytes = _up(max(wbytes or 0, extent(t, wv)) + 16, 16)
        self.xbytes = _up(extent(F32, xv) + 16, 16)
        self.dbytes = _up(extent(F32, dv) + 16, 4)
        batch = f"-b{self.ne02}x{self.ne03}.{self.ne12}x{self.ne13}" if (self.ne02, self.ne03, self.ne12, self.ne13) != (1, 1, 1, 1) else ""
        self.name = f"{TYPE_NAME[t]}-K{self.K}-N{self.N}-M{self.M}{batch}-{layout}{tag}"

    def is_dense(self):
        return not alterations(self)

    def __repr__(self):
        return self.name


def generic_case(family, t, K, N, M, layout):
    if layout in LAYOUTS_2D:
        parts, ne02, ne03, ne12, ne13 = LAYOUTS_2D[layout], 1, 1, 1, 1
    else:
        parts, ne02, ne03, ne12, ne13 = LAYOUTS_3D[layout]
    wv, xv, dv = layout_views(t, K, N, M, ne02, ne03, ne12, ne13, parts)
    wbytes = N * row_size(t, 2 * K) if "w_col_slice" in parts else None
    return Case(family, t, layout, wv, xv, dv, wbytes)


def attention_case(kind, qlen, n_past=None):
    """the two contractions of the eager attention block over F16 cache views, with test_attention_composite's strides: K.Q-like -- the weight is the view
    [hd, n_kv, nkv] of a [ML, nkv hd] key cache, src1 the permuted query [hd, qlen, nh] of a [qlen, nh, hd] buffer; V.P-like -- the weight is the view [n_kv, hd, nkv]
    of a [nkv hd, ML] transposed value cache (rows of n_kv out of ML positions), src1 the dense probabilities [n_kv, qlen, nh].  n_kv = 264 of ML = 320 positions"""
    hd, nh, nkv, ML, n_kv = 128, 4, 2, 320, 264
    KD = hd * nkv
    if kind == "kq_like":
        wv = View([hd, n_kv, nkv, 1], [2, KD * 2, hd * 2, KD * ML * 2], 0)
        xv = View([hd, qlen, nh, 1], [4, nh * hd * 4, hd * 4, nh * hd * qlen * 4], 0)
        dv = dense_view(F32, [n_kv, qlen, nh, 1])
        wbytes = ML * KD * 2
    else:
        wv = View([n_kv, hd, nkv, 1], [2, ML * 2, ML * hd * 2, ML * KD * 2], 0)
        xv = dense_view(F32, [n_kv, qlen, nh, 1])
        dv = dense_view(F32, [hd, qlen, nh, 1])
        wbytes = KD * ML * 2
    return Case("float", F16, kind, wv, xv, dv, wbytes)


# ---- what a layout changes -------------------------------------------------------------------------------------------------------------------
def alterations(c):
    """[(label, operand "w" / "x" / "d", field 1 / 2 / 3 / "offset", dense value)]: every stride of a dimension with more than one entry that differs from the dense
    one, and every offset"""
    out = []
    for op, t, v in (("w", c.t, c.wv), ("x", F32, c.xv), ("d", F32, c.dv)):
        dn = dense_view(t, v.ne)
        for i in (1, 2, 3):
            if v.ne[i] > 1 and v.nb[i] != dn.nb[i]:
                out.append((f"{op}.nb[{i}]", op, i, dn.nb[i]))
        if v.offset:
            out.append((f"{op}.offset", op, "offset", 0))
    return out


def altered_view(v, field, value):
    if field == "offset":
        return View(v.ne, v.nb, value)
    nb = list(v.nb)
    nb[field] = value
    return View(v.ne, nb, v.offset)


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------------
def _starts(v):
    """the byte offset of every row of the view: [ne3, ne2, ne1]"""
    i1, i2, i3 = (np.arange(v.ne[i], dtype=np.int64) * v.nb[i] for i in (1, 2, 3))
    return v.offset + i3[:, None, None] + i2[None, :, None] + i1[None, None, :]


def _row_bytes_index(t, v):
    return (_starts(v)[..., None] + np.arange(row_size(t, v.ne[0]), dtype=np.int64)).reshape(-1)


def scatter(raw, t, v, rows):
    """rows: uint8 [ne3, ne2, ne1, row bytes] -> into the view of raw"""
    raw[_row_bytes_index(t, v)] = np.ascontiguousarray(rows).reshape(-1).view(np.uint8)


def gather(raw, t, v):
    """the view's rows as uint8 [ne3, ne2, ne1, row bytes]"""
    return raw[_row_bytes_index(t, v)].reshape(v.ne[3], v.ne[2], v.ne[1], row_size(t, v.ne[0]))


def view_mask(nbytes, t, v):
    m = np.zeros(nbytes, bool)
    m[_row_bytes_index(t, v)] = True
    return m


Built = collections.namedtuple("Built", "w_raw x_raw d_raw w_dense x_dense")


@functools.lru_cache(maxsize=4)
def build(c):
    """-> Built: the raw buffers (uint8; read-only but d_raw's copies) and the dense operands: w_dense uint8 [ne03, ne02, N, row bytes], x_dense float32
    [ne13, ne12, M, K]"""
    rng = np.random.default_rng(zlib.crc32(c.name.encode()))
    rows = c.ne03 * c.ne02 * c.N
    if c.t in FLOAT_TYPES:
        wd = np.ascontiguousarray(rng.standard_normal((rows, c.K)).astype(np.float16 if c.t == F16 else np.float32)).view(np.uint8)
    else:
        wd = rand_blocks(c.t, rows, c.K, rng)
    wd = wd.reshape(c.ne03, c.ne02, c.N, row_size(c.t, c.K))
    xd = rng.standard_normal((c.ne13, c.ne12, c.M, c.K)).astype(np.float32)
    w_raw, x_raw = np.full(c.wbytes, POISON, np.uint8), np.full(c.xbytes, POISON, np.uint8)
    scatter(w_raw, c.t, c.wv, wd)
    scatter(x_raw, F32, c.xv, xd.view(np.uint8).reshape(c.ne13, c.ne12, c.M, 4 * c.K))
    d_raw = np.full(c.dbytes, SENTINEL, np.uint8)
    for a in (w_raw, x_raw, d_raw, wd, xd):
        a.setflags(write=False)
    assert np.array_equal(gather(w_raw, c.t, c.wv), wd)
    return Built(w_raw, x_raw, d_raw, wd, xd)


def oracle_over_views(O, c, b, wv=None, xv=None, dv=None):
    """orc_mul_mat over the (possibly altered) views of the raw buffers -> the whole dst buffer afterwards (uint8)"""
    wv, xv, dv = wv or c.wv, xv or c.xv, dv or c.dv
    assert extent(c.t, wv) <= b.w_raw.size and extent(F32, xv) <= b.x_raw.size and extent(F32, dv) <= b.d_raw.size
    d = b.d_raw.copy()
    O.mul_mat(O.tensor(b.w_raw, c.t, wv.ne, wv.nb, wv.offset), O.tensor(b.x_raw, O.F32, xv.ne, xv.nb, xv.offset), O.tensor(d, O.F32, dv.ne, dv.nb, dv.offset))
    return d


def x_contiguous(c):
    """ggml_is_contiguous(src1): every stride of a dimension with more than one entry is the dense one"""
    return all(c.xv.ne[i] == 1 or c.xv.nb[i] == dense_view(F32, c.xv.ne).nb[i] for i in (1, 2, 3))


_expected = {}


def expected(O, c):
    """-> (want float32 [ne13, ne12, M, N]: the oracle over the DENSE copies; the whole dst buffer expected afterwards: want through the view, SENTINEL elsewhere).
    Computed once per case and shared, read-only"""
    if c.name not in _expected:
        if len(_expected) > 64:
            _expected.clear()
        b = build(c)
        want = np.zeros((c.ne13, c.ne12, c.M, c.N), np.float32)
        # An F32 weight reads src1 in place, and the reference tries tinyBLAS only on a contiguous src1 (ggml-cpu.c:1269-1271): with padded or permuted src1 rows
        # the product has ggml_vec_dot_f32's order at every shape, so the dense copy of src1 would be another computation.  Those cases keep their src1 view here
        # (weight and dst dense); the reference backend on the same views is what holds them (test_matmul_layout_model.py b)
        x = O.tensor(b.x_dense, O.F32, c.xv.ne) if c.t != F32 or x_contiguous(c) else O.tensor(b.x_raw, O.F32, c.xv.ne, c.xv.nb, c.xv.offset)
        O.mul_mat(O.tensor(b.w_dense, c.t, c.wv.ne), x, O.tensor(want, O.F32, c.dv.ne))
        exp = b.d_raw.copy()
        scatter(exp, F32, c.dv, want.view(np.uint8).reshape(c.ne13, c.ne12, c.M, 4 * c.N))
        want.setflags(write=False)
        exp.setflags(write=False)
        _expected[c.name] = (want, exp)
    return _expected[c.name]


# ---- the case lists ----------------------------------------------------------------------------------------------------------------------------
TUNED_N, TUNED_M = (7, 20, 130), (1, 3, 6, 12, 40, 70)
KQ_M = (1, 5, 9)
FLOAT_SHAPES = [(100, 17, 1), (128, 20, 1), (100, 17, 3), (128, 20, 3), (128, 20, 40), (203, 17, 40)]          # (K, N, M)


def _keep(c):
    """a layout that changes nothing observable at this shape is the dense case over again"""
    return c.layout == "dense" or bool(alterations(c))


def _cases():
    out = []
    for t in TUNED:
        for K in (512,) if BLCK[t] == 256 else (512, 96):
            for M in TUNED_M:
                out += [generic_case("tuned", t, K, N, M, lay) for N in TUNED_N for lay in LAYOUTS_2D]
                out += [generic_case("tuned", t, K, 20, M, lay) for lay in LAYOUTS_3D]
    for t in KQ_TYPES:
        for i, (K, N) in enumerate(W.shapes_of(t)):
            for M in KQ_M:
                out += [generic_case("kq", t, K, N, M, lay) for lay in LAYOUTS_2D]
                if i == 0:
                    out += [generic_case("kq", t, K, N, M, lay) for lay in LAYOUTS_3D]
    for t in FLOAT_TYPES:
        for K, N, M in FLOAT_SHAPES:
            out += [generic_case("float", t, K, N, M, lay) for lay in LAYOUTS_2D]
            if M > 1 and K != 100:
                out += [generic_case("float", t, K, N, M, lay) for lay in LAYOUTS_3D]
    out += [attention_case(kind, qlen) for kind in ("kq_like", "vp_like") for qlen in (1, 3, 40)]
    out = [c for c in out if _keep(c)]
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()
TUNED_CASES = [c for c in CASES if c.family == "tuned"]
KQ_CASES = [c for c in CASES if c.family == "kq"]
FLOAT_CASES = [c for c in CASES if c.family == "float"]
case_id = lambda c: c.name  # noqa: E731


# ---- routes ------------------------------------------------------------------------------------------------------------------------------------
Thresholds = collections.namedtuple("Thresholds", "mmx_min mmq_min mma_min mmf_min")


@functools.lru_cache(maxsize=1)
def thresholds():
    """the column thresholds between the kernels as the library reports them: cllm_mul_mat_ex_min_cols() (the exact-order GEMM) and the options table"""
    L = load_package().lib.get()
    n = L.cllm_options_describe(None, 0)
    buf = C.create_string_buffer(n + 1)
    assert L.cllm_options_describe(buf, n + 1) == n
    rows = {f[0]: f for f in (line.split("\t") for line in buf.value.decode().splitlines())}
    val = lambda name: int(rows[name][9])  # noqa: E731          (columns: tests/test_options.py COLS; 9 = value)
    return Thresholds(int(L.cllm_mul_mat_ex_min_cols()), val("CLLM_MMQ_MIN_COLS"), val("CLLM_MMA_MIN_COLS"), val("CLLM_MMF_EXACT_MIN_COLS"))


def _aligned16(*views):
    return all((v.offset | v.nb[1] | v.nb[2] | v.nb[3]) % 16 == 0 for v in views)


def route_of(c, th, prefill=1, attn=1, f16=False):
    """the kernel cllm_op_mul_mat launches for the case (csrc/capi.hip cllm_op_mul_mat, mm_route; csrc/matmul_f.hip launch_mul_mat_f; csrc/gemv_kq.hip
    kq_launch_nc).  prefill / attn: 1 the exact modes, 0 the fast ones; f16: the opt-in fp16 prefill.  Device buffers are 256-byte aligned, so a pointer is as
    aligned as its offset"""
    if c.family == "float":
        t8 = c.M >= 2 and c.K % 8 == 0 and c.N % 4 == 0 and (c.t == F16 or x_contiguous(c))         # an F32 weight reads src1 in place: tinyBLAS only when it is contiguous
        if c.t == F16 and c.M >= th.mma_min and attn == 0 and _aligned16(c.wv, c.xv):
            return "mma_f16"
        if c.t == F16 and c.M >= th.mmf_min and not (c.t == F16 and c.M >= th.mma_min and attn == 0):
            if t8 and _aligned16(c.wv, c.xv) and c.K <= 128 and c.M > 32 and c.N >= 256:
                return "mmf_exact_kq"
            return "mmf_exact_t8" if t8 else "mmf_exact_vd"
        return "f_t8" if t8 else "f_vd"
    if c.family == "kq":
        return "gemv_kq_nc1" if c.M == 1 else "gemv_kq_nc4" if c.M <= 4 else "gemv_kq_nc8" if c.M <= 8 else "gemv_kq_nc8+ragged"
    dense_matrix = c.wv.nb[1] == row_size(c.t, c.K) and c.ne02 == 1 and c.ne03 == 1
    if dense_matrix and c.M == 1 and c.ne12 == 1 and c.ne13 == 1:
        return "decode_one_launch"
    if c.M >= th.mmq_min and (f16 or prefill == 0):
        return "dense_f16" if f16 else "mmq"
    if c.M >= th.mmx_min:
        return "mmx"
    return "decode_two_launches" if c.M == 1 else "mmvq"


ROUTES = ("decode_one_launch", "decode_two_launches", "mmvq", "mmx", "mmq", "dense_f16", "gemv_kq_nc1", "gemv_kq_nc8", "gemv_kq_nc8+ragged",
          "f_vd", "f_t8", "mmf_exact_t8", "mmf_exact_vd", "mmf_exact_kq", "mma_f16")
