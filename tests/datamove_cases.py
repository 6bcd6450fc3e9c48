"""The cases that tests/test_datamove_model.py (CPU: oracle against the reference) and tests/test_gpu_datamove.py (the kernels against the reference)
share: SET_ROWS into F32 / F16 / Q8_0, CPY / CONT between views, GET_ROWS in its batched form and SOFT_MAX with a mask tensor.  A case holds host
buffers (bytes) and ref_ggml.View descriptions of the tensors cut from them; the reference, the oracle and the device tensors are all built from
those.  Arrays are in numpy order (reversed ne).  Every buffer is built once and is read-only.

Every shape is the smallest that reaches the code it is named after.  The trip sizes quoted are the kernels' grid caps times 256 threads:
k_set_rows and k_get_rows 8192 blocks (2 097 152 elements), k_set_rows_q8_0 8192 blocks of 32 eight-lane groups (262 144 quant blocks),
k_cpy and k_cpy_qrows 16384 blocks (4 194 304 elements / two-byte units)."""
import numpy as np

import ref_ggml as R
from elementwise_cases import assert_same_words, shape_of  # noqa: F401  (the tests take them from here)
from ref_ggml import View
from synth_helpers import rand_blocks

F32, F16, Q4_0, Q8_0, Q4_K, Q6_K, I32, I64 = 0, 1, 2, 8, 12, 14, 26, 27
NP_OF = {F32: np.float32, F16: np.float16, I32: np.int32, I64: np.int64}
TYPE_NAME = {F32: "f32", F16: "f16", Q4_0: "q4_0", Q8_0: "q8_0", Q4_K: "q4_k", Q6_K: "q6_k", I32: "i32", I64: "i64"}


def frozen(a):
    a.setflags(write=False)
    return a


def padded_rows(view_ne, type_, extra_bytes, offset=0):
    """a view of ne whose rows lie `extra_bytes` apart beyond their own length, starting `offset` bytes into its buffer: (View, bytes the buffer needs)"""
    ne = list(view_ne) + [1] * (4 - len(view_ne))
    nb1 = R.row_bytes(type_, ne[0]) + extra_bytes
    nb = [R._BLOCK[type_][0], nb1, nb1 * ne[1], nb1 * ne[1] * ne[2]]
    return View(type_, ne, nb, offset), offset + nb[3] * ne[3]


def filled(view, nbytes, values, fill):
    """a buffer of nbytes (rounded up to whole blocks of the view's type) holding `fill` bytes and, where the un-permuted view addresses, the rows of `values`
    (an array of the view's element type, or raw block bytes, in the order of view.ne)"""
    size = R._BLOCK[view.type][0]
    rb = R.row_bytes(view.type, view.ne[0])
    if view.offset == 0 and view.nb[1] == rb and nbytes == view.nb[3] * view.ne[3]:
        return np.ascontiguousarray(values).reshape(-1).view(np.uint8).copy()          # dense
    buf = np.full(-(-nbytes // size) * size, fill, np.uint8)
    rows = np.ascontiguousarray(values).reshape(-1).view(np.uint8).reshape(view.ne[3], view.ne[2], view.ne[1], rb)
    for i3 in range(view.ne[3]):
        for i2 in range(view.ne[2]):
            at = view.offset + i3 * view.nb[3] + i2 * view.nb[2] + np.arange(view.ne[1])[:, None] * view.nb[1] + np.arange(rb)[None, :]
            buf[at] = rows[i3, i2]
    return buf


def gather(buf, view):
    """the rows the un-permuted view addresses in a buffer, as bytes [ne3, ne2, ne1, row bytes]; `outside(buf, view)`: every other byte"""
    rb = R.row_bytes(view.type, view.ne[0])
    at = (view.offset + np.arange(view.ne[3])[:, None, None, None] * view.nb[3] + np.arange(view.ne[2])[None, :, None, None] * view.nb[2]
          + np.arange(view.ne[1])[None, None, :, None] * view.nb[1] + np.arange(rb)[None, None, None, :])
    return buf[at]


# ---- values ----------------------------------------------------------------------------------------------------------------------------------
def f16_edge_values():
    """ref_ggml.special_values() without its NaNs, and the fp16 edges of test_set_rows: 65504, the tie at 65520, 2^-24, the ties at 2^-25 and 1.5 * 2^-25, +-0,
    an overflow and an underflow"""
    s = R.special_values()
    s = s[~np.isnan(s)]
    e = np.array([65504.0, 65520.0, -65520.0, 2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 1.5 * 2.0 ** -25, 0.0, -0.0, 70000.0, 1e-8, -1e-8], np.float32)
    return np.concatenate([e, s])


def floats_with_edges(n, seed):
    """normal * 10 with the edge values spread over it, as many as fit, starting at a place of the list that depends on the seed"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 10).astype(np.float32)
    e = np.roll(f16_edge_values(), -7 * seed)
    k = min(e.size, n)
    x[(np.arange(k) * n) // k] = e[:k]
    return x


def q8_special_blocks():
    """[k, 32] float32, one row a block (finite values only): all zero; constant; the largest magnitude negative; the largest magnitude in each of the eight
    four-value lanes in turn, in the first and in the last element; ties (x * (127 / amax) exactly k + 0.5, k even and odd, both signs) with 127 / amax == 1 and == 2;
    amax subnormal, and normal but so small that 127 / amax overflows (below 3.74e-37), with zeros in the block (0 * inf); the smallest amax whose inverse is finite;
    amax above 65504 * 127, where the stored fp16 scale is inf, and at FLT_MAX; random at 1e-3, 1 and 40"""
    rng = np.random.default_rng(808)
    rnd = lambda s=1.0: (rng.standard_normal(32) * s).astype(np.float32)          # noqa: E731
    b = [np.zeros(32, np.float32), np.full(32, 0.37, np.float32), np.full(32, -2.5, np.float32)]
    x = rnd(); x[5] = -np.abs(x).max() * 1.5; b.append(x)
    for at in [4 * lane + 1 for lane in range(8)] + [0, 31]:
        x = rnd(); x[at] = np.abs(x).max() * (1.25 if at % 8 else -1.25); b.append(x)
    x = np.arange(32, dtype=np.float32) - 16 + 0.5; x[0] = 127.0; b.append(x)                      # 127 / amax == 1: -14.5 .. 15.5
    x = (np.arange(32, dtype=np.float32) - 16 + 0.5) / 2; x[31] = -63.5; b.append(x)               # 127 / amax == 2: x * 2 == k + 0.5
    x = (np.arange(32, dtype=np.float32) * 4 + 0.5); x[1] = 1.5; x[2] = 2.5; x[0] = -127.0; b.append(x)      # up to 124.5, amax negative
    sub = rng.integers(1, 1 << 23, 32, dtype=np.uint64).astype(np.uint32).view(np.float32)          # subnormals, both signs, and zeros
    sub[::3] *= -1; sub[[4, 9]] = 0.0; sub[20] = -0.0; b.append(sub.copy())
    x = np.zeros(32, np.float32); x[13] = np.uint32(1).view(np.float32); b.append(x)               # amax the smallest subnormal
    x = rnd(1e-38); x[7] = 0.0; x[30] = 3.0e-37; b.append(x)                                     # normal amax, 127 / amax == inf
    x = rnd(1e-37); x[3] = 0.0; x[8] = np.float32(3.8e-37); b.append(x)                          # 127 / amax finite again
    x = rnd(2e6); x[17] = 65504.0 * 127 * 1.01; b.append(x)                                       # d above 65504 (below the tie at 65520), 65520 and beyond -> inf
    x = rnd(3e6); x[2] = -65520.0 * 127; b.append(x)
    x = rnd(1e30); x[9] = np.finfo(np.float32).max; b.append(x)
    b += [rnd(1e-3), rnd(1.0), rnd(40.0)]
    out = np.stack(b).astype(np.float32)
    assert np.isfinite(out).all()
    return out


def q8_source(nblk, seed):
    """[nblk, 32] float32: the special blocks (as many as fit, starting at a place that depends on the seed) spread over random blocks at 1e-3, 1 and 40"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((nblk, 32)) * np.array([1e-3, 1.0, 40.0])[rng.integers(0, 3, nblk)][:, None]).astype(np.float32)
    s = np.roll(q8_special_blocks(), -5 * seed, axis=0)
    k = min(len(s), nblk)
    x[(np.arange(k) * nblk) // k] = s[:k]
    return x


# ---- SET_ROWS --------------------------------------------------------------------------------------------------------------------------------
class SetRows:
    """src [ne0, n, ne2, ne3] F32 (dense, or a column block of a parent with wider rows) set into dst [ne0, rows, ne2, ne3] at idx [n (, i_ne1 (, i_ne2))];
    dst dense, or a view at a byte offset with padded rows.  Indices are distinct within a plane and in range"""

    def __init__(self, name, dst_type, src_ne, rows, idx_ne, idx_type=I64, src_pad=0, dst_pad=0, dst_offset=0):
        self.name, self.dst_type, self.src_ne, self.rows, self.idx_ne, self.idx_type = name, dst_type, list(src_ne) + [1] * (4 - len(src_ne)), rows, list(idx_ne), idx_type
        self.src_pad, self.dst_pad, self.dst_offset = src_pad, dst_pad, dst_offset
        self._built = None

    def __repr__(self):
        return self.name

    def build(self):
        """(dst0 bytes, dst View, src float32 buffer, src View, idx array, idx buffer with a tail of valid rows behind idx)"""
        if self._built is None:
            ne0, n, ne2, ne3 = self.src_ne
            seed = 5000 + sum((i + 3) * v for i, v in enumerate(self.src_ne + self.idx_ne)) + self.dst_type + self.rows
            rng = np.random.default_rng(seed)
            values = (q8_source(ne0 // 32 * n * ne2 * ne3, seed) if self.dst_type == Q8_0 else floats_with_edges(ne0 * n * ne2 * ne3, seed))
            left = 16 if self.src_pad else 0                                    # the column block starts 4 floats into the parent's rows
            sv, snb = padded_rows(self.src_ne, F32, self.src_pad, left)
            src = filled(sv, snb, values, 0x5a).view(np.float32)
            dv, dnb = padded_rows([ne0, self.rows, ne2, ne3], self.dst_type, self.dst_pad, self.dst_offset)
            size = R._BLOCK[self.dst_type][0]
            dst0 = rng.integers(0, 256, -(-(dnb + self.dst_offset) // size) * size, dtype=np.uint8)
            ishape = tuple(reversed(self.idx_ne))
            planes = int(np.prod(ishape[:-1]))
            idx = np.stack([rng.permutation(self.rows)[:n] for _ in range(planes)]).reshape(ishape).astype(NP_OF[self.idx_type])
            tail = rng.integers(0, self.rows, n * ne2 * ne3).astype(idx.dtype)          # read only by a wrong broadcast: in range, inside the buffer
            self._built = tuple(frozen(a) if isinstance(a, np.ndarray) else a for a in (dst0, dv, src, sv, idx, np.concatenate([idx.reshape(-1), tail])))
        return self._built


def set_rows_cases():
    c = []
    for t in (F16, F32):
        n = TYPE_NAME[t]
        for it in (I32, I64):
            for ne0 in (1, 7, 33, 1024):                 # the reference converts a row with a vector body and a scalar tail
                for rows in (1, 3, 9):
                    c.append(SetRows(f"{n}_{TYPE_NAME[it]}_ne0_{ne0}_rows_{rows}", t, [ne0, rows], 64, [rows], it))
            for idx_ne in ([5], [5, 4], [5, 2, 2], [5, 4, 2]):
                c.append(SetRows(f"{n}_{TYPE_NAME[it]}_broadcast_{'x'.join(map(str, idx_ne))}", t, [32, 5, 4, 2], 64, idx_ne, it))
        c.append(SetRows(f"{n}_source_column_block", t, [33, 5, 4, 2], 64, [5, 2, 1], I64, src_pad=28))
        c.append(SetRows(f"{n}_destination_view_at_an_offset", t, [33, 5, 2, 2], 16, [5, 2, 2], I32, dst_pad=24, dst_offset=40))
        c.append(SetRows(f"{n}_past_one_trip", t, [1024, 2100], 2100, [2100], I32))
    return c


def set_rows_q8_0_cases():
    c = []
    for ne0 in (32, 64, 128, 4096):
        for rows in (1, 3, 9):
            c.append(SetRows(f"q8_0_ne0_{ne0}_rows_{rows}", Q8_0, [ne0, rows], 64, [rows], I64))
    for rows in (7, 33, 257):                            # 7, 33, 257 blocks: no multiple of a wave's 8 nor of a workgroup's 32
        c.append(SetRows(f"q8_0_blocks_{rows}", Q8_0, [32, rows], 300, [rows], I32))
    for it in (I32, I64):
        for idx_ne in ([5], [5, 4], [5, 2, 2], [5, 4, 2]):
            c.append(SetRows(f"q8_0_{TYPE_NAME[it]}_broadcast_{'x'.join(map(str, idx_ne))}", Q8_0, [64, 5, 4, 2], 64, idx_ne, it))
    c.append(SetRows("q8_0_source_column_block", Q8_0, [64, 5, 4, 2], 64, [5, 2, 1], I64, src_pad=32))
    # rows of 68 bytes, 74 apart (2 * 37), the view 10 bytes into its buffer
    c.append(SetRows("q8_0_destination_view_at_an_offset", Q8_0, [64, 5, 2, 2], 16, [5, 2, 2], I32, dst_pad=6, dst_offset=10))
    # past one trip of 262 144 blocks.  [4096, 2049]: 262 272 blocks, the second trip holds 128 (16 whole waves).  [32, 262153]: the second trip holds 9, one whole
    # wave and one with a single live group -- the waves kept alive past nblk and clamped to block nblk - 1
    c.append(SetRows("q8_0_past_one_trip", Q8_0, [4096, 2049], 2049, [2049], I32))
    c.append(SetRows("q8_0_past_one_trip_partial_last_wave", Q8_0, [32, 262153], 262153, [262153], I32))
    return c


# ---- CPY / CONT ------------------------------------------------------------------------------------------------------------------------------
class Cpy:
    """src_view of the buffer src0 copied into dst_view of dst0 (both bytes); dst_view None: CONT"""

    def __init__(self, name, make):
        self.name, self._make, self._built = name, make, None

    def __repr__(self):
        return self.name

    def build(self):
        """(src0, src View, dst0 or None, dst View or None, nan: the elements of the destination's rows whose source is a NaN, or None)"""
        if self._built is None:
            out = self._make()
            self._built = tuple(frozen(a) if isinstance(a, np.ndarray) else a for a in (out + (None,))[:5])
        return self._built


def values_of(t, n, seed):
    rng = np.random.default_rng(seed)
    if t == F32:
        return floats_with_edges(n, seed)
    if t == F16:
        h = rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
        return np.where((h & 0x7fff) > 0x7c00, np.uint16(0x3c00), h).view(np.float16)          # no NaNs
    return rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)


def _dense_pair(ts, td, ne, seed):
    def make():
        sv, dv = View(ts, ne), View(td, ne)
        n = sv.nelements()
        return values_of(ts, n, seed).view(np.uint8), sv, np.random.default_rng(seed + 1).integers(0, 256, n * R._BLOCK[td][0], dtype=np.uint8), dv
    return make


def _all_halves():
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    nan = (h & 0x7fff) > 0x7c00
    assert int(nan.sum()) == 2046
    return h.view(np.uint8), View(F16, [256, 256]), np.zeros(65536 * 4, np.uint8), View(F32, [256, 256]), nan


def _permuted(t, axes):
    def make():
        v = View(t, [8, 4, 3, 2], axes=axes)
        return values_of(t, v.nelements(), 6000 + t).view(np.uint8), v, None, None
    return make


def _reshaped(ts, td):
    """[6, 4, 5] -> [10, 12], both column blocks of wider parents"""
    def make():
        sv, sn = padded_rows([6, 4, 5], ts, 3 * R._BLOCK[ts][0], 2 * R._BLOCK[ts][0])
        dv, dn = padded_rows([10, 12], td, 5 * R._BLOCK[td][0], 3 * R._BLOCK[td][0])
        src0 = filled(sv, sn, values_of(ts, 120, 6100 + ts * 3 + td), 0x11)
        return src0, sv, np.random.default_rng(6200).integers(0, 256, -(-dn // 4) * 4, dtype=np.uint8), dv
    return make


V_KD, V_QLEN, V_ML = 256, 5, 64


def _v_cache(n_past):
    """the V-cache write of test_cpy_v_cache_transposed_and_cont: v [KD, qlen] F32 transposed into columns n_past .. n_past + qlen of the F16 cache [ML, KD]"""
    def make():
        v = values_of(F32, V_KD * V_QLEN, 6300 + n_past)
        cache = np.random.default_rng(6301).standard_normal(V_KD * V_ML).astype(np.float16)
        return v.view(np.uint8), View(F32, [V_KD, V_QLEN], axes="transpose"), cache.view(np.uint8), View(F16, [V_QLEN, V_KD], [2, V_ML * 2, V_ML * V_KD * 2, V_ML * V_KD * 2], n_past * 2)
    return make


def _big_f32_f16():
    ne = [1000, 4200]                                     # 4 200 000 elements against 4 194 304 a trip
    return values_of(F32, 4200000, 6400).view(np.uint8), View(F32, ne), np.zeros(4200000 * 2, np.uint8), View(F16, ne)


def q8_rows(ne0, rows, seed):
    """quantized rows with every byte value among the quants and scales of every kind (bytes are only moved)"""
    return np.random.default_rng(seed).integers(0, 256, rows * R.row_bytes(Q8_0, ne0), dtype=np.uint8)


def _q8_permuted(strided):
    def make():
        sv = View(Q8_0, [128, 5, 3], axes=(0, 2, 1, 3))                       # -> [128, 3, 5]
        src0 = q8_rows(128, 15, 6500)
        if not strided:
            return src0, sv, np.random.default_rng(6501).integers(0, 256, src0.nbytes, dtype=np.uint8), View(Q8_0, [128, 3, 5])
        dv, dn = padded_rows([128, 3, 5] if strided == "same_shape" else [128, 5, 3], Q8_0, 6, 34)          # or rows regrouped: row e of one to row e of the other
        return src0, sv, np.random.default_rng(6502).integers(0, 256, -(-dn // 34) * 34, dtype=np.uint8), dv
    return make


def _q8_big():
    """[4096, 965, 2] through permute(0, 2, 1, 3): 1930 rows of 2176 two-byte units, 4 199 680 against 4 194 304 a trip"""
    src0 = q8_rows(4096, 1930, 6600)
    return src0, View(Q8_0, [4096, 965, 2], axes=(0, 2, 1, 3)), np.zeros(src0.nbytes, np.uint8), View(Q8_0, [4096, 2, 965])


def cpy_cases():
    c = []
    for ne0 in (1, 7, 8, 9, 33):
        c.append(Cpy(f"f32_f16_ne0_{ne0}", _dense_pair(F32, F16, [ne0, 5, 3, 2], 6700 + ne0)))
        c.append(Cpy(f"f16_f32_ne0_{ne0}", _dense_pair(F16, F32, [ne0, 5, 3, 2], 6800 + ne0)))
    c.append(Cpy("f16_f32_all_65536_halves", _all_halves))
    for t in (F32, F16, I32):
        for axes in ((0, 2, 1, 3), (1, 0, 2, 3), "transpose"):
            c.append(Cpy(f"cont_{TYPE_NAME[t]}_{axes if isinstance(axes, str) else 'permute_' + ''.join(map(str, axes))}", _permuted(t, axes)))
    for ts, td in ((F32, F32), (F32, F16), (F16, F32), (F16, F16), (I32, I32)):
        c.append(Cpy(f"reshaped_strided_{TYPE_NAME[ts]}_{TYPE_NAME[td]}", _reshaped(ts, td)))
    c += [Cpy("v_cache_n_past_0", _v_cache(0)), Cpy(f"v_cache_n_past_{V_ML - V_QLEN}", _v_cache(V_ML - V_QLEN))]
    c.append(Cpy("f32_f16_past_one_trip", _big_f32_f16))
    c += [Cpy("q8_0_permuted_into_dense", _q8_permuted(False)), Cpy("q8_0_permuted_into_strided", _q8_permuted("same_shape")),
          Cpy("q8_0_permuted_into_strided_of_another_shape", _q8_permuted("regrouped")), Cpy("q8_0_past_one_trip", _q8_big)]
    return c


# ---- GET_ROWS --------------------------------------------------------------------------------------------------------------------------------
class GetRows:
    """table [ne0, rows, ne2, ne3] of `type_`, idx an I32 view [n, ne2, ne3] of a buffer: dense, with padded rows at an offset, or transposed (nb[0] != 4)"""

    def __init__(self, name, type_, ne, n, form):
        self.name, self.type, self.ne, self.n, self.form, self._built = name, type_, list(ne) + [1] * (4 - len(ne)), n, form, None

    def __repr__(self):
        return self.name

    def build(self):
        """(table bytes, idx buffer int32, idx View)"""
        if self._built is None:
            ne0, rows, ne2, ne3 = self.ne
            rng = np.random.default_rng(7000 + self.type + 31 * self.n)
            if self.type in (F32, F16):
                table = (rng.standard_normal(ne0 * rows * ne2 * ne3) * 3).astype(NP_OF[self.type]).view(np.uint8)
            else:
                table = rand_blocks(self.type, rows * ne2 * ne3, ne0, rng).reshape(-1)
            ids = rng.integers(0, rows, (ne3, ne2, self.n)).astype(np.int32)        # repeats allowed: reads
            ids[0, 0, 0], ids[-1, -1, -1], ids[0, -1, 0] = 0, rows - 1, rows - 1
            if self.n > 1:
                ids[0, 0, 1] = ids[0, 0, 0]
            if self.form == "dense":
                v = View(I32, [self.n, ne2, ne3])
                buf = ids.reshape(-1).copy()
            elif self.form == "padded":
                v, nbytes = padded_rows([self.n, ne2, ne3], I32, 12, 8)
                buf = filled(v, nbytes, ids, 0x7f).view(np.int32)                  # 0x7f7f7f7f between the rows: out of range
            else:                                                                  # ids stored [ne3, n, ne2]; the view's dims 0 and 1 swapped
                v = View(I32, [ne2, self.n, ne3], axes="transpose")
                buf = np.ascontiguousarray(ids.transpose(0, 2, 1)).reshape(-1)
            self._built = (frozen(table), frozen(buf), v)
        return self._built


def get_rows_cases():
    c = [GetRows(f"{TYPE_NAME[t]}_batched_{form}", t, [256, 6, 3, 2], 4, form) for t in (F32, F16, Q8_0, Q4_0, Q4_K, Q6_K) for form in ("dense", "padded", "transposed")]
    c += [GetRows(f"{TYPE_NAME[t]}_past_one_trip", t, [1024, 64], 2100, "dense") for t in (F32, Q8_0)]          # 2 150 400 destination elements
    return c


# ---- SOFT_MAX with a mask ------------------------------------------------------------------------------------------------------------------------
SOFT_N0 = [1, 7, 8, 13, 40, 520]
SOFT_X_NE = [5, 4, 2]                                       # ne1, ne2, ne3 of x
SOFT_MASKS = [[5], [8], [5, 2, 1], [5, 4, 2], [5, 1, 2]]   # ne1 (, ne2, ne3) of the mask: 2-D, padded (ne1 > x's), broadcast over ne2 / ne3, full
SOFT_SCALES = [1.0, 0.125]
SOFT_DEAD_ROW = 3                                           # the mask row i1 == 3 of the mask's LAST (i2, i3) plane is -inf in every column


class SoftMax:
    def __init__(self, n0, mask_ne, scale):
        self.n0, self.mask_ne, self.scale, self._built = n0, list(mask_ne) + [1] * (3 - len(mask_ne)), scale, None
        self.name = f"n0_{n0}_mask_{'x'.join(map(str, mask_ne))}_scale_{scale}"

    def __repr__(self):
        return self.name

    def dead_rows(self):
        """the rows of x (bool [ne3, ne2, ne1]) whose every column is masked: named from the shapes alone.  The reference's result there is NaN"""
        n1, n2, n3 = SOFT_X_NE
        _, m2, m3 = self.mask_ne
        dead = np.zeros((n3, n2, n1), bool)
        for i3 in range(n3):
            for i2 in range(n2):
                dead[i3, i2, SOFT_DEAD_ROW] = (i2 % m2 == m2 - 1) and (i3 % m3 == m3 - 1)
        return dead

    def build(self):
        """(x float32 [2, 4, 5, n0], mask float32 [m3, m2, m1, n0], a buffer that holds the mask followed by a tail of zeros): the mask's values are 0, -inf
        and multiples of 1 / 8 in [-16, 4], all exact in fp16"""
        if self._built is None:
            n1, n2, n3 = SOFT_X_NE
            m1, m2, m3 = self.mask_ne
            rng = np.random.default_rng(8000 + self.n0 + 7 * m1 + 13 * m2 + 17 * m3)
            x = (rng.standard_normal((n3, n2, n1, self.n0)) * 3).astype(np.float32)
            kind = rng.random((m3, m2, m1, self.n0))
            mask = np.where(kind < 0.3, -np.inf, np.where(kind < 0.5, 0.0, rng.integers(-128, 33, kind.shape) / 8.0)).astype(np.float32)
            keep = rng.integers(0, self.n0, (m3, m2, m1))                         # one column of every row stays visible ...
            live = np.take_along_axis(mask, keep[..., None], -1)
            np.put_along_axis(mask, keep[..., None], np.where(np.isinf(live), np.float32(-0.5), live), -1)
            mask[m3 - 1, m2 - 1, SOFT_DEAD_ROW, :] = -np.inf                       # ... but this one's
            assert np.array_equal(mask.astype(np.float16).astype(np.float32), mask)
            self._built = (frozen(x), frozen(mask), frozen(np.concatenate([mask.reshape(-1), np.zeros(x.size, np.float32)])))
        return self._built


def soft_max_cases():
    return [SoftMax(n0, m, s) for n0 in SOFT_N0 for m in SOFT_MASKS for s in SOFT_SCALES]
