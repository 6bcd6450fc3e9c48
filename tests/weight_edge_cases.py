"""Weight blocks whose SCALE FIELDS are what real model files hold and synth_helpers.rand_blocks never writes: negative, fp16-subnormal, zero and maximal scales, and
blocks whose every decoded integer is the format's largest.  Shared by tests/test_weight_edge_model.py (CPU: the oracle against the reference build, word for word)
and tests/test_gpu_weight_edges.py (the kernels against the oracle).  Plain numpy; finite scale fields only (a file with an fp16 inf / NaN scale is refused on load).

edge_blocks(t, rows, K, rng, profile) is rand_blocks(t, rows, K, rng) with only the scale fields overwritten (`saturated` overwrites the quants and the packed
integer sub-scales instead).  The fp16 fields of a block are listed once, in FIELDS, and held against TYPE_SIZE below.

Profiles (every fp16 field of the type is treated alike; MXFP4 has one E8M0 exponent byte instead):
  signed     rand_blocks' magnitudes, the sign of each field drawn per block; block 0 of every row is positive and block 1 negative in every field, so both signs meet
             in one row and in the first pair of blocks (the codebook formats accumulate blocks 2i and 2i + 1 in two accumulators)
  subnormal  half of the blocks keep their normal scale; the others take a bit pattern 0x0001..0x03ff with either sign.  0x0001, 0x03ff and 0x0400 (the smallest
             normal) are forced into blocks 0, 1, 2 of every row.  A row of two blocks (K = 512 of a 256-element format) cannot hold three: there row r takes
             pattern r mod 3 in block r mod 2, so any three neighbouring rows hold all three, and its other block stays drawn (normal or subnormal).
             MXFP4: exponent bytes 0..3
  zero       +0 in a third of the blocks, -0 in another third (drawn per field: a type with a minimum gets d == 0 with dmin != 0 and the reverse; blocks 0 / 1 of
             row 2 are forced to those two); row 0 is all zero blocks, row 1 all zero but its last block.  MXFP4 has no zero scale: it takes exponent byte 0
  large      magnitudes from 2^10 up to 0x7bff (65504), either sign, 0x7bff and 0xfbff forced into blocks 0 and 1 of every row.  MXFP4: bytes 124..200 for mat-mul
             (for_get_rows=True: the whole range 0..255, whose top decodes to +-inf)
  saturated  rand_blocks' scales; every quant byte and packed sub-scale at the pattern that decodes to the largest magnitude (see _saturate)
  tiny       (mat-mul only) `subnormal`, and every third row (0, 3, ..) holds nothing but the patterns 0x0001..0x0003, with tiny_activations: for the 15 formats
             with Q8_K activations the scale products d_w * d_x are fp32 subnormals and those rows' sums are nonzero fp32 subnormals; for the 7 formats with
             Q8_0 / Q8_1 activations (ACT_FP16_SCALE) the activation scale itself rounds to zero in fp16 and every output is +-0 (see tiny_activations)

Shapes: shapes_of / M_VALUES / GET_ROWS_SHAPE -- the smallest that reach every code path (two super-blocks; an unpaired last 32-block at K = 96; an odd row count;
one column, a column chunk, and 40 columns where mmx.hip takes the four tuned types).  The forced one-column forms of the 32-block types take only some shapes
(gemv_rows32.hip: rows a multiple of the rows per wave and whole dwords; gemv_team32.hip: rows a multiple of 8, K >= 256 and a step per emit wave, K >= 800 for
teams of 5), anything else falls back to k_gemv_dec without a word: ROWS32_SHAPES and TEAM32_SHAPES are shapes they take."""
import numpy as np

from synth_helpers import BLCK, TYPE_SIZE, rand_blocks

F32, F16, I32 = 0, 1, 26
Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 2, 3, 6, 7, 8, 10, 11, 12, 13, 14
IQ2_XXS, IQ2_XS, IQ3_XXS, IQ1_S, IQ4_NL, IQ3_S, IQ2_S, IQ4_XS, IQ1_M, TQ1_0, TQ2_0, MXFP4 = 16, 17, 18, 19, 20, 21, 22, 23, 29, 34, 35, 39
TUNED = (Q4_K, Q4_0, Q4_1, Q8_0)
ALL_TYPES = TUNED + (Q5_K, Q6_K, Q2_K, Q3_K, IQ4_XS, TQ1_0, TQ2_0, IQ2_XXS, IQ2_XS, IQ2_S, IQ3_XXS, IQ3_S, IQ1_S, IQ1_M, Q5_0, Q5_1, IQ4_NL, MXFP4)
TYPE_NAME = {Q4_0: "q4_0", Q4_1: "q4_1", Q5_0: "q5_0", Q5_1: "q5_1", Q8_0: "q8_0", Q2_K: "q2_k", Q3_K: "q3_k", Q4_K: "q4_k", Q5_K: "q5_k", Q6_K: "q6_k",
             IQ2_XXS: "iq2_xxs", IQ2_XS: "iq2_xs", IQ3_XXS: "iq3_xxs", IQ1_S: "iq1_s", IQ4_NL: "iq4_nl", IQ3_S: "iq3_s", IQ2_S: "iq2_s", IQ4_XS: "iq4_xs",
             IQ1_M: "iq1_m", TQ1_0: "tq1_0", TQ2_0: "tq2_0", MXFP4: "mxfp4", F16: "f16"}

# byte offsets of the fp16 fields of a block: d first, then the minimum (m / dmin) where the type has one.  IQ1_M scatters its one fp16 over the top nibbles of
# the four 16-bit scale words at 48..55 ("nibbles"); MXFP4 has an E8M0 exponent byte at 0 and no fp16 ("e8m0")
FIELDS = {Q4_0: (0,), Q5_0: (0,), Q8_0: (0,), IQ4_NL: (0,), IQ4_XS: (0,), IQ2_XXS: (0,), IQ2_XS: (0,), IQ2_S: (0,), IQ3_XXS: (0,), IQ3_S: (0,), IQ1_S: (0,),
          Q4_1: (0, 2), Q5_1: (0, 2), Q4_K: (0, 2), Q5_K: (0, 2), Q2_K: (80, 82), Q3_K: (108,), Q6_K: (208,), TQ1_0: (52,), TQ2_0: (64,),
          IQ1_M: "nibbles", MXFP4: "e8m0"}
assert set(FIELDS) == set(ALL_TYPES) and len(ALL_TYPES) == 22
for _t, _f in FIELDS.items():
    assert _f in ("nibbles", "e8m0") or all(o % 2 == 0 and o + 2 <= TYPE_SIZE[_t] for o in _f), _t
    if _t in (Q2_K, Q3_K, Q6_K, TQ1_0, TQ2_0):          # the scale closes the block
        assert _f[-1] + 2 == TYPE_SIZE[_t], _t
assert TYPE_SIZE[IQ1_M] == 56 and TYPE_SIZE[MXFP4] == 17

PROFILES = ("signed", "subnormal", "zero", "large", "saturated", "tiny")
GET_ROWS_PROFILES = ("signed", "subnormal", "zero", "large", "saturated")
M_VALUES = (1, 5, 40)
GET_ROWS_SHAPE = (12, 5)          # table rows, indices
FORCED_SUB = (0x0001, 0x03ff, 0x0400)
ACT_FP16_SCALE = (Q4_0, Q4_1, Q8_0, Q5_0, Q5_1, IQ4_NL, MXFP4)          # dot products over Q8_0 / Q8_1 activations: the activation block scale is an fp16
ROWS32_SHAPES = [(512, 20)]                   # 20 rows: whole waves of 2 and of 4 rows; K = 512: rows of whole dwords in all three formats
TEAM32_SHAPES = [(1024, 8), (1024, 24)]       # one and three units of 8 rows; 32 blocks: four steps of eight, one per emit wave of a team of 4 or 5


def shapes_of(t):
    """(K, N) of the mat-mul cases of a type"""
    return [(512, 20), (512, 7)] if BLCK[t] == 256 else [(96, 20), (512, 7), (512, 20)]


def n_fields(t):
    return 1 if isinstance(FIELDS[t], str) else len(FIELDS[t])


def get_fields(t, blocks, K):
    """the fp16 fields of rows of block bytes as uint16 [rows, nb, fields] (MXFP4: the exponent bytes)"""
    rows, nb = blocks.shape[0], K // BLCK[t]
    b = blocks.reshape(rows, nb, TYPE_SIZE[t])
    f = FIELDS[t]
    if f == "e8m0":
        return b[:, :, 0:1].astype(np.uint16)
    if f == "nibbles":
        sc = np.ascontiguousarray(b[:, :, 48:56]).view(np.uint16).reshape(rows, nb, 4).astype(np.uint32)
        return (((sc[..., 0] >> 12) | ((sc[..., 1] >> 12) << 4) | ((sc[..., 2] >> 12) << 8) | ((sc[..., 3] >> 12) << 12)).astype(np.uint16))[..., None]
    return np.stack([b[:, :, o].astype(np.uint16) | (b[:, :, o + 1].astype(np.uint16) << 8) for o in f], axis=-1)


def put_fields(t, blocks, K, v):
    """write uint16 [rows, nb, fields] into the fp16 fields (in place)"""
    rows, nb = blocks.shape[0], K // BLCK[t]
    b = blocks.reshape(rows, nb, TYPE_SIZE[t])
    f = FIELDS[t]
    v = np.asarray(v, np.uint16)
    if f == "e8m0":
        b[:, :, 0] = v[..., 0].astype(np.uint8)
    elif f == "nibbles":
        sc = np.ascontiguousarray(b[:, :, 48:56]).view(np.uint16).reshape(rows, nb, 4)
        for k in range(4):
            sc[:, :, k] = (sc[:, :, k] & 0x0fff) | (((v[..., 0] >> (4 * k)) & 0xf) << 12)
        b[:, :, 48:56] = sc.view(np.uint8).reshape(rows, nb, 8)
    else:
        for i, o in enumerate(f):
            b[:, :, o] = (v[..., i] & 0xff).astype(np.uint8)
            b[:, :, o + 1] = (v[..., i] >> 8).astype(np.uint8)


def _saturate(t, b, rng):
    """b [rows, nb, TYPE_SIZE] in place: every decoded integer at the format's largest magnitude, the scale fields untouched.  Ones everywhere is that pattern for most
    formats (nibbles 15, 6-bit scales and mins 63, the grid formats' top index with every sign set, trits 2, MXFP4's code 15 = -12); where the all-zero pattern
    decodes further from zero (Q4_0: -8 against 7, Q5_0: -16 against 15, Q6_K: -32 against 31, IQ4_NL: -127 against 113, Q3_K: -4 * -32 against 3 * 31, IQ4_XS: -127 * -32) odd blocks
    take zeros; Q8_0 blocks are all -128 or all +127; Q6_K's int8 sub-scales are -128 and 127 in turn; TQ2_0 takes 2-bit values 2 (+1), the largest a file holds"""
    rows, nb = b.shape[:2]
    keep = get_fields(t, b.reshape(rows, -1), nb * BLCK[t])
    b[:] = 0xff
    if t in (Q4_0, Q5_0, IQ4_NL, Q3_K, IQ4_XS, Q6_K):
        b[:, 1::2] = 0
    if t == Q8_0:
        b[:, :, 2:34] = np.where(rng.random((rows, nb, 1)) < 0.5, 0x80, 0x7f).astype(np.uint8)
        b[:, :2, 2:34] = np.array([0x80, 0x7f], np.uint8)[None, : min(nb, 2), None]
    if t == Q6_K:
        b[:, :, 192:208] = np.tile(np.array([0x80, 0x7f], np.uint8), 8)
        b[:, 1::2, 192:208] = np.tile(np.array([0x7f, 0x80], np.uint8), 8)
    if t == TQ2_0:
        b[:, :, :64] = 0xaa
    put_fields(t, b.reshape(rows, -1), nb * BLCK[t], keep)


def edge_blocks(t, rows, K, rng, profile, for_get_rows=False):
    """rand_blocks(t, rows, K, rng) with the scale fields of `profile` (module docstring): block bytes [rows, row bytes]"""
    assert profile in PROFILES and K % BLCK[t] == 0
    out = rand_blocks(t, rows, K, rng)
    nb, nf = K // BLCK[t], n_fields(t)
    if profile == "saturated":
        _saturate(t, out.reshape(rows, nb, TYPE_SIZE[t]), rng)
        return out
    v = get_fields(t, out, K)
    shape = (rows, nb, nf)
    if t == MXFP4:
        if profile == "signed":
            return out                                            # a power of two has no sign: rand_blocks' exponents
        if profile in ("subnormal", "tiny"):
            v = rng.integers(0, 4, shape).astype(np.uint16)
            v[:, : min(nb, 3), 0] = np.array([0, 1, 3], np.uint16)[: min(nb, 3)]
        elif profile == "zero":
            v[rng.random(shape) < 2 / 3] = 0
            v[0] = 0
            v[1, : nb - 1] = 0
        else:
            v = rng.integers(0, 256, shape).astype(np.uint16) if for_get_rows else rng.integers(124, 201, shape).astype(np.uint16)
            v[:, 0, 0] = 255 if for_get_rows else 200
            if nb > 1:
                v[:, 1, 0] = 0 if for_get_rows else 124
        put_fields(t, out, K, v)
        return out
    sign = (rng.integers(0, 2, shape) << 15).astype(np.uint16)
    if profile == "signed":
        sign[:, 0] = 0
        if nb > 1:
            sign[:, 1] = 0x8000
        v = (v & 0x7fff) | sign
    elif profile in ("subnormal", "tiny"):
        sub = rng.random((rows, nb, 1)) < 0.5
        v = np.where(sub, rng.integers(1, 0x400, shape).astype(np.uint16) | sign, v)
        for r in range(rows):
            pats = dict(enumerate(FORCED_SUB)) if nb >= 3 else {r % nb: FORCED_SUB[r % 3]}
            for i, p in pats.items():
                v[r, i] = p | (sign[r, i] if p != 0x0400 else 0)
        if profile == "tiny":
            v[0::3] = rng.integers(1, 4, v[0::3].shape).astype(np.uint16) | sign[0::3]
    elif profile == "zero":
        u = rng.random(shape)
        v = np.where(u < 1 / 3, 0, np.where(u < 2 / 3, 0x8000, v)).astype(np.uint16)
        v[0] = sign[0]                                            # every block of row 0: +0 or -0
        v[1, : nb - 1] = sign[1, : nb - 1]
        v[1, nb - 1] = get_fields(t, out, K)[1, nb - 1]           # ... of row 1 but the last, which keeps its scale
        if nf == 2 and rows > 2 and nb > 1:
            keep = get_fields(t, out, K)[2]
            v[2, 0] = (0x8000, keep[0, 1])                        # d == -0, dmin != 0
            v[2, 1] = (keep[1, 0], 0)                             # d != 0, dmin == +0
    else:                                                         # large
        v = rng.integers(0x6400, 0x7c00, shape).astype(np.uint16) | sign
        v[:, 0] = 0x7bff
        if nb > 1:
            v[:, 1] = 0xfbff
    put_fields(t, out, K, v)
    return out


def f16_table(rows, n0, profile, rng):
    """an F16 GET_ROWS table with the same patterns as the scale fields: uint16 [rows, n0] viewed as float16"""
    v = rng.standard_normal((rows, n0)).astype(np.float16).view(np.uint16)
    sign = (rng.integers(0, 2, v.shape) << 15).astype(np.uint16)
    if profile == "subnormal":
        v = np.where(rng.random(v.shape) < 0.5, rng.integers(1, 0x400, v.shape).astype(np.uint16) | sign, v)
        v[:, :3] = FORCED_SUB
    elif profile == "zero":
        u = rng.random(v.shape)
        v = np.where(u < 1 / 3, 0, np.where(u < 2 / 3, 0x8000, v)).astype(np.uint16)
        v[0] = sign[0]
    elif profile in ("large", "saturated"):
        v = rng.integers(0x6400, 0x7c00, v.shape).astype(np.uint16) | sign
        v[:, 0], v[:, 1] = 0x7bff, 0xfbff
    return np.ascontiguousarray(v).view(np.float16)


def activations(t, M, K, rng, profile):
    """float32 [M, K].  saturated: +1 or -1, constant over a block of the type, so every Q8 quant is +-127 and the integer block sums are the largest there are;
    tiny: tiny_activations; every other profile: standard normal"""
    if profile == "saturated":
        s = np.where(rng.random((M, K // BLCK[t], 1)) < 0.5, -1.0, 1.0)
        s[:, :2, 0] = np.array([1.0, -1.0])[: min(2, K // BLCK[t])]
        return np.ascontiguousarray(np.broadcast_to(s, (M, K // BLCK[t], BLCK[t])).reshape(M, K)).astype(np.float32)
    if profile == "tiny":
        return tiny_activations(M, K, rng)
    return rng.standard_normal((M, K)).astype(np.float32)


def tiny_activations(M, K, rng):
    """odd tokens: standard normal times 2^-113; even tokens (so the one token of M = 1 too): +-2^-119 times uniform(0.25, 1) with one +-2^-119 per 32-block -- as
    small as the activation quantizer takes: below amax = 2^-120 its 127 / amax overflows (that case belongs to the Q8_0 tests), and the builder asserts every
    32-block's amax above that.  With Q8_K activations (fp32 block scale, about 2^-126 and 2^-120) every scale product d_w * d_x is an fp32 subnormal for the even
    tokens, and their sums over the rows of patterns 0x0001..0x0003 are nonzero fp32 subnormals.  With Q8_0 / Q8_1 activations the block scale is an fp16 and
    rounds to zero: every output of those formats (ACT_FP16_SCALE) is +-0, and what their `tiny` cases hold is that flush and the sign of a zero sum, nothing more
    (d_x is 0 whatever d_w is; at a d_x that fp16 can hold, two fp16 scales give 2^-48 at the least, and no fp32 subnormal is reachable)"""
    x = rng.standard_normal((M, K)) * 2.0 ** -113
    small = rng.uniform(0.25, 1.0, (M, K)) * np.where(rng.random((M, K)) < 0.5, -1.0, 1.0) * 2.0 ** -119
    small[:, ::32] = np.where(rng.random((M, K // 32)) < 0.5, -1.0, 1.0) * 2.0 ** -119
    x[0::2] = small[0::2]
    x = x.astype(np.float32)
    assert np.all(np.abs(x.reshape(M, K // 32, 32)).max(-1) > 2.0 ** -120)
    return x


def seed_of(*key):
    return [int(k) if not isinstance(k, str) else sum(ord(c) * (i + 1) for i, c in enumerate(k)) for k in key]


def mat_mul_case(t, profile, K, N, M):
    """seeded inputs of one mat-mul case: weight bytes [N, row bytes], activations [M, K]; built once, read-only"""
    rng = np.random.default_rng(seed_of(t, profile, K, N, M))
    w = edge_blocks(t, N, K, rng, profile)
    x = activations(t, M, K, rng, profile)
    w.setflags(write=False)
    x.setflags(write=False)
    return w, x


def get_rows_case(t, profile, n0):
    """-> table (block bytes [rows, row bytes], or float16 [rows, n0] for F16), ids int32 [5] (a row twice, the first and the last row)"""
    rows, n = GET_ROWS_SHAPE
    rng = np.random.default_rng(seed_of(t, profile, n0, 77))
    table = f16_table(rows, n0, profile, rng) if t == F16 else edge_blocks(t, rows, n0, rng, profile, for_get_rows=True)
    ids = np.array([rows - 1, 0, 2, 1, 2], np.int32)[:n]
    table.setflags(write=False)
    return table, ids


def get_rows_widths(t):
    return (512,) if t == F16 or BLCK[t] == 256 else (96, 512)
