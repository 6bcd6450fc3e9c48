"""The inputs of the weight-quantizer tests (from_float_ref of Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q4_K and F16), shared by tests/test_weight_quant_model.py
(CPU: oracle, numpy mirror and the reference build) and tests/test_gpu_weight_quant.py (cllm_op_quantize_rows on the device).  Pure numpy, seeded: every
call returns the same floats.  Every case is a named float32 array [rows, K] with K the smallest that reaches the behaviour: 32 for one block, 256 for one
Q4_K super-block, the block count times that for the launch geometries.

special_blocks()         named 32-weight blocks, ONE list for all types: each type-specific block (a scale on an fp16 edge of Q5_0, say) is an ordinary input
                         of the other types, so nothing is lost by running all of them everywhere
q4k_super_blocks()       named 256-weight super-blocks: every special block as a sub-block (position i mod 8, Gaussian neighbours), the special blocks eight
                         at a time, and the Q4_K-only constructions
geometry(t, nb, layout, scale)   nb blocks as one row or as nb rows of one block: Gaussian at `scale` with key special blocks laid first, last and on both
                         sides of the workgroup boundary (256 threads: 256 blocks of 32 weights, 32 super-blocks)
f16_cases()              the F16 conversions: every half, every midpoint of adjacent halves with its float neighbours, the thresholds, the NaNs

The overflow class: 1 / d is inf for |d| < 2^-128 -- and already for d slightly above it, where the quotient rounds up past FLT_MAX.  THRESHOLD[t] is the
block maximum (Q8_0, Q4_0, Q5_0) or range (Q4_1, Q5_1) at which d == 2^-128."""
import functools

import numpy as np

import oracle as O

F = np.float32
B32_TYPES = (O.Q8_0, O.Q4_0, O.Q4_1, O.Q5_0, O.Q5_1)
SIGNED_TYPES = (O.Q8_0, O.Q4_0, O.Q5_0)
TYPES = B32_TYPES + (O.Q4_K, O.F16)
NAME = {O.Q8_0: "q8_0", O.Q4_0: "q4_0", O.Q4_1: "q4_1", O.Q5_0: "q5_0", O.Q5_1: "q5_1", O.Q4_K: "q4_K", O.F16: "f16"}
SCALES = (1.0, 1e-3, 40.0)
DIVISOR = {O.Q8_0: 127.0, O.Q4_0: 8.0, O.Q5_0: 16.0, O.Q4_1: 15.0, O.Q5_1: 31.0}          # |d| = (block maximum or range) / DIVISOR
THRESHOLD = {t: DIVISOR[t] * 2.0 ** -128 for t in B32_TYPES}                               # 3.73e-37, 2.35e-38, 4.70e-38; ranges 4.41e-38, 9.11e-38

# stored scales on the edges of fp16: (d, the half it must round to)
D_EDGES = (
    (2.0 ** -25 * (1 - 2.0 ** -10), 0x0000),      # below half of the smallest subnormal: 0
    (2.0 ** -25, 0x0000),                          # the halfway point between 0 and 2^-24: to even, 0
    (2.0 ** -25 * (1 + 2.0 ** -10), 0x0001),      # just above it
    (2.0 ** -24 * (1 - 2.0 ** -10), 0x0001),      # just below the smallest subnormal
    (2.0 ** -24 * (1 + 2.0 ** -10), 0x0001),      # just above it
    (1.5 * 2.0 ** -24, 0x0002),                    # halfway 1 | 2: to even
    (2.5 * 2.0 ** -24, 0x0002),                    # halfway 2 | 3: to even
    (2.0 ** -14 * (1 - 2.0 ** -11), 0x0400),      # halfway between the largest subnormal and the smallest normal half
    (1 + 2.0 ** -11, 0x3c00),                      # halfway 1 | 1 + 2^-10: to even
    (1 + 3 * 2.0 ** -11, 0x3c02),                  # halfway, odd below: up
    (65504.0, 0x7bff),                             # the largest half
    (65519.0, 0x7bff),                             # just below where fp16 becomes inf
    (65520.0, 0x7c00),                             # halfway 65504 | 65536: inf
)


def _pattern(rng, top=1.0):
    """32 factors in [-0.9, 0.9] with eight zeros and one element (index 7) of magnitude exactly 1"""
    p = rng.uniform(-0.9, 0.9, 32)
    p[rng.choice(32, 8, replace=False)] = 0.0
    p[7] = top
    return p


def block_with_scale(t, d, rng):
    """a block whose scale, as type t computes it, is d (up to the roundings of DIVISOR * d and of the quotient: exact for the D_EDGES)"""
    p = _pattern(rng)
    if t in SIGNED_TYPES:
        p[7] = 1.0 if t == O.Q8_0 else -1.0            # d = max / -8, / -16: a negative maximum stores a positive scale
        return (p * (DIVISOR[t] * d)).astype(F)
    v = np.abs(p) * (DIVISOR[t] * d)                   # min 0 (the zeros), max DIVISOR * d
    return v.astype(F)


@functools.lru_cache(None)
def special_blocks():
    """[(name, float32[32])]; no NaN, no inf.  Cached: treat the arrays as read-only"""
    rng = np.random.default_rng(20240)
    out = []

    def add(name, v):
        v = np.asarray(v, np.float64).astype(F).reshape(32).copy()
        assert np.isfinite(v).all(), name
        out.append((name, v))

    z = np.zeros(32)
    add("zero", z)
    add("neg_zero", -z)
    add("const_pos", z + 0.37)
    add("const_neg", z - 0.37)
    for p in (0, 15, 16, 31):
        for sgn, tag in ((1.0, "pos"), (-1.0, "neg")):
            v = z.copy()
            v[p] = 1.7 * sgn
            add(f"one_{tag}_at_{p}", v)
    # the block maximum twice, with opposite signs: the first decides the sign of d.  (-a, +a) is also the clamp case: +a lands on 16.5 -> 16 (Q5_0: 32.5 -> 32)
    for tag, (p, q) in (("lo", (3, 9)), ("hi", (19, 27)), ("cross", (5, 21))):
        for first, name in ((1.0, "pn"), (-1.0, "np")):
            v = np.clip(rng.standard_normal(32) * 0.5, -2.0, 2.0)
            v[p], v[q] = 2.5 * first, -2.5 * first
            add(f"tie_{name}_{tag}", v)
    add("clamp_neg_max", np.linspace(-2.5, 2.5, 32))                  # v[0] = -2.5 is the first maximum, v[31] = +2.5 the element that needs the clamp
    add("all_pos_offset", np.abs(rng.standard_normal(32)) + 3.0)
    add("all_neg", -np.abs(rng.standard_normal(32)) - 0.1)
    v = z + 0.37; v[11] = 0.91
    add("flat_but_one_high", v)
    v = z + 0.37; v[20] = -0.2
    add("flat_but_one_low", v)
    # x * id + off exactly on integers and exactly on .5: blocks whose scale is +-1
    k = np.arange(32)
    v = (k - 16) * 0.5; v[0] = 127.0
    add("grid_q8_0_id1", v)                                           # roundf: halves away from zero
    v = (k - 16) * 0.5; v[0] = -8.0
    add("grid_q4_0_d1", v)
    v = (k - 16) * 0.5; v[0] = 8.0
    add("grid_q4_0_dm1", v)                                           # d = -1
    v = (k - 16) + 0.5 * (k % 2); v[0] = -16.0
    add("grid_q5_0_d1", v)
    v = np.minimum(k * 0.5, 15.0); v[31] = 15.0
    add("grid_q4_1_d1", v)                                            # also Q4_K's first grid (iscale = 1): k + 0.5 are ties of nearest_int, to even
    v = k - 0.5 * (k % 2); v[31] = 31.0
    add("grid_q5_1_d1", v)
    # stored scales on the fp16 edges, per type
    for t in B32_TYPES:
        for i, (d, _) in enumerate(D_EDGES):
            add(f"d_edge_{NAME[t]}_{i}", block_with_scale(t, d, rng))
    # the offset formats: a minimum that overflows fp16 next to a scale that does not, and the reverse
    v = -70000.0 + np.abs(_pattern(rng)) * 15.0
    add("m_inf_d_finite", v)
    for t in (O.Q4_1, O.Q5_1):
        add(f"d_inf_m_finite_{NAME[t]}", -100.0 + np.abs(_pattern(rng)) * DIVISOR[t] * 65520.0)
    # the overflow class: 1 / d is inf.  Per type: half the threshold (positive and negative maximum), the threshold itself, just above it (1 / d still rounds to inf),
    # and the control one binade up
    for t in B32_TYPES:
        thr = THRESHOLD[t]
        for tag, amax, sgn in (("below", thr / 2, 1.0), ("below_neg", thr / 2, -1.0), ("quarter", thr / 4, 1.0), ("at", thr, 1.0), ("above", thr * 2, 1.0), ("above_neg", thr * 2, -1.0)):
            p = _pattern(rng, sgn)
            if t not in SIGNED_TYPES:
                p = np.abs(p) * sgn                                   # the range: min 0, max amax -- or min -amax, max 0
            add(f"ovf_{NAME[t]}_{tag}", p * amax)
    v = z.copy(); v[:3] = (1e-39, 5e-40, -3e-40)
    add("sub_issue", v)
    add("sub_mixed", _pattern(rng) * 1e-40)
    add("sub_neg_max", _pattern(rng, -1.0) * 3e-39)
    add("sub_pos_only", np.abs(_pattern(rng)) * 1e-39)
    v = z.copy(); v[5], v[9] = 1.4e-45, -1.4e-45
    add("sub_smallest", v)                                            # max / -8 rounds to zero: d == 0, not the overflow class
    add("normal_tiny", _pattern(rng) * 3e-38)
    # huge finite values: max - min overflows (Q4_1 / Q5_1), sum_x2 overflows (Q4_K)
    v = rng.standard_normal(32); v[3], v[20] = 3e38, -3e38
    add("huge_pm", v)
    v = rng.standard_normal(32); v[3] = 3e38
    add("huge_pos", v)
    v = np.where(k % 3 == 0, 3e38, np.where(k % 3 == 1, -3e38, 0.0))
    add("huge_all", v)
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    return out


def special_rows():
    """(names, float32[n, 32]): one block per row"""
    sb = special_blocks()
    return [n for n, _ in sb], np.stack([v for _, v in sb])


Q4K_PATH3_POSITIONS = (0, 3, 4, 7)            # both halves of the 12-byte scale packing (codes 0..3 whole bytes, 4..7 split)


@functools.lru_cache(None)
def q4k_super_blocks():
    """[(name, float32[256])]"""
    rng = np.random.default_rng(20241)
    out = []
    sb = special_blocks()
    for i, (name, v) in enumerate(sb):
        x = rng.standard_normal(256).astype(F)
        x[32 * (i % 8): 32 * (i % 8) + 32] = v
        out.append((f"{name}@{i % 8}", x))
    for i in range(0, len(sb) - 7, 8):
        out.append((f"pack_{sb[i][0]}", np.concatenate([v for _, v in sb[i: i + 8]])))
    # a sub-block whose range is 1e-3 of its neighbours', not constant: its 6-bit code rounds to 0, the quants of its own search stay
    for pos in Q4K_PATH3_POSITIONS:
        x = rng.standard_normal(256).astype(F)
        x[32 * pos: 32 * pos + 32] = (rng.standard_normal(32) * 1e-3).astype(F)
        out.append((f"tiny_range_at_{pos}", x))
    x = rng.standard_normal(256).astype(F)
    x[32 * 2: 32 * 3] = (rng.standard_normal(32) * 10.0 - 40.0).astype(F)
    out.append(("code63_scale_and_min", x))                           # one sub-block holds the largest scale and the largest minimum
    out.append(("all_pos_gauss", (np.abs(rng.standard_normal(256)) + 0.5).astype(F)))
    # positive multiples c_j * l, l in 1 .. 15: the first grid fits exactly (error 0, nothing beats it), min stays 0: max_min == 0, inv_min == 0
    x = np.concatenate([2.0 ** -j * rng.integers(1, 16, 32) for j in range(8)]).astype(F)
    x[::32] = 15.0 * 2.0 ** -np.arange(8)
    out.append(("all_pos_grid", x))
    out.append(("eight_const", np.repeat(np.array([0.37, -0.37, 0.0, 5.0, -1e-3, 1e-3, -7.0, 2.0], F), 32)))
    names = [n for n, _ in out]
    assert len(set(names)) == len(names)
    return out


def special_case(t):
    """(names, float32[rows, K]) of the special blocks for type t: K = 32, or 256 for Q4_K"""
    if t == O.Q4_K:
        sb = q4k_super_blocks()
        return [n for n, _ in sb], np.stack([v for _, v in sb])
    return special_rows()


# ---- launch geometries ---------------------------------------------------------------------------------------------------------
BLOCK_COUNTS = {**{t: (1, 255, 256, 257, 513) for t in B32_TYPES}, O.Q4_K: (1, 7, 31, 32, 33, 65), O.F16: (1, 255, 256, 257)}
PER_WORKGROUP = {**{t: 256 for t in B32_TYPES}, O.Q4_K: 32, O.F16: 256}
LAYOUTS = ("row", "rows")
KEY_BLOCKS = ("zero", "clamp_neg_max", "sub_issue", "tie_np_cross", "grid_q4_0_d1", "huge_pm", "ovf_q8_0_below", "ovf_q4_1_below", "one_neg_at_31", "d_edge_q4_0_12", "m_inf_d_finite")
KEY_SUPER_BLOCKS = ("tiny_range_at_4", "code63_scale_and_min", "eight_const", "all_pos_grid", "tiny_range_at_0", "pack_zero", "sub_issue", "huge_pm", "tiny_range_at_7")


def laid_positions(t, nb):
    """the blocks that carry a special block: the first three, the last three and three on either side of every workgroup boundary"""
    per = PER_WORKGROUP[t]
    pos = set(range(3)) | set(range(nb - 3, nb))
    for edge in range(per, nb + 1, per):
        pos |= set(range(edge - 3, edge + 3))
    return sorted(p for p in pos if 0 <= p < nb)


def geometry(t, nb, layout, scale):
    """(float32[rows, K], {block index: name of the special block laid there})"""
    assert t != O.F16 and nb in BLOCK_COUNTS[t] and layout in LAYOUTS
    bs = O.BLCK[t]
    rng = np.random.default_rng([20242, t, nb, int(round(np.log10(scale) * 10)) + 100])
    x = (rng.standard_normal((nb, bs)) * scale).astype(F)
    pool = dict(q4k_super_blocks() if t == O.Q4_K else special_blocks())
    keys = KEY_SUPER_BLOCKS if t == O.Q4_K else KEY_BLOCKS
    keys = [next(n for n in pool if n == k or n.startswith(k + "@")) for k in keys]      # a special block inside a super-block is named block@position
    laid = {}
    for p in laid_positions(t, nb):
        laid[p] = keys[(p + nb) % len(keys)]
        x[p] = pool[laid[p]]
    return (x.reshape(1, nb * bs) if layout == "row" else x), laid


def geometry_ids(t):
    return [(nb, layout) for nb in BLOCK_COUNTS[t] for layout in LAYOUTS]


ROUND_TRIP_BLOCKS = ("zero", "clamp_neg_max", "sub_issue", "tie_np_cross", "grid_q4_0_d1", "one_neg_at_31", "const_neg", "ovf_q8_0_below", "all_pos_offset")


def round_trip_case(t):
    """float32[3, K]: the rows that are quantized and dequantized again on the device -- Gaussian with special blocks whose stored scales are finite, so that no
    dequantized word is a NaN (a NaN's sign and payload are the processor's, not the format's)"""
    rng = np.random.default_rng([20244, t])
    if t == O.F16:
        return (rng.standard_normal((3, 85)) * 3.0).astype(F)
    pool = dict(special_blocks())
    x = rng.standard_normal((33, 32)).astype(F)
    for i, k in enumerate(ROUND_TRIP_BLOCKS):
        x[(7 * i + 2) % 33] = pool[k]
    return x.reshape(3, -1) if t != O.Q4_K else np.concatenate([x, rng.standard_normal((15, 32)).astype(F)]).reshape(3, 512)


def dequantize_expected(t, raw, n):
    """the floats the bytes `raw` decode to: the oracle's dequantize_row (F16: the exact widening, in numpy)"""
    return np.ascontiguousarray(raw).view(np.float16).astype(F) if t == O.F16 else O.dequantize(t, raw, n)


# ---- F16 --------------------------------------------------------------------------------------------------------------------------
def f16_cases():
    """{name: float32[n]}.  `nan` holds every NaN (all 2046 half NaNs as floats, quiet and signalling float NaNs of both signs); no other case holds one"""
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    hv = h.view(np.float16).astype(F)                                 # exact: every half is a float
    nan = np.isnan(hv)
    out = {"all_halves": hv[~nan]}
    lo = np.arange(0x7bff, dtype=np.uint16)                           # adjacent finite halves lo, lo + 1 of the positive side
    mid = ((lo.view(np.float16).astype(np.float64) + (lo + 1).astype(np.uint16).view(np.float16).astype(np.float64)) / 2).astype(F)
    assert np.array_equal(mid.astype(np.float64) * 2, lo.view(np.float16).astype(np.float64) + (lo + 1).astype(np.uint16).view(np.float16).astype(np.float64))   # exact in fp32
    tri = np.stack([np.nextafter(mid, F(0)), mid, np.nextafter(mid, F(np.inf))], axis=1).reshape(-1)
    out["midpoints"] = np.concatenate([tri, -tri])
    e = [65504.0, 65519.996, 65520.0, 3.4028234663852886e38, np.inf, 0.0, 1.401298464324817e-45, 2.0 ** -25]
    e = np.array(e, F)
    e = np.concatenate([e, [np.nextafter(F(2.0 ** -25), F(0)), np.nextafter(F(2.0 ** -25), F(1))]]).astype(F)
    out["extremes"] = np.concatenate([e, -e])
    fn = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff, 0x7fa00000, 0xffa00000, 0x7f801000, 0xff801000, 0x7fc00001, 0xff8fffff], np.uint32).view(F)
    out["nan"] = np.concatenate([hv[nan], fn])
    assert np.isnan(out["nan"]).all() and not any(np.isnan(v).any() for k, v in out.items() if k != "nan")
    pool = np.concatenate([out["all_halves"], out["midpoints"], out["extremes"]])
    rng = np.random.default_rng(20243)
    for n in BLOCK_COUNTS[O.F16]:
        x = rng.choice(pool, n).astype(F)
        x[0], x[-1] = F(65520.0), F(-65519.996)
        out[f"n_{n}"] = x
    return out


# ---- reading Q4_K blocks back (coverage assertions) ---------------------------------------------------------------------------------
def q4k_fields(raw):
    """raw bytes of Q4_K blocks -> (d, dmin as float32 [n], codes sc [n, 8], codes m [n, 8], nibbles [n, 8, 32]); get_scale_min_k4 and the qs layout restated in numpy"""
    b = np.ascontiguousarray(raw, np.uint8).reshape(-1, 144)
    d = b[:, 0:2].copy().view(np.float16).astype(F)[:, 0]
    dmin = b[:, 2:4].copy().view(np.float16).astype(F)[:, 0]
    s = b[:, 4:16].astype(np.int32)
    sc = np.concatenate([s[:, 0:4] & 63, (s[:, 8:12] & 0xF) | ((s[:, 0:4] >> 6) << 4)], axis=1)
    m = np.concatenate([s[:, 4:8] & 63, (s[:, 8:12] >> 4) | ((s[:, 4:8] >> 6) << 4)], axis=1)
    qs = b[:, 16:].reshape(-1, 4, 32)
    nib = np.stack([qs & 0xF, qs >> 4], axis=2).reshape(-1, 8, 32)
    return d, dmin, sc, m, nib
