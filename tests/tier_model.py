"""A plain-numpy error model of the tolerance-tier product kernels (no GPU, no package import).

The exact path is pinned word for word to the reference CPU build.  Three product kernels are NOT, by construction -- they do not share the
reference's fp32 summation order: k_mmq (mmq.hip, prefill mode 0), k_mmd (dense_f16.hip, CLLM_PREFILL=f16) and the free-order decode mat-vec
(gemv_free32.hip).  This module says, per OUTPUT ELEMENT, how far such a kernel may be from the float64 value of what it computes.

1. Decoders (float64 / integers, exact): decode_q4_0 / _q4_1 / _q8_0 / _q4_K for weight rows, decode_q8_0 / _q8_1 / _q8_K for activation rows, taking
   the raw block bytes (tests/synth_helpers.rand_blocks, oracle.quantize_q8_*).  dequant64 is the float64 value of dequantize_row_*.

2. terms(wtype, w_row_bytes, act_row_bytes): the float64 terms T_i one output element sums --
     Q4_0 / Q8_0 : per 32-block b               d_w[b] d_x[b] s_b                          s_b = sum_j q_w[b][j] q_x[b][j], an exact integer
     Q4_1        : the same with nibbles 0..15, then per 32-block  m_w[b] s_x[b]           (the Q8_1 block's s = fp16(d_x sum q_x); mmq.hip:16-17, 268-279)
     Q4_K        : per 32-sub-block  d_w d_x sc[b] s_b,  then per 32-sub-block  -dmin_w d_x mn[b] bsum_x[b]   (bsum over the sub-block's 32 quants)
   R = sum T_i, S = sum |T_i|, n_t = len(T).

3. The fast-mode / free-order bound:     |got - R| <= (n_t + 8) 2^-24 S        (fast_bound)
   Derivation.  u = 2^-24 is the unit roundoff of fp32.
     * Every term is FORMED with at most three fp32 roundings: int -> float of the integer sum (exact below 2^24; Q4_K's super-block sum
       sum_b sc[b] s_b reaches 2^25 and rounds once), the scale product d_w d_x, and the multiply.  [Q4_K: k_mmq converts the exact integer sum of the eight
       sub-blocks and multiplies once: its error u |sum_b sc[b] s_b| <= u sum_b |sc[b] s_b| is covered by the finer per-sub-block S.]  So each computed term is
       T_i (1 + e_i), |e_i| <= 3u + O(u^2).  Where the last multiply is fused with the add (fmaf), one of the three does not happen.
     * A sum of n_t fp32 numbers in ANY order (any tree, any number of partial accumulators) has an error of at most (n_t - 1) u sum |terms| to first order.
     * Together: (n_t - 1 + 3) u S = (n_t + 2) u S to first order.  The remaining + 6 u S absorbs the second-order terms ((n_t + 2)^2 u^2 S <= 6 u S for
       n_t <= 10000) and the one extra rounding an epilogue adds to the finished sum.
     * Extra addends that the kernel adds to the finished sum in fp32 (a residual, a bias): each is one more term (n_t + 1) with |addend| in S
       (fast_bound(..., extra=...)).
   The reference's own AVX2 order adds the eight int32 lanes of a block SEPARATELY (each lane: fmaf(d_w d_x, float(lane sum), acc[lane])), i.e. its
   terms are the eight lane parts of T_b.  Their absolute sum can exceed |T_b| when the lane parts cancel, so the reference is judged with the SAME formula over
   its own, finer terms (lane_terms): n_t = 8 per block.  The kernels are judged over block terms, the tighter of the two; both uses are stated in the tests.

4. The f16 bound (f16_bound).  dense_f16.hip forms every weight in fp16 while staging (commit(), dense_f16.hip:105-153), mirrored here in numpy (np.float16
   arithmetic is correctly rounded per operation; where the kernel uses ONE fused fp16 fma the mirror forms the exact float64 value and rounds it once):
     Q4_0 : (nib - 8) exact [:145-146: (1024 + nib) - 1032], times d: one fp16 multiply                        w16 = f16((nib - 8) d)
     Q8_0 : q exact [:131-132: (1024 + (q ^ 0x80)) - 1152], times d: one fp16 multiply                          w16 = f16(q d)
     Q4_1 : one fp16 fma [:142-143]                                                                           w16 = f16(nib d + m)
     Q4_K : d1 = f16(d sc), m1 = f16(-(dmin mn)) [:115-117: the fp32 products are exact, 11 x 6 bits], one fp16 fma [:123]     w16 = f16(nib d1 + m1)
   the activations are rounded to fp16 (k_f32_to_f16, :215-221).  R = sum_k w16_k x16_k in float64.  The products are exact in fp32 (11 x 11 bits), so the only
   error is the fp32 accumulation over K terms:  |got - R| <= 2 K 2^-24 sum_k |w16_k x16_k|; the factor 2 allows for the matrix core's internal
   accumulation of the 16 products of one instruction not being one correctly rounded fp32 add per step.  The mirror is exact, so no 2^-11 term is needed.
"""
import numpy as np

Q4_0, Q4_1, Q8_0, Q4_K = 2, 3, 8, 12
U32 = 2.0 ** -24
W_BLOCK_BYTES = {Q4_0: 18, Q4_1: 20, Q8_0: 34, Q4_K: 144}


def _blocks(b, nbytes):
    b = np.ascontiguousarray(b, np.uint8)
    lead = b.shape[:-1]
    assert b.shape[-1] % nbytes == 0, "row bytes are not whole blocks"
    return b.reshape(lead + (b.shape[-1] // nbytes, nbytes))


def _f16(bb):
    """two bytes per entry -> the fp16 value as float64"""
    return np.ascontiguousarray(bb).view(np.float16)[..., 0].astype(np.float64)


def _nibbles(qs):
    """qs[..., 16] bytes -> [..., 32]: elements 0..15 the low nibbles, 16..31 the high ones (block_q4_0 / block_q4_1)"""
    return np.concatenate([qs & 15, qs >> 4], axis=-1).astype(np.int64)


# ---- weight rows ------------------------------------------------------------------------------------------------
def decode_q4_0(b):
    """-> d [..., nb], q [..., nb, 32] (nib - 8)"""
    bl = _blocks(b, 18)
    return {"d": _f16(bl[..., 0:2]), "q": _nibbles(bl[..., 2:18]) - 8}


def decode_q4_1(b):
    """-> d, m [..., nb], q [..., nb, 32] (nibbles 0..15); w = q d + m"""
    bl = _blocks(b, 20)
    return {"d": _f16(bl[..., 0:2]), "m": _f16(bl[..., 2:4]), "q": _nibbles(bl[..., 4:20])}


def decode_q8_0(b):
    """-> d [..., nb], q [..., nb, 32] int8 (weights and Q8_0 activations share the format)"""
    bl = _blocks(b, 34)
    return {"d": _f16(bl[..., 0:2]), "q": bl[..., 2:34].view(np.int8).astype(np.int64)}


def decode_q4_K(b):
    """-> d, dmin [..., nsb], sc, mn [..., nsb, 8] (the 6-bit sub-scales / mins, get_scale_min_k4), q [..., nsb, 8, 32] (nibbles 0..15);
    w = d sc q - dmin mn.  64 elements share 32 bytes: sub-block 2j the low nibbles, 2j + 1 the high ones"""
    bl = _blocks(b, 144)
    s = bl[..., 4:16].astype(np.int64)
    sc = np.concatenate([s[..., 0:4] & 63, (s[..., 8:12] & 15) | ((s[..., 0:4] >> 6) << 4)], axis=-1)
    mn = np.concatenate([s[..., 4:8] & 63, (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)], axis=-1)
    qs = bl[..., 16:144].reshape(bl.shape[:-1] + (4, 32))
    q = np.stack([qs & 15, qs >> 4], axis=-2).reshape(bl.shape[:-1] + (8, 32)).astype(np.int64)
    return {"d": _f16(bl[..., 0:2]), "dmin": _f16(bl[..., 2:4]), "sc": sc, "mn": mn, "q": q}


# ---- activation rows --------------------------------------------------------------------------------------------
def decode_q8_1(b):
    """-> d, s [..., nb] (s = fp16(d sum q)), q [..., nb, 32]"""
    bl = _blocks(b, 36)
    return {"d": _f16(bl[..., 0:2]), "s": _f16(bl[..., 2:4]), "q": bl[..., 4:36].view(np.int8).astype(np.int64)}


def decode_q8_K(b):
    """-> d [..., nsb] (fp32), q [..., nsb, 256], bsums [..., nsb, 16] (int16 sums of 16 quants)"""
    bl = _blocks(b, 292)
    d = np.ascontiguousarray(bl[..., 0:4]).view(np.float32)[..., 0].astype(np.float64)
    bs = np.ascontiguousarray(bl[..., 260:292]).view(np.int16).astype(np.int64)
    return {"d": d, "q": bl[..., 4:260].view(np.int8).astype(np.int64), "bsums": bs}


W_DECODE = {Q4_0: decode_q4_0, Q4_1: decode_q4_1, Q8_0: decode_q8_0, Q4_K: decode_q4_K}
ACT_DECODE = {Q4_0: decode_q8_0, Q4_1: decode_q8_1, Q8_0: decode_q8_0, Q4_K: decode_q8_K}


def dequant64(wtype, b):
    """the float64 value of dequantize_row_* for rows of block bytes: [..., K].  Each is ONE rounding away from the reference's fp32 result at the most:
    (nib - 8) d, q d: exact products; nib d + m and (d sc) nib - (dmin mn): d sc and dmin mn are exact in fp32 (11 x 6 bits), so is their product with a nibble
    (21 bits) -- the fp32 code rounds once, at the final add / subtract, and float32(this value) is that same rounding"""
    w = W_DECODE[wtype](b)
    if wtype == Q4_1:
        v = w["q"] * w["d"][..., None] + w["m"][..., None]
    elif wtype == Q4_K:
        v = (w["d"][..., None] * w["sc"])[..., None] * w["q"] - (w["dmin"][..., None] * w["mn"])[..., None]
        return v.reshape(v.shape[:-3] + (-1,))
    else:
        v = w["q"] * w["d"][..., None]
    return v.reshape(v.shape[:-2] + (-1,))


def block_isums(wtype, w_rows, act_rows):
    """the exact integer block dot products s[m, n, b] over 32-element (sub-)blocks, for weight rows [N, bytes] and activation rows [M, bytes]"""
    w, a = W_DECODE[wtype](w_rows), ACT_DECODE[wtype](act_rows)
    qw = w["q"].reshape(w["q"].shape[0], -1, 32).astype(np.float64)             # [N, nb32, 32]
    qa = a["q"].reshape(a["q"].shape[0], -1, 32).astype(np.float64)             # [M, nb32, 32]
    s = np.matmul(qa.transpose(1, 0, 2), qw.transpose(1, 2, 0))                 # [nb32, M, N]: integers below 2^53, exact in float64
    return s.transpose(1, 2, 0)


def terms_matrix(wtype, w_rows, act_rows, lanes=False):
    """T[m, n, i]: the terms of every output element of act_rows [M, bytes] x w_rows [N, bytes].  Order: the scale terms of the blocks in K order, then (Q4_1, Q4_K)
    the min terms of the blocks in K order.  lanes=True: every scale term split into the eight int32 lanes of the reference's AVX2 dot products
    (elements 4l .. 4l + 3 of the 32-block; Q4_K: the same split of each sub-block), the order the reference's fp32 accumulators see"""
    w, a = W_DECODE[wtype](w_rows), ACT_DECODE[wtype](act_rows)
    if lanes:
        qw = w["q"].reshape(w["q"].shape[0], -1, 4).astype(np.float64)
        qa = a["q"].reshape(a["q"].shape[0], -1, 4).astype(np.float64)
        s = np.matmul(qa.transpose(1, 0, 2), qw.transpose(1, 2, 0)).transpose(1, 2, 0)      # [M, N, nb32 * 8]
        rep = 8
    else:
        s = block_isums(wtype, w_rows, act_rows)
        rep = 1
    if wtype == Q4_K:
        dw = np.repeat((w["d"][..., None] * w["sc"]).reshape(w["d"].shape[0], -1), rep, axis=-1)            # [N, nb32 (* 8)]: d sc
        dx = np.repeat(a["d"], 8 * rep, axis=-1)                                                               # [M, nb32 (* 8)]
        t = s * dw[None, :, :] * dx[:, None, :]
        bs = a["bsums"].reshape(a["bsums"].shape[0], -1, 2).sum(-1).astype(np.float64)                         # [M, nb32]: the sub-block's 32 quants
        mw = (w["dmin"][..., None] * w["mn"]).reshape(w["d"].shape[0], -1)                                     # [N, nb32]
        tm = -(mw[None, :, :] * (np.repeat(a["d"], 8, axis=-1) * bs)[:, None, :])
        return np.concatenate([t, tm], axis=-1)
    t = s * np.repeat(w["d"], rep, axis=-1)[None, :, :] * np.repeat(a["d"], rep, axis=-1)[:, None, :]
    if wtype == Q4_1:
        return np.concatenate([t, w["m"][None, :, :] * a["s"][:, None, :]], axis=-1)
    return t


def terms(wtype, w_row_bytes, act_row_bytes):
    """the float64 terms T_i of ONE output element (one weight row, one activation row)"""
    return terms_matrix(wtype, np.asarray(w_row_bytes)[None], np.asarray(act_row_bytes)[None])[0, 0]


def n_blocks32(wtype, T):
    """how many of the terms along the last axis are scale terms (= 32-element blocks of K)"""
    return T.shape[-1] // 2 if wtype in (Q4_1, Q4_K) else T.shape[-1]


def fast_bound(T, extra=None):
    """-> R, bound for the fast-mode / free-order tier: (n_t + 8) 2^-24 S over the last axis of T; extra: a list of fp32 addends (broadcastable to R) the
    kernel adds to the finished sum -- each is one more term"""
    R, S, n_t = T.sum(-1), np.abs(T).sum(-1), T.shape[-1]
    for e in (extra or []):
        e = np.asarray(e, np.float64)
        R, S, n_t = R + e, S + np.abs(e), n_t + 1
    return R, (n_t + 8) * U32 * S


# ---- the f16 mode ------------------------------------------------------------------------------------------------
def f16_weights(wtype, b):
    """dense_f16.hip's fp16 weights for rows of block bytes: [..., K] float64 values, each exactly an fp16 number (the steps: the module docstring, item 4)"""
    w = W_DECODE[wtype](b)
    h = lambda v: np.asarray(v, np.float64).astype(np.float16).astype(np.float64)     # ONE correct rounding of an exactly represented float64 value
    if wtype in (Q4_0, Q8_0):
        v = h(w["q"] * w["d"][..., None])
    elif wtype == Q4_1:
        v = h(w["q"] * w["d"][..., None] + w["m"][..., None])
    else:
        d1, m1 = h(w["d"][..., None] * w["sc"]), h(-(w["dmin"][..., None] * w["mn"]))
        v = h(d1[..., None] * w["q"] + m1[..., None])
        return v.reshape(v.shape[:-3] + (-1,))
    return v.reshape(v.shape[:-2] + (-1,))


def f16_bound(wtype, w_rows, x):
    """-> R [M, N], bound [M, N] for D = f16(W) . f16(x)^T, x [M, K] float32: 2 K 2^-24 sum_k |w16 x16|"""
    w16 = f16_weights(wtype, w_rows)
    x16 = np.asarray(x, np.float32).astype(np.float16).astype(np.float64)
    K = x16.shape[-1]
    return x16 @ w16.T, 2 * K * U32 * (np.abs(x16) @ np.abs(w16).T)


# ---- the cases the CPU model tests and the GPU tests share ---------------------------------------------------------
Q32_TYPES = (Q4_0, Q4_1, Q8_0)
# (wtype, K, N, M, ne02, ne12): the plain product in fast mode
FAST_CASES = [(t, K, N, M, 1, 1) for t in Q32_TYPES for K, N, M in [(32, 3, 64), (96, 10, 33), (288, 129, 65), (4128, 130, 129), (768, 1, 33), (4352, 127, 257)]] + \
             [(Q4_K, K, N, M, 1, 1) for K, N, M in [(256, 3, 64), (768, 129, 65), (4352, 130, 129), (2048, 1, 33)]] + \
             [(t, K, N, M, a, b) for t in Q32_TYPES + (Q4_K,) for K, N, M, a, b in [(512, 19, 40, 2, 4), (256, 12, 33, 1, 3)]]
# the fused forms of cllm_op_mul_mat_ex in fast mode: one K % 256 != 0 shape per 32-block type, one Q4_K shape; M >= 33, N even, N / 2 not a multiple of 8
# (SiLU's polynomial body AND its libm tail, except N = 10: the tail only)
FUSED_CASES = [(Q4_0, 288, 130, 65), (Q4_1, 96, 10, 33), (Q8_0, 800, 66, 40), (Q4_K, 768, 130, 65)]
# the f16 mode, at both tiles
F16_CASES = [(t, K, N, M) for t in Q32_TYPES for K, N, M in [(96, 10, 33), (288, 129, 65), (4128, 130, 129)]] + \
            [(Q4_K, K, N, M) for K, N, M in [(768, 129, 65), (4352, 130, 129)]]
# the free-order decode tier: one column
FREE_CASES = [(t, K, N) for t in Q32_TYPES for K, N in [(32, 2), (544, 8), (2848, 24), (4096, 130), (11008, 256)]]


QUIET_FAST, QUIET_F16 = 2.0 ** -12, 2.0 ** -7


def case_inputs(wtype, K, N, M, ne02=1, ne12=1, quiet=QUIET_FAST):
    """seeded inputs of a case: weight block bytes [ne02 * N, row bytes] (rand_blocks) and activations [ne12, M, K] float32.  With more than one token the LAST one
    (a ragged tile row at every shape here) is a quiet one, `quiet` times the others: its outputs are far below max |ref| of the matrix, where a max-norm
    check sees nothing (the f16 cases take 2^-7, which keeps nearly all of its fp16 activations normal numbers)"""
    from synth_helpers import rand_blocks
    r = np.random.default_rng([wtype, K, N, M, ne02, ne12])
    w = rand_blocks(wtype, N * ne02, K, r)
    x = r.standard_normal((ne12, M, K)).astype(np.float32)
    if M > 1:
        x[:, M - 1, :] *= np.float32(quiet)
    return w, x


def act_rows(O, wtype, x):
    """the reference's activation quantization of the rows of x [M, K] (oracle.quantize_q8_*): [M, row bytes]"""
    q = O.quantize_q8_K if wtype == Q4_K else O.quantize_q8_1 if wtype == Q4_1 else O.quantize_q8_0
    return np.stack([q(r) for r in np.asarray(x, np.float32).reshape(-1, x.shape[-1])])
