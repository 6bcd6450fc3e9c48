"""A plain-numpy model of the flash attention kernels (fattn.hip: k_fattn, k_fattn_merge): no GPU, no package import.

It says, per OUTPUT ELEMENT, how far the kernel may be from the float64 value of what it computes, and it restates the kernel's algorithm step by step so
that the CPU suite can show (a) that the inputs below drive the paths they claim to and (b) that the bound separates a right kernel from a wrong one.

1. Operand mirror (q_operand, kv_operand): the float64 values of exactly what the matrix cores multiply.
     F16 cache : q rounded to fp16 (fattn.hip:123); k, v as stored.
     Q8_0 cache: k, v entries fp16(fp32(d) q) (fa_q8_8 / q8_cvt: d has 11 bits, q 8: the fp32 product is exact, the fp16 conversion rounds once);
                 Q per 32-block  fp16(dq rint(x id)),  d = amax / 127, id = 127 / amax (0 for a zero block), dq = fp16(d), in float32 (fattn.hip:108-123).

2. Reference (reference): over those operands, in float64, with x_i = scale k_i.q + mask_i (natural units) and P = softmax over the visible keys,
     R[n, h, :] = sum_i P_i v_i          A[n, h, :] = sum_i P_i |v_i|
   and the scores in the kernel's base-2 units.  A row with nothing visible gives R = A = 0.

3. The bound (reference()["bound"]).  u = 2^-24 (fp32), EXP = 2^-23 (v_exp_f32: 1 ulp).  The kernel computes, per visible key,
     e_i = fma(t_i, sc2, -m),  t_i = s_i + f_i mask_mul,  p_i = exp2(e_i),   l = sum p_i (fp32),   O = sum fp16(p_i) v_i (fp32),   out = O / l
   with s_i the fp32 MFMA sum of the D exact products k_d q_d, sc2 = fl(scale LOG2E), mask_mul = fl(LOG2E / sc2), m the lazy exponent reference.
   m itself carries NO error: whatever value it has, l and O are built against the same m, and a rescale multiplies both by the same alpha, so O / l does
   not depend on it in exact arithmetic.  What remains:
     (a) fp16(p) in O against the unrounded p in l (fattn.hip:349).  p <= 2^FA_TAU, so fp16 never overflows; for p >= 2^-14 the rounding is 2^-11 p, below
         that fp16 is subnormal: at most 2^-25 absolute.  Relative to l:            2^-11 A  +  n_vis 2^-25 max_i |v_i|        (l >= 1, see (e))
         With splits, the n_s keys of split s enter through its merge weight 2^(m_s - M) <= min(1, 2^(xmax_s - xmax + FA_TAU)) (m_s is at most the split's
         maximum, M at least the overall maximum less FA_TAU):                      sum_s min(1, 2^(xmax_s - xmax + FA_TAU)) n_s 2^-25 max_{i in s} |v_i|
     (b) the error delta_i of the exponent argument (base-2 units), which makes p_i wrong by ln2 delta_i + EXP relatively.  An error eps of every p moves the
         numerator by eps A and the denominator by eps l:                           2 eps_row A,   eps_row = ln2 max_i delta_i + EXP
         delta_i <= 2 D u sc2 sum_d |k_d q_d|      fp32 MFMA accumulation of D exact products (the convention of tier_model.py section 4)
                  + 5 u G_i,   G_i = sc2 |s_i| + log2e |f_i| + max_j |x_j|:  the roundings that touch the argument, each relative to a part of G_i --
                    sc2 (the float LOG2E and the product: 2, on the score part); mask_mul (the float LOG2E, the division, f mask_mul: 3, on the mask part;
                    sc2's own error cancels between mask_mul and the fma); the add s + f mask_mul (1); the fma's result (1, |e_i| <= |x_i| + |m| and |m| is a
                    computed tile maximum).  At most 4 touch any one part; the fifth absorbs the second-order terms.
     (c) fp32 accumulation.  A workgroup walks n_in <= chunk visible keys: O through MFMAs (2 n_in u A by the same convention), l per lane (n_in / 2 + 1
         adds), every rescale one more rounding of O and of l (at most one per tile), the epilogue's 1 / l and product, in all
                                                                                    (2.5 n_in + 2 tiles_per_chunk + 5) u A
     (d) the merge (splits > 1): weights exp2(m_s - M) are NOT common factors (2 EXP A); w l and w O one rounding each, L a tree of depth 8 over 256 entries,
         O in G = 1024 / D interleaved partial sums of ceil(splits / G) terms plus G - 1 adds:
                                                                                    (ceil(splits / G) + G + 10) u A + 2 EXP A
     (e) l >= 1: m never exceeds the running maximum, and the key that set it has p = 1; in the merge the split holding M has weight 1.
   bound = A (2^-11 + 2 eps_row + [(c)] + [(d)]) + [(a)'s absolute part].  Nothing here is fitted to GPU output.  At ordinary score magnitudes (Gaussian q, k: a
   few nats) 2^-11 A is the largest term; the steered profiles below pay 2 eps_row for their 20 .. 30 base-2 units of score.

4. emulate(): the kernel's loop in numpy -- 64-position tiles, the FA_TAU lazy rescale, fp32 l, fp16 P, fp32 O, chunk / splits as launch_fattn computes them
   (launch_plan), the merge -- with named mutations, returning the number of non-trivial rescales per row.  A tile in which a row sees nothing is a no-op for
   that row (every p = exp2(-inf) = 0), which is all the kernel's block-uniform tile skip amounts to.

5. Score profiles (profile()) and the case list the CPU model tests and the GPU tests share (CASES).
"""
import functools

import numpy as np

F16, Q8_0 = 1, 8
U32, U16, EXP_ULP = 2.0 ** -24, 2.0 ** -11, 2.0 ** -23
FA_TAU, FA_MAX_SPLITS, FA_DIV = 8.0, 256, 64
LOG2E = 1.4426950408889634
LOG2E32 = np.float32(LOG2E)
MUTATIONS = ("no_l_rescale", "no_o_rescale", "lim_plus", "lim_minus", "drop_last_ragged", "leak_hidden", "merge_w1", "merge_l_unweighted",
             "mask_row_next", "kv_head_next", "k_batch0")
# the single-token form above the long-context threshold (launch_attn_long_flash; tests/attn_long_model.py): the number of positions is read on the device
# (fattn_args::n_kv_dev) and whole splits lie past it.  ignore_n_kv_dev: the kernel walks all the rows it was given; empty_split_weight_1: a split that saw no
# key enters the merge with weight 1 and l = 1 instead of (m = -inf, l = 0)
LONG_MUTATIONS = ("ignore_n_kv_dev", "empty_split_weight_1")


def launch_plan(N, H, Hkv, n_kv, scratch=True, div=FA_DIV):
    """-> decode, chunk, splits as launch_fattn (fattn.hip:493-507) computes them; scratch=False: a caller without split-KV scratch (cllm_op_attn_prefill)"""
    decode = N * (H // Hkv) <= 32
    tiles = (n_kv + 63) // 64
    chunk, splits = tiles * 64, 1
    if decode and n_kv > 64:
        per = max(tiles // div, 1, (tiles + FA_MAX_SPLITS - 1) // FA_MAX_SPLITS)
        chunk, splits = per * 64, (tiles + per - 1) // per
        if splits > 1 and not scratch:
            chunk, splits = tiles * 64, 1
    return decode, chunk, splits


# ---- operands ------------------------------------------------------------------------------------------------------------
def q8_0_quantize(x):
    """quantize_row_q8_0 over the last axis: float32 [..., K] -> block bytes [..., K / 32 * 34]"""
    x = np.ascontiguousarray(x, np.float32)
    xb = x.reshape(x.shape[:-1] + (-1, 32))
    amax = np.max(np.abs(xb), axis=-1)
    d = amax / np.float32(127.0)
    with np.errstate(divide="ignore"):
        idv = np.where(amax != 0, np.float32(127.0) / amax, np.float32(0.0)).astype(np.float32)
    out = np.zeros(xb.shape[:-1] + (34,), np.uint8)
    out[..., 0:2] = np.ascontiguousarray(d.astype(np.float16)[..., None]).view(np.uint8)
    out[..., 2:34] = np.rint(xb * idv[..., None]).astype(np.int8).view(np.uint8)
    return out.reshape(x.shape[:-1] + (-1,))


def kv_operand(kv_t, a):
    """the K / V values the kernel multiplies, float64 [..., D]: a is float16 [..., D] (F16) or Q8_0 block bytes [..., D / 32 * 34]"""
    if kv_t == F16:
        return np.asarray(a, np.float16).astype(np.float64)
    a = np.ascontiguousarray(a, np.uint8)
    bl = a.reshape(a.shape[:-1] + (-1, 34))
    d = np.ascontiguousarray(bl[..., 0:2]).view(np.float16)[..., 0].astype(np.float32)
    q = bl[..., 2:34].view(np.int8).astype(np.float32)
    v = (d[..., None] * q).astype(np.float16).astype(np.float64)
    return v.reshape(a.shape[:-1] + (-1,))


def q_operand(kv_t, q):
    """the Q values the kernel multiplies, float64, from float32 q [..., D]"""
    q = np.asarray(q, np.float32)
    if kv_t == F16:
        return q.astype(np.float16).astype(np.float64)
    xb = q.reshape(q.shape[:-1] + (-1, 32))
    amax = np.max(np.abs(xb), axis=-1)
    d = amax / np.float32(127.0)
    with np.errstate(divide="ignore"):
        idv = np.where(amax != 0, np.float32(127.0) / amax, np.float32(0.0)).astype(np.float32)
    dq = d.astype(np.float16).astype(np.float32)
    x = dq[..., None] * np.rint(xb * idv[..., None])
    return x.astype(np.float16).astype(np.float64).reshape(q.shape)


# ---- visibility ----------------------------------------------------------------------------------------------------------
def mask_of_head(mask, h):
    """mask None | [N, n_kv] | [H, N, n_kv] (the ne[2] == H form, read as h % ne2) -> the [N, n_kv] rows of head h, float32"""
    if mask is None:
        return None
    m = np.asarray(mask)
    return (m[h % m.shape[0]] if m.ndim == 3 else m).astype(np.float32)


def additive(mask, h, N, n_kv, causal_past):
    """[N, n_kv] float64: the additive term of every (query, key), -inf where hidden (mask tensor, or the in-kernel causal rule kv <= causal_past + n)"""
    m = mask_of_head(mask, h)
    add = np.zeros((N, n_kv)) if m is None else m[:, :n_kv].astype(np.float64)
    if causal_past is not None:
        add = np.where(np.arange(n_kv)[None, :] <= causal_past + np.arange(N)[:, None], add, -np.inf)
    return add


# ---- the float64 reference and the bound ------------------------------------------------------------------------------------
def reference(Qop, Kop, Vop, mask, causal_past, scale, n_kv, plan):
    """Qop [B, H, N, D], Kop / Vop [B, Hkv, >= n_kv, D] float64 (operand mirror); mask: see mask_of_head; causal_past None | int; scale: the float the kernel
    is given; plan = launch_plan(...).  -> dict R, A, bound [B, N, H, D]; x2 [B, H, N, n_kv] (the scaled scores in base-2 units, -inf hidden); n_vis [B, N, H]"""
    B, H, N, D = Qop.shape
    Hkv = Kop.shape[1]
    r = H // Hkv
    _, chunk, splits = plan
    sc2 = float(np.float32(scale)) * LOG2E
    R, A, bound = (np.zeros((B, N, H, D)) for _ in range(3))
    x2 = np.full((B, H, N, n_kv), -np.inf)
    n_vis = np.zeros((B, N, H), np.int64)
    G = 1024 // D
    for b in range(B):
        for h in range(H):
            K, V, Q = Kop[b, h // r, :n_kv], Vop[b, h // r, :n_kv], Qop[b, h]
            s = Q @ K.T
            T = np.abs(Q) @ np.abs(K).T
            add = additive(mask, h, N, n_kv, causal_past)
            vis = np.isfinite(add)
            x = np.where(vis, s * sc2 + np.where(vis, add, 0.0) * LOG2E, -np.inf)
            x2[b, h] = x
            nv = vis.sum(1)
            n_vis[b, :, h] = nv
            live = nv > 0
            mx = np.where(live, np.max(x, axis=1, initial=-np.inf), 0.0)
            p = np.where(vis, np.exp2(x - mx[:, None]), 0.0)
            l = np.where(live, p.sum(1), 1.0)
            P = p / l[:, None]
            R[b, :, h] = P @ V
            A[b, :, h] = P @ np.abs(V)
            xabs = np.max(np.where(vis, np.abs(x), 0.0), axis=1)
            Gi = np.abs(s) * sc2 + np.abs(np.where(vis, add, 0.0)) * LOG2E + xabs[:, None]
            delta = np.where(vis, 2 * D * U32 * sc2 * T + 5 * U32 * Gi, 0.0)
            eps_row = np.log(2.0) * delta.max(1) + EXP_ULP
            pad = np.zeros((N, splits * chunk), bool)
            pad[:, :n_kv] = vis
            n_s = pad.reshape(N, splits, chunk).sum(2)
            n_in = n_s.max(1)
            c = 2.5 * n_in + 2 * (chunk // 64) + 5
            rel = U16 + 2 * eps_row + c * U32
            if splits > 1:
                rel = rel + ((splits + G - 1) // G + G + 10) * U32 + 2 * EXP_ULP
            # (a)'s absolute part, per split: n_s keys, max |v| over them, weight min(1, 2^(xmax_s - xmax + FA_TAU)) (no split: one chunk, weight 1)
            xp = np.full((N, splits * chunk), -np.inf)
            xp[:, :n_kv] = x
            xs_max = xp.reshape(N, splits, chunk).max(2)
            with np.errstate(invalid="ignore"):
                w = np.where(n_s > 0, np.minimum(1.0, np.exp2(xs_max - np.where(live, xs_max.max(1), 0.0)[:, None] + FA_TAU)), 0.0)
            absb = np.zeros((N, D))
            for sp in range(splits):
                lo, hi = sp * chunk, min(n_kv, sp * chunk + chunk)
                if not n_s[:, sp].any():
                    continue
                vm = np.max(np.where(vis[:, lo:hi, None], np.abs(V)[None, lo:hi, :], 0.0), axis=1)
                absb += (w[:, sp] * n_s[:, sp] * 2.0 ** -25)[:, None] * vm
            bound[b, :, h] = A[b, :, h] * rel[:, None] + absb
    return {"R": R, "A": A, "bound": bound, "x2": x2, "n_vis": n_vis}


# ---- the kernel's algorithm, step by step -------------------------------------------------------------------------------------
def emulate(Qop, Kop, Vop, mask, causal_past, scale, n_kv, plan, mutate=()):
    """operands as in reference(); Kop / Vop may hold rows beyond n_kv (a cache view: the `leak_hidden` mutant reads the first of them).
    -> out [B, N, H, D] float32, info: rescales [B, N, H] (moves of m_run from a finite value), big_p [B, N, H] (tiles with max p > 2),
    wmin [B, N, H] (the smallest non-zero merge weight, log2)"""
    mutate = set(mutate)
    assert mutate <= set(MUTATIONS) | set(LONG_MUTATIONS), mutate
    B, H, N, D = Qop.shape
    Hkv, rows = Kop.shape[1], Kop.shape[2]
    if "ignore_n_kv_dev" in mutate:
        n_kv = rows
    r = H // Hkv
    _, chunk, splits = plan
    f32 = np.float32
    sc2 = f32(f32(scale) * LOG2E32)
    mask_mul = f32(LOG2E32 / sc2)
    out = np.zeros((B, N, H, D), f32)
    rescales, big_p = np.zeros((B, N, H), np.int64), np.zeros((B, N, H), np.int64)
    wmin = np.zeros((B, N, H))
    leak = "leak_hidden" in mutate
    n_ext = min(rows, n_kv + 1) if leak else n_kv
    for b in range(B):
        for h in range(H):
            kb = 0 if "k_batch0" in mutate else b
            hk = ((h + 1) % H) // r if "kv_head_next" in mutate else h // r
            K32, V32, q32 = Kop[kb, hk, :n_ext].astype(f32), Vop[b, hk, :n_ext].astype(f32), Qop[b, h].astype(f32)
            s = q32 @ K32.T                                                    # fp32 accumulation of exact products
            m = mask_of_head(mask, h)
            kvs = np.arange(n_ext)[None, :]
            vis = np.ones((N, n_ext), bool)
            if m is not None:
                if "mask_row_next" in mutate:
                    m = np.roll(m, -1, axis=0)
                mv = np.full((N, n_ext), -np.inf, f32)
                mv[:, :n_kv] = m[:, :n_kv]
                vis &= mv != -np.inf
                with np.errstate(invalid="ignore"):
                    t = s + np.where(vis, mv * mask_mul, f32(0.0)).astype(f32)
            else:
                t = s
                vis[:, n_kv:] = False
            if causal_past is not None:
                lim = causal_past + np.arange(N)[:, None] + ("lim_plus" in mutate) - ("lim_minus" in mutate)
                vis &= (kvs <= lim) & (kvs < n_kv)
            if leak:                                                           # the first hidden key after the row's last visible one
                last = np.where(vis.any(1), n_ext - 1 - np.argmax(vis[:, ::-1], axis=1), -1)
                j = last + 1
                ok = j < n_ext
                vis[np.arange(N)[ok], j[ok]] = True
                t = t.copy()
                t[np.arange(N)[ok], j[ok]] = s[np.arange(N)[ok], j[ok]]
            if "drop_last_ragged" in mutate and n_kv % 64:
                vis[:, n_kv - 1] = False
            t = np.where(vis, t, f32(-np.inf)).astype(f32)
            ms, ls, os_ = [], [], []
            for sp in range(splits):
                kv_lo, kv_hi = sp * chunk, min(n_kv, sp * chunk + chunk)
                if leak and sp == splits - 1:
                    kv_hi = n_ext
                m_run, l_run, o = np.full(N, -np.inf, f32), np.zeros(N, f32), np.zeros((N, D), f32)
                for kv0 in range(kv_lo, kv_hi, 64):
                    tt = t[:, kv0:min(kv0 + 64, kv_hi)]
                    if not np.any(tt != -np.inf):
                        continue                                               # nothing of this tile visible to any row
                    mx = (np.max(tt, axis=1) * sc2).astype(f32)
                    with np.errstate(invalid="ignore"):
                        grow = mx > m_run + f32(FA_TAU)
                        alpha = np.where(grow, np.exp2(np.where(grow, m_run - mx, f32(0.0))), f32(1.0)).astype(f32)
                    rescales[b, :, h] += grow & (m_run != -np.inf)
                    if "no_l_rescale" not in mutate:
                        l_run = l_run * alpha
                    if "no_o_rescale" not in mutate:
                        o = o * alpha[:, None]
                    m_run = np.where(grow, mx, m_run).astype(f32)
                    msafe = np.where(m_run == -np.inf, f32(0.0), m_run).astype(np.float64)
                    p = np.exp2((tt.astype(np.float64) * np.float64(sc2) - msafe[:, None]).astype(f32)).astype(f32)      # one rounding, as the fma
                    big_p[b, :, h] += p.max(1) > 2.0
                    l_run = (l_run + p.sum(1, dtype=f32)).astype(f32)
                    o = o + p.astype(np.float16).astype(f32) @ V32[kv0:kv0 + tt.shape[1]]
                ms.append(m_run), ls.append(l_run), os_.append(o)
            if splits == 1:
                l = ls[0]
                inv = np.where(l == 0, f32(0.0), f32(1.0) / np.where(l == 0, f32(1.0), l)).astype(f32)
                out[b, :, h] = os_[0] * inv[:, None]
                continue
            ms, ls, os_ = np.stack(ms), np.stack(ls), np.stack(os_)            # [splits, N], [splits, N, D]
            M = ms.max(0)
            Ms = np.where(M == -np.inf, f32(0.0), M)
            w = np.exp2(ms - Ms[None]).astype(f32)
            if "empty_split_weight_1" in mutate:
                w, ls = np.where(ms == -np.inf, f32(1.0), w), np.where(ms == -np.inf, f32(1.0), ls)
            wmin[b, :, h] = np.min(np.where(w > 0, np.log2(np.where(w > 0, w, 1.0)), 0.0), axis=0)
            if "merge_w1" in mutate:
                w = np.ones_like(w)
            L = (ls if "merge_l_unweighted" in mutate else w * ls).sum(0, dtype=f32)
            acc = (w[:, :, None] * os_).sum(0, dtype=f32)
            inv = np.where(L == 0, f32(0.0), f32(1.0) / np.where(L == 0, f32(1.0), L)).astype(f32)
            out[b, :, h] = acc * inv[:, None]
    return out, {"rescales": rescales, "big_p": big_p, "wmin": wmin}


# ---- score profiles ----------------------------------------------------------------------------------------------------------
PROFILES = ("ascending", "stairs7", "descending", "sink_mixed", "edge", "split_maxima", "gaussian")
SIGMA = 0.25                     # the Gaussian part of q and k: scale q.k has a standard deviation of SIGMA^2 nats (0.09 base-2 units)


def levels(name, Hkv, rows, n_kv, chunk, lead):
    """the steered part of the scores in base-2 units, per (kv head, key): [Hkv, rows]"""
    i = np.arange(rows, dtype=np.float64)
    tile = np.floor(i / 64)
    lev = np.zeros((Hkv, rows))
    if name == "ascending":
        lev[:] = 13.0 * tile + 0.03 * (i % 64)
    elif name == "stairs7":
        lev[:] = 7.0 * tile + 0.01 * (i % 64)
    elif name == "descending":
        lev[:] = -np.minimum(15.0 * tile, 30.0) - 0.01 * (i % 64)
    elif name == "sink_mixed":
        lev[:, lead] = 14.0
    elif name == "edge":
        lev[:] = i * min(1.0, 40.0 / rows) * LOG2E
    elif name == "split_maxima":
        lev[:] = -6.0 * (np.floor(i / chunk) % 3)
        for hk in range(Hkv):
            lev[hk, 0 if hk % 2 == 0 else n_kv - 1] = 45.0
    lev -= 0.5 * (lev[:, :n_kv].max() + lev[:, :n_kv].min())
    return lev


def make_mask(mode, N, H, n_kv, n_past, plan, rng):
    """-> None | float16 [N, n_kv] | float16 [H, N, n_kv], and the number of leading keys hidden from every query"""
    decode, chunk, splits = plan
    kv, n = np.arange(n_kv)[None, :], np.arange(N)[:, None]
    if mode is None:
        return None, 0
    if mode == "causal":                              # CoreAttention::before_eval: -inf beyond n_past + n
        return np.where(kv <= n_past + n, 0.0, -np.inf).astype(np.float16), 0
    if mode == "bias":                                # finite additive values; decode: one middle split fully masked; prefill: fully masked leading tile(s), one fully masked query
        m = (rng.standard_normal((N, n_kv)) * 0.25).astype(np.float32)
        lead = 0
        if decode:
            if splits > 2:
                m[:, (splits // 2) * chunk:(splits // 2 + 1) * chunk] = -np.inf
        else:
            lead = 64
            m[:, :lead] = -np.inf
            m[N // 2, :] = -np.inf
        return m.astype(np.float16), lead
    if mode == "heads":                               # ne[2] == H: causal, and every head hides its own fifth of the keys (never the first or the last)
        hh = np.arange(H)[:, None, None]
        keep = ((kv[None] + hh) % 5 != 0) | (kv[None] == 0) | (kv[None] == n_kv - 1)
        return np.where((kv[None] <= n_past + n[None]) & keep, 0.0, -np.inf).astype(np.float16), 0
    raise ValueError(mode)


def profile(name, D, N, H, Hkv, n_kv, n_past, kv_t, seed, mask_mode=None, rows=None, scratch=True, plan=None):
    """-> q float32 [H, N, D]; k, v [Hkv, rows, D] float16 or Q8_0 block bytes [Hkv, rows, D / 32 * 34]; mask (make_mask).  rows >= n_kv: the rows of a cache
    view past n_kv continue the profile.  Scores are steered through ONE shared unit direction u added to otherwise Gaussian q and k (whose Gaussian parts are
    orthogonal to u): scale q.k = level(key) gate(query, head) + Gaussian noise, in base-2 units.  plan: the (decode, chunk, splits) of a launcher other than
    launch_fattn (tests/attn_long_model.py)"""
    rows = rows or n_kv
    rng = np.random.default_rng([PROFILES.index(name), D, N, H, Hkv, n_kv, n_past, kv_t, seed])
    plan = plan or launch_plan(N, H, Hkv, n_kv, scratch)
    mask, lead = make_mask(mask_mode, N, H, n_kv, n_past, plan, rng)
    u = rng.choice([-1.0, 1.0], D) / np.sqrt(D)
    orth = lambda g: g - (g @ u)[..., None] * u
    sigma = 0.1 if name == "edge" else SIGMA          # edge: a slope of 40 nats over all rows must order neighbouring keys
    gq, gk = orth(rng.standard_normal((H, N, D))) * sigma, orth(rng.standard_normal((Hkv, rows, D))) * sigma
    v = rng.standard_normal((Hkv, rows, D))
    # three columns in four keep ONE sign over all keys (|R| = A there: the bound is a relative one); the last quarter is zero-mean and cancels as real V does
    v[..., :3 * D // 4] = np.abs(v[..., :3 * D // 4]) * rng.choice([-1.0, 1.0], 3 * D // 4)
    if name == "gaussian":                            # the data of tests/test_gpu_fattn.py
        q, k = rng.standard_normal((H, N, D)) * 1.5, rng.standard_normal((Hkv, rows, D)) * 0.8
    else:
        lev = levels(name, Hkv, rows, n_kv, plan[1], lead)
        sc2 = LOG2E / np.sqrt(D)
        c = max(1.0, np.sqrt(np.abs(lev).max() / sc2))
        gate = np.ones((H, N))
        if name == "sink_mixed":
            gate = ((np.arange(N)[None, :] + np.arange(H)[:, None]) % 2 == 0).astype(np.float64)
            v[:, lead] *= 8.0
        q = gq + (c * gate)[..., None] * u
        k = gk + (lev / (c * sc2))[..., None] * u
    q = q.astype(np.float32)
    if kv_t == F16:
        return q, k.astype(np.float16), v.astype(np.float16), mask
    return q, q8_0_quantize(k), q8_0_quantize(v), mask


# ---- the cases the CPU model tests and the GPU tests share ---------------------------------------------------------------------
# (api, kv type, D, N, H, Hkv, n_kv, n_past, profile(s: one per batch), mask mode, ML)
#   api "fa": cllm_op_flash_attn_ext; "prefill": cllm_op_attn_prefill in prefill mode 0 (in-kernel causal mask, V^T cache of ML positions, no split-KV scratch)
def _cases():
    c = []
    for kv_t in (F16, Q8_0):                          # decode: packed GQA rows, 5 splits with a 44-position tail
        for p in ("ascending", "descending", "split_maxima", "sink_mixed"):
            for mm in (None, "causal", "bias"):
                c.append(("fa", kv_t, 128, 1, 8, 2, 300, 299, (p,), mm, 0))
    for n_kv in (64, 65, 128):                        # the split boundary
        c.append(("fa", F16, 128, 1, 8, 2, n_kv, n_kv - 1, ("ascending",), None, 0))
        c.append(("fa", Q8_0, 128, 1, 8, 2, n_kv, n_kv - 1, ("split_maxima",), "causal", 0))
    c.append(("fa", F16, 64, 1, 4, 4, 8128, 8127, ("split_maxima",), None, 0))      # 127 splits
    for kv_t in (F16, Q8_0):                          # the decode / prefill switch: N r = 32 and 33
        c.append(("fa", kv_t, 128, 8, 8, 2, 78, 70, ("edge",), "causal", 0))
        c.append(("fa", kv_t, 128, 11, 6, 2, 81, 70, ("edge",), "causal", 0))
    for D in (128, 64):                               # prefill: two query blocks, the second ragged
        for kv_t in (F16, Q8_0):
            for p, mm in (("ascending", "causal"), ("ascending", "bias"), ("stairs7", "causal"), ("stairs7", "bias"), ("edge", "causal"),
                          ("sink_mixed", "causal"), ("sink_mixed", "bias")):
                c.append(("fa", kv_t, D, 130, 4, 2, 191, 61, (p,), mm, 0))
    # ne[3] = 2 with different K / V per batch, a mask of ne[2] = H with a different visible set per head
    c.append(("fa", F16, 128, 1, 8, 2, 300, 299, ("ascending", "split_maxima"), "heads", 0))
    c.append(("fa", Q8_0, 64, 130, 4, 2, 191, 61, ("edge", "descending"), "heads", 0))
    c.append(("fa", F16, 128, 8, 8, 2, 78, 70, ("sink_mixed", "edge"), "heads", 0))
    for N, n_past in ((130, 0), (130, 61), (200, 0), (200, 61)):
        for p in ("ascending", "edge"):
            c.append(("prefill", F16, 128, N, 4, 2, n_past + N, n_past, (p,), None, (n_past + N + 23) // 8 * 8))
    c.append(("prefill", F16, 64, 130, 4, 2, 191, 61, ("edge",), None, 208))
    return c


CASES = _cases()
case_id = lambda c: "-".join("+".join(v) if isinstance(v, tuple) else str(v) for v in c)


@functools.lru_cache(maxsize=None)
def case_data(case):
    """-> dict: q [B, H, N, D] float32; k, v [B, Hkv, rows, ..] as the cache holds them; mask; plan; causal_past; scale; and ref = reference(...) over the
    operand mirror.  Computed once per case and shared; nobody writes to it"""
    api, kv_t, D, N, H, Hkv, n_kv, n_past, profs, mm, ML = case
    rows = ML if api == "prefill" else n_kv
    parts = [profile(p, D, N, H, Hkv, n_kv, n_past, kv_t, b, mm, rows, scratch=api == "fa") for b, p in enumerate(profs)]
    q, k, v = (np.stack([p[i] for p in parts]) for i in range(3))
    mask = parts[0][3]
    plan = launch_plan(N, H, Hkv, n_kv, scratch=api == "fa")
    scale = np.float32(1.0 / np.sqrt(D))
    causal_past = n_past if api == "prefill" else None
    Qop, Kop, Vop = q_operand(kv_t, q), kv_operand(kv_t, k), kv_operand(kv_t, v)
    ref = reference(Qop, Kop, Vop, mask, causal_past, scale, n_kv, plan)
    for a in (q, k, v, Qop, Kop, Vop) + tuple(ref.values()) + ((mask,) if mask is not None else ()):
        a.setflags(write=False)
    return {"q": q, "k": k, "v": v, "mask": mask, "plan": plan, "scale": scale, "causal_past": causal_past, "n_kv": n_kv,
            "Qop": Qop, "Kop": Kop, "Vop": Vop, "ref": ref}


def emulate_case(case, mutate=()):
    d = case_data(case)
    return emulate(d["Qop"], d["Kop"], d["Vop"], d["mask"], d["causal_past"], d["scale"], d["n_kv"], d["plan"], mutate)
