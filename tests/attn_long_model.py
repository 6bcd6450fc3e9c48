"""Single-token attention above the long-context threshold (CLLM_ATTN_LONG): the inputs, plans and references the CPU model tests (test_attn_long_model.py) and
the GPU tests (test_gpu_attn_long.py, test_gpu_ops.py) share.  Plain numpy and the CPU oracle: no GPU, no package import.

1. long_flash_plan(): decode / chunk / splits as launch_attn_long_flash (fattn.hip) computes them from its scratch.  The split-KV flash form is judged with
   fattn_model's reference, bound and emulation under that plan: VL = 1, no mask, n_kv read on the device (position + 1), the padded extent splits * chunk >= ML,
   so whole splits see no key and enter the merge as (m = -inf, l = 0).  Nothing here adds a constant to that bound.
2. decode_inputs(): qkv / caches of one call of cllm_op_rope_kv_attn_decode whose ROTATED operands are given (a fattn_model score profile), with the caches
   POISONED past n_kv: the V cache holds fp16 NaN there, the K cache values of exponent 2^14.  The node sequence the results are compared with views n_kv
   positions only, so the reference never sees the poison; a kernel that multiplies a zero probability with a stale V entry, or takes a maximum over a stale
   score, does.
3. soft_max_boundary_rows(), attn_boundary_case(): rows whose soft-max total puts (float)(1 / sum) next to a float rounding boundary, where every soft-max kernel
   (soft_total_order_safe, common.h) gives up its tree total and redoes the sum in the reference's serial order.  Random rows get there once in ~2^20.
"""
import ctypes
import ctypes.util
import functools

import numpy as np

import fattn_model as FM
import oracle as O

f32, f64 = np.float32, np.float64
FREQ_BASE = 500000.0


def attn_scale(hd):
    return float(f32(1.0) / np.sqrt(f32(hd)))


# ---- (1) the split-KV flash form ---------------------------------------------------------------------------------------------------
def decode_wsize(nh, ML):
    """cllm_attn_decode_wsize above the threshold: fp32 scores + fp16 probabilities of every head"""
    return nh * ML * 6


def long_flash_plan(nh, hd, ML, s_bytes=None, nkv=None):
    """-> (decode, chunk, splits) as launch_attn_long_flash computes them (q_bytes, max_splits, per, tiles), None where it returns CLLM_E_UNSUPPORTED.
    s_bytes: the scratch the caller passes (default: what cllm_attn_decode_wsize asks for)"""
    s_bytes = decode_wsize(nh, ML) if s_bytes is None else s_bytes
    if hd not in (64, 128) or ML % 8 or ML > 1 << 30:
        return None
    if nkv is not None and (nkv <= 0 or nh % nkv or nh // nkv > 32):
        return None
    q_bytes = (nh * hd * 4 + 255) & ~255
    if s_bytes <= q_bytes:
        return None
    max_splits = min((s_bytes - q_bytes) // (nh * (hd + 4) * 4), FM.FA_MAX_SPLITS)
    if max_splits < 4:
        return None
    tiles = (ML + 63) // 64
    per = max((tiles + max_splits - 1) // max_splits, tiles // 32, 1)
    return True, per * 64, (tiles + per - 1) // per


def rope(x, pos, hd, mode):
    """the oracle's ROPE of [heads, hd] float32 at one position (a negative position: the inverse rotation, up to the roundings of the rotation)"""
    x = np.ascontiguousarray(x, f32).reshape(1, -1, hd)
    y = np.zeros_like(x)
    O.rope(O.tensor(x, O.F32, [hd, x.shape[1], 1]), np.array([pos], np.int32), None, O.tensor(y, O.F32, [hd, x.shape[1], 1]), hd, mode, FREQ_BASE)
    return y[0]


def poison(kc, vc, n_kv, rng):
    """in place: everything past n_kv is garbage that shows: V NaN, K +-[2^14, 2^15)"""
    ML = kc.shape[0]
    if n_kv < ML:
        kc[n_kv:] = (rng.choice([-1.0, 1.0], (ML - n_kv, kc.shape[1])) * rng.uniform(16384.0, 32752.0, (ML - n_kv, kc.shape[1]))).astype(np.float16)
        vc[:, n_kv:] = np.float16(np.nan)


def decode_inputs(hd, nh, nkv, mode, ML, n_kv, q_rot, K, V, rng):
    """q_rot [nh, hd], K / V [nkv, >= n_kv, hd]: the operands the attention is to see AFTER RoPE (row n_kv - 1 of K / V: the new token's).
    -> qkv (un-rotated projections), kc0 [ML, KD], vc0 [KD, ML] (fp16, poisoned past n_kv, garbage at the new token's row / column as well: the call writes
    them), and the operands it really gets: Q [nh, hd] float32 (the oracle's rotation of qkv; the kernel rounds it to fp16), Kop / Vop [nkv, ML, hd] fp16 with
    the row the call writes (the inverse rotation and the rotation each round: ~1e-7 of the profile, but these ARE the operands)"""
    QD, KD, pos = nh * hd, nkv * hd, n_kv - 1
    kc0, vc0 = np.zeros((ML, KD), np.float16), np.zeros((KD, ML), np.float16)
    kc0[:n_kv] = np.ascontiguousarray(K[:, :n_kv].transpose(1, 0, 2)).reshape(n_kv, KD)
    vc0[:, :n_kv] = np.ascontiguousarray(V[:, :n_kv].transpose(0, 2, 1)).reshape(KD, n_kv)
    poison(kc0, vc0, pos, rng)
    qkv = np.concatenate([rope(q_rot, -pos, hd, mode).reshape(QD), rope(K[:, pos].astype(f32), -pos, hd, mode).reshape(KD), V[:, pos].astype(f32).reshape(KD)])
    qkv = np.ascontiguousarray(qkv, f32)
    Q = rope(qkv[:QD].reshape(nh, hd), pos, hd, mode)
    Kop, Vop = np.zeros((nkv, ML, hd), np.float16), np.zeros((nkv, ML, hd), np.float16)
    Kop[:] = kc0.reshape(ML, nkv, hd).transpose(1, 0, 2)
    Vop[:] = vc0.reshape(nkv, hd, ML).transpose(0, 2, 1)
    Kop[:, pos] = rope(qkv[QD:QD + KD].reshape(nkv, hd), pos, hd, mode).astype(np.float16)
    Vop[:, pos] = qkv[QD + KD:].reshape(nkv, hd).astype(np.float16)
    return qkv, kc0, vc0, Q, Kop, Vop


FLASH_SHAPES = [(128, 8, 2, 0), (128, 8, 8, 2), (64, 8, 4, 0), (64, 4, 1, 2), (128, 16, 2, 2)]      # (hd, nh, nkv, rope mode): r2 = 4, 1, 2, 4, 8
FLASH_ML = (1024, 2112)                          # 2112: 33 tiles, no multiple of 64 x per: the last split is ragged
FLASH_PROFILES = ("split_maxima", "ascending", "gaussian")


def flash_n_kv(ML):
    return (513, 576, 577, ML - 1, ML)


# (hd, nh, nkv, mode, ML, n_kv, profile)
FLASH_CASES = [s + (ML, n_kv, p) for s in FLASH_SHAPES for ML in FLASH_ML for n_kv in flash_n_kv(ML) for p in FLASH_PROFILES]
flash_id = lambda c: "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def flash_case_inputs(case):
    """-> dict: qkv, kc0, vc0 (the call's inputs), plan, n_kv, scale, Qop / Kop / Vop [1, ..] float64 (the operand mirror, poison included past n_kv).
    Computed once per case and shared; nobody writes to it"""
    hd, nh, nkv, mode, ML, n_kv, prof = case
    plan = long_flash_plan(nh, hd, ML, nkv=nkv)
    q, k, v, _ = FM.profile(prof, hd, 1, nh, nkv, n_kv, n_kv - 1, FM.F16, 0, None, rows=n_kv, plan=plan)
    rng = np.random.default_rng([FLASH_PROFILES.index(prof), hd, nh, nkv, mode, ML, n_kv])
    qkv, kc0, vc0, Q, Kop, Vop = decode_inputs(hd, nh, nkv, mode, ML, n_kv, q[:, 0], k, v, rng)
    Qop = FM.q_operand(FM.F16, Q)[None, :, None, :]
    Kop, Vop = FM.kv_operand(FM.F16, Kop)[None], FM.kv_operand(FM.F16, Vop)[None]
    d = {"qkv": qkv, "kc0": kc0, "vc0": vc0, "plan": plan, "n_kv": n_kv, "scale": f32(attn_scale(hd)), "Qop": Qop, "Kop": Kop, "Vop": Vop}
    for a in (qkv, kc0, vc0, Qop, Kop, Vop):
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def flash_case_data(case):
    """flash_case_inputs and ref = fattn_model.reference(...) under the long plan: (a)-(e) with VL = 1, no mask, a merge over `splits` partials"""
    d = dict(flash_case_inputs(case))
    d["ref"] = FM.reference(d["Qop"], d["Kop"], d["Vop"], None, None, d["scale"], d["n_kv"], d["plan"])
    for a in d["ref"].values():
        a.setflags(write=False)
    return d


def emulate_flash_case(case, mutate=()):
    d = flash_case_data(case)
    with np.errstate(invalid="ignore", over="ignore"):      # ignore_n_kv_dev walks the poison
        return FM.emulate(d["Qop"], d["Kop"], d["Vop"], None, None, d["scale"], d["n_kv"], d["plan"], mutate)


def random_case(hd, nh, nkv, mode, ML, n_kv, seed=0):
    """ordinary Gaussian projections and caches (the data of test_rope_kv_attn_decode_equals_the_node_sequence), poisoned past n_kv"""
    rng = np.random.default_rng([hd, nh, nkv, mode, ML, n_kv, seed])
    QD, KD = nh * hd, nkv * hd
    qkv = rng.standard_normal(QD + 2 * KD).astype(f32)
    kc0, vc0 = rng.standard_normal((ML, KD)).astype(np.float16), rng.standard_normal((KD, ML)).astype(np.float16)
    poison(kc0, vc0, n_kv, rng)
    return qkv, kc0, vc0


# ---- (3) the reference's soft_max, restated -------------------------------------------------------------------------------------------
def _fma(a, b, c, exact=True):
    """fmaf over float32 arrays: the product is exact in double; exact=True rounds the sum to ODD in double first (the residual of TwoSum decides), so that the
    final rounding to float32 is the single rounding of an fma; exact=False rounds twice (differs once in ~2^29: only for searching)"""
    with np.errstate(all="ignore"):                                 # (arguments far outside the soft_max's range overflow on purpose)
        p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
        c = np.asarray(c, f32).astype(f64)
        s = p + c
        if exact:
            bb = s - p
            err = (p - (s - bb)) + (c - bb)
            s = np.atleast_1d(s)
            fix = (np.broadcast_to(err, s.shape) != 0) & ((s.view(np.int64) & 1) == 0)
            s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


_H = float.fromhex


def v_expf(x, exact=True):
    """one lane of the reference's AVX2 ggml_v_expf (ggml-cpu/vec.h:1230-1267), op for op, over a float32 array"""
    x = np.atleast_1d(np.asarray(x, f32))
    r = f32(_H("0x1.8p23"))
    z = _fma(x, f32(_H("0x1.715476p+0")), r, exact)
    n = z - r
    b = _fma(-n, f32(_H("0x1.7f7d1cp-20")), _fma(-n, f32(_H("0x1.62e4p-1")), x, exact), exact)
    e = z.view(np.uint32) << np.uint32(23)
    k = (e + np.uint32(0x3f800000)).view(f32)
    c = np.abs(n) > f32(126.0)
    u = b * b
    j = _fma(_fma(_fma(f32(_H("0x1.0e4020p-7")), b, f32(_H("0x1.573e2ep-5")), exact), u, _fma(f32(_H("0x1.555e66p-3")), b, f32(_H("0x1.fffdb6p-2")), exact), exact),
             u, f32(_H("0x1.ffffecp-1")) * b, exact)
    res = _fma(j, k, k, exact)
    if np.any(c):
        g = np.where(n <= 0, np.uint32(0x82000000), np.uint32(0))
        s1 = (g + np.uint32(0x7f000000)).view(f32)
        s2 = (e - g).view(f32)
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            big = np.where(np.abs(n) > f32(192.0), s1 * s1, _fma(s2, j, s2, exact) * s1)
        res = np.where(c, big, res)
    return res


_libm = None


def libm_expf(x):
    """the host's expf (what the reference's scalar tail calls), element by element"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.expf.restype, _libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    return np.array([_libm.expf(float(v)) for v in np.atleast_1d(x)], f32)


def group_sums(e):
    """the float sums of whole groups of 8 with the reference's pairing (extractf128 add, movehl add, movehdup add)"""
    v = e.reshape(-1, 8)
    a = v[:, :4] + v[:, 4:]
    return (a[:, 0] + a[:, 2]) + (a[:, 1] + a[:, 3])


def soft_max_terms(x):
    """-> the exponentials of ggml_vec_soft_max_f32 over one row (polynomial below n & ~7, expf for the leftovers), float32"""
    x = np.asarray(x, f32)
    nv = x.size & ~7
    d = x - x.max()
    return np.concatenate([v_expf(d[:nv]), libm_expf(d[nv:]) if nv < x.size else np.zeros(0, f32)]).astype(f32)


def serial_total(e):
    """the reference's double total: the group sums one by one, then the leftovers (np.cumsum adds in order)"""
    nv = e.size & ~7
    t = np.concatenate([group_sums(e[:nv]).astype(f64), e[nv:].astype(f64)])
    return float(np.cumsum(t)[-1])


def pairwise_total(e):
    """the same terms added as a tree (numpy's pairwise sum): what a kernel that ignored the order would get"""
    nv = e.size & ~7
    return float(np.sum(np.concatenate([group_sums(e[:nv]).astype(f64), e[nv:].astype(f64)])))


def boundary_distance(total):
    """|low 29 bits of the mantissa of 1 / total - 2^28|, as soft_total_order_safe (common.h) measures it"""
    rinv = np.atleast_1d(1.0 / np.asarray(total, f64))
    return np.abs((rinv.view(np.int64) & 0x1fffffff) - 0x10000000)


def half_window(n):
    """half of soft_total_order_safe's window m + 24, m = n >> 3: a tree total differs from the serial one by at most (m + log2 m) / 2 of these units, so
    it lands inside the whole window whenever the serial one is inside this half"""
    return ((n >> 3) + 24) / 2


def on_boundary(x):
    """the condition on a row: the reference's own serial total within half of the kernels' window"""
    return bool(boundary_distance(serial_total(soft_max_terms(x)))[0] <= half_window(np.asarray(x).size))


def soft_max_restated(x):
    """the probabilities of one row as the reference computes them"""
    e = soft_max_terms(x)
    return e * f32(1.0 / serial_total(e))


def _sweep_floats(lo_bits, count):
    return (np.uint32(lo_bits) + np.arange(count, dtype=np.uint32)).view(f32)


def soft_max_boundary_rows(n, rows, rng):
    """-> x float32 [rows, n], deciding bool [rows].  Random logits (3 N(0, 1), the rows of test_soft_max); ONE element of the last whole group of 8 is swept over
    the consecutive floats of the binade below the row's maximum until the reference's serial total meets on_boundary().  The hit rate per candidate is
    (n / 8 + 24) / 2^29: a binade (2^23 candidates) gives 0.5 (n = 64) to 8 (n = 4097) rows, so rows are redrawn until one hits.  deciding: a pairwise total
    rounds 1 / sum to ANOTHER float than the serial one (reported; not required: it needs the reciprocal within ~1e-16 of a tie)"""
    assert n >= 16
    out, deciding = np.zeros((rows, n), f32), np.zeros(rows, bool)
    nv, CH = n & ~7, 1 << 20
    for r in range(rows):
        for attempt in range(200):
            x = (rng.standard_normal(n) * 3).astype(f32)
            js = nv - 8 + int(rng.integers(8))
            am = int(np.argmax(x))
            if am >= nv - 8:                                        # the maximum stays out of the swept group
                x[am], x[0] = x[0], x[am]
            mx = x.max()
            if mx < 2.0:
                continue
            lo = f32(2.0 ** (np.floor(np.log2(mx)) - 1))            # the binade [lo, 2 lo) below the maximum: candidates never move it
            x[js] = lo
            e = soft_max_terms(x)
            gs = group_sums(e[:nv]).astype(f64)
            prefix = float(np.cumsum(gs[:-1])[-1]) if gs.size > 1 else 0.0
            last = e[nv - 8:nv].copy()
            l = js - (nv - 8)
            found = None
            for c0 in range(0, 1 << 23, CH):
                xc = _sweep_floats(lo.view(np.uint32) + np.uint32(c0), CH)
                v = np.broadcast_to(last, (CH, 8)).copy()
                v[:, l] = v_expf(xc - mx, exact=False)
                a = v[:, :4] + v[:, 4:]
                tot = prefix + ((a[:, 0] + a[:, 2]) + (a[:, 1] + a[:, 3])).astype(f64)
                for t in e[nv:]:
                    tot = tot + f64(t)
                for i in np.flatnonzero(boundary_distance(tot) <= half_window(n)):
                    x[js] = xc[i]
                    if on_boundary(x):                              # the exact restatement has the last word
                        found = i
                        break
                if found is not None:
                    break
            if found is not None:
                break
        else:
            raise RuntimeError(f"no boundary row at n = {n}")
        out[r] = x
        e = soft_max_terms(x)
        deciding[r] = f32(1.0 / serial_total(e)) != f32(1.0 / pairwise_total(e))
    return out, deciding


@functools.lru_cache(maxsize=None)
def boundary_rows(n, rows, seed):
    """soft_max_boundary_rows, seeded, computed once per (n, rows, seed)"""
    x, dec = soft_max_boundary_rows(n, rows, np.random.default_rng([n, rows, seed]))
    x.setflags(write=False)
    return x, dec


# ---- the node sequence on the CPU oracle ---------------------------------------------------------------------------------------------
def oracle_node_sequence(hd, nh, nkv, mode, ML, n_kv, qkv, kc0, vc0):
    """ROPE -> SET_ROWS, CPY of the V column, ROPE(q), MUL_MAT(K, Q), SCALE, SOFT_MAX, MUL_MAT(V, P) over views of n_kv positions, all on the oracle.
    -> dict k_cache, v_cache (fp16), scores (scaled) [nh, n_kv], p [nh, n_kv], out [nh * hd]"""
    QD, KD, pos = nh * hd, nkv * hd, n_kv - 1
    kc, vc = np.array(kc0, np.float16), np.array(vc0, np.float16)
    q = rope(qkv[:QD].reshape(nh, hd), pos, hd, mode)
    kc[pos] = rope(qkv[QD:QD + KD].reshape(nkv, hd), pos, hd, mode).reshape(KD).astype(np.float16)
    vc[:, pos] = qkv[QD + KD:].astype(np.float16)
    sc, ctx = np.zeros((nh, 1, n_kv), f32), np.zeros((nh, 1, hd), f32)
    S = O.tensor(sc, O.F32, [n_kv, 1, nh])
    O.mul_mat(O.tensor(kc, O.F16, [hd, n_kv, nkv], nb=[2, KD * 2, hd * 2, KD * ML * 2]), O.tensor(q, O.F32, [hd, 1, nh], nb=[4, nh * hd * 4, hd * 4, nh * hd * 4]), S)
    O.scale(S, S, attn_scale(hd))
    scores = sc[:, 0].copy()
    O.soft_max(S, None, S)
    O.mul_mat(O.tensor(vc, O.F16, [n_kv, hd, nkv], nb=[2, ML * 2, ML * hd * 2, ML * KD * 2]), S, O.tensor(ctx, O.F32, [hd, 1, nh]))
    return {"k_cache": kc, "v_cache": vc, "scores": scores, "p": sc[:, 0].copy(), "out": ctx.reshape(QD).copy()}


def attn_boundary_case(hd, nh, nkv, ML, n_past, mode, rng):
    """-> dict qkv, kc0, vc0, hits (the heads whose soft-max row meets on_boundary()), oracle (oracle_node_sequence of the case).
    Random projections and caches; then the score of ONE cached position j < n_past is steered through its stored K row (post-RoPE: never rotated again):
    the row of one kv head becomes two non-zero fp16 entries at dims a = 0 and b = 1, which feed different accumulators of ggml_vec_dot_f16, every other product
    is an exact zero, so the score of head h there is fl(fl(q_a k_a + q_b k_b) scale).  fp16 pairs (k_a, k_b) are enumerated for the r heads of the group until
    one head's serial total meets the condition; the oracle's own scores then decide which heads hit."""
    n_kv, QD, KD, r = n_past + 1, nh * hd, nkv * hd, nh // nkv
    qkv = rng.standard_normal(QD + 2 * KD).astype(f32)
    kc0, vc0 = rng.standard_normal((ML, KD)).astype(np.float16), rng.standard_normal((KD, ML)).astype(np.float16)
    poison(kc0, vc0, n_kv, rng)
    qh = rope(qkv[:QD].reshape(nh, hd), n_past, hd, mode).astype(np.float16).astype(f32)
    base = oracle_node_sequence(hd, nh, nkv, mode, ML, n_kv, qkv, kc0, vc0)["scores"]
    scale, nv, a, b = f32(attn_scale(hd)), n_kv & ~7, 0, 1
    pos16 = np.arange(0x3c00, 0x5000, dtype=np.uint16).view(np.float16).astype(f32)            # [1, 32): five binades
    kb_all = np.concatenate([pos16, -pos16])
    ka_all = np.concatenate([pos16[2048:], -pos16[2048:]])                                     # [4, 32)
    ka_all = ka_all[rng.permutation(ka_all.size)]
    for attempt in range(4 * nkv):
        g, G = attempt % nkv, nv // 8 - 1 - attempt // nkv
        j = 8 * G
        heads = []
        for h in range(g * r, g * r + r):
            x = base[h].copy()
            x[j] = -np.inf
            mx = x.max()
            x[j] = mx                                                # (a placeholder: the candidates replace its exponential)
            e = np.concatenate([v_expf(x[:nv] - mx), libm_expf(x[nv:] - mx) if nv < n_kv else np.zeros(0, f32)]).astype(f32)
            gs = group_sums(e[:nv]).astype(f64)
            heads.append((h, mx, float(np.cumsum(gs[:G])[-1]) if G else 0.0, e[j:j + 8].copy(), np.concatenate([gs[G + 1:], e[nv:].astype(f64)])))
        for c0 in range(0, ka_all.size, 128):
            ka = ka_all[c0:c0 + 128, None]
            for h, mx, prefix, grp, rest in heads:
                s = ((qh[h, a] * ka + qh[h, b] * kb_all[None, :]) * scale).astype(f32).reshape(-1)
                ok = (s < mx - f32(0.1)) & (s > mx - f32(6.0))
                v = np.broadcast_to(grp, (s.size, 8)).copy()
                v[:, 0] = v_expf(s - mx, exact=False)
                aa = v[:, :4] + v[:, 4:]
                tot = prefix + ((aa[:, 0] + aa[:, 2]) + (aa[:, 1] + aa[:, 3])).astype(f64)
                for t in rest:
                    tot = tot + t
                for i in np.flatnonzero(ok & (boundary_distance(tot) <= half_window(n_kv))):
                    kc = kc0.copy()
                    kc[j, g * hd:(g + 1) * hd] = 0
                    kc[j, g * hd + a], kc[j, g * hd + b] = ka[i // kb_all.size, 0], kb_all[i % kb_all.size]
                    orc = oracle_node_sequence(hd, nh, nkv, mode, ML, n_kv, qkv, kc, vc0)
                    hits = [hh for hh in range(nh) if on_boundary(orc["scores"][hh])]
                    if h in hits:
                        return {"qkv": qkv, "kc0": kc, "vc0": vc0, "hits": hits, "oracle": orc, "j": j}
    raise RuntimeError("no boundary head found")


# ---- the case lists of tests/test_gpu_attn_long.py: (kind, hd, nh, nkv, mode, ML, n_kv, extra) ------------------------------------------------
#   kind "flash": extra = the score profile (flash_case_inputs);  "random": random_case, extra = a seed;  "short_ws": random_case with one byte of scratch less than
#   cllm_attn_decode_wsize asks for;  "boundary": boundary_attn_case;  "boundary_nt": the same inputs called WITHOUT a RoPE table (rope_cs = NULL: the general
#   kernel k_attn_decode computes cos / sin itself)
N3 = (513, 544, 545, 1023, 1024, 1025, 1032)     # k_attn_long_pv: nch 16 | 17 (the clamped refill loop alone, then one whole group before it), 31, 32 (i0 + 2 UC <= nch), leftovers 0 .. 31
INSTANCES = [("random", hd, r2 * 2, 2, mode, 1024, 777, 0) for hd in (64, 128) for mode in (0, 2) for r2 in (1, 2, 4, 8)]
CASE_LISTS = {
    # CLLM_ATTN_LONG_FLASH=1: the split-KV flash form; one byte of scratch too few (the dispatcher then skips both long forms), and 64 query heads per kv head
    # (declined by both long forms: r2 > 32): the one-launch kernel k_attn_dec
    "flash": [("flash",) + c for c in FLASH_CASES] + [("short_ws", 128, 8, 2, 0, 1024, 600, 0), ("random", 64, 64, 1, 0, 1024, 600, 0)],
    # CLLM_ATTN_LONG_3=1: the three launches at an aligned ML (the n_kv of N3 that fit 1024 positions)
    "three": [("random", 128, 8, 2, 0, 1024, n, 0) for n in N3 if n <= 1024],
    # CLLM_ATTN_LONG=64: nch 2 .. 16, one or no whole chunk per lane group, most score workgroups return at i_lo >= n_kv
    "thr64": [("random", 128, 8, 2, 0, 512, n, 0) for n in (65, 96, 97, 127, 512)],
    "default": [("random", 128, 8, 2, 0, 1032, n, 0) for n in N3]                       # ML % 32 == 8: the three-launch form
               + [("random", 128, 8, 2, 0, 1024, n, 0) for n in N3 if n <= 1024]        # the fused form on the inputs of "three"
               + [("random", 128, 8, 2, 0, ML, n, 0) for ML, n in ((1056, 1056), (1056, 1055), (2048, 2048), (2048, 2017), (4096, 2560))]
               + INSTANCES,
}
case_key = lambda c: "-".join(str(v) for v in c)


def case_inputs(case):
    """-> qkv, kc0, vc0 of a case of CASE_LISTS"""
    kind, hd, nh, nkv, mode, ML, n_kv, extra = case
    if kind == "flash":
        d = flash_case_inputs(case[1:])
        return d["qkv"], d["kc0"], d["vc0"]
    if kind in ("boundary", "boundary_nt"):
        d = boundary_attn_case((hd, nh, nkv, ML, n_kv - 1, mode))
        return d["qkv"], d["kc0"], d["vc0"]
    return random_case(hd, nh, nkv, mode, ML, n_kv, extra)


BOUNDARY_ATTN = [(128, 8, 2, 1024, 299, 0), (128, 8, 2, 1024, 499, 0), (128, 8, 2, 1024, 776, 0), (128, 8, 2, 1032, 776, 0)]      # (hd, nh, nkv, ML, n_past, mode)


@functools.lru_cache(maxsize=None)
def boundary_attn_case(shape):
    return attn_boundary_case(*shape, np.random.default_rng(list(shape)))


CASE_LISTS["default"] += [("boundary", hd, nh, nkv, mode, ML, n_past + 1, 0) for hd, nh, nkv, ML, n_past, mode in BOUNDARY_ATTN]
CASE_LISTS["default"] += [("boundary_nt", hd, nh, nkv, mode, ML, n_past + 1, 0) for hd, nh, nkv, ML, n_past, mode in BOUNDARY_ATTN[:2]]
