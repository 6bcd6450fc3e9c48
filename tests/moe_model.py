"""The sparse-MoE path of one token and of a prompt: the launch plans, the oracle chains and the case lists the CPU model tests (test_moe_model.py) and the GPU tests
(test_gpu_moe.py) share.  Plain numpy and the CPU oracle: no GPU, no package import.

1. plan_*(): the geometry arithmetic of the launchers restated as pure functions of (wtype, K, rows, slots | k, epi, n_cu) -> Plan(grid, kfull, nrem, npre, capped),
   None where the launcher returns CLLM_E_UNSUPPORTED:  launch_gemv_decode_id (gemv_decode.hip), launch_gemv_decode_id_combine / launch_gemv_decode_id_router_silu /
   launch_moe_router (gemv_moe.hip), launch_mmvq_id (mmvq.hip, CLLM_MMVQ_WG 256 / CLLM_MMVQ_OCC 8: the defaults of options.def), launch_gemv_kq_id (gemv_kq.hip);
   mul_mat_id_path(): which of them cllm_op_mul_mat_id (capi.hip) ends in.
   What the restatement shows about the documented refusals: K <= 32768 keeps every LDS sum below the 160 KB - 256 the launchers allow (the largest, the combine's two activation rows of a 32-weight
   format at K 32768, is 129280 bytes), so the LDS refusals of the decode forms cannot be reached: the K bound refuses first (test_moe_model.py asserts this).
2. ref_*(): every fused form node by node on the oracle, in GenericSparseMLP::forward's order.
3. the case lists: every entry says in `want` what geometry it is there for; test_moe_model.py holds each to it at 256 and at 64 compute units.
"""
import collections
import functools
import zlib

import numpy as np

import oracle as O
from synth_helpers import rand_blocks

f32 = np.float32
EPS = 1e-5
TUNED = (O.Q4_K, O.Q8_0, O.Q4_0, O.Q4_1)
COVERAGE = (O.Q5_K, O.Q6_K, O.Q2_K, O.Q3_K, O.Q5_0, O.Q5_1, O.IQ4_NL, O.MXFP4, O.IQ4_XS, O.TQ1_0, O.TQ2_0, O.IQ2_XXS, O.IQ2_XS, O.IQ2_S, O.IQ3_XXS, O.IQ3_S, O.IQ1_S, O.IQ1_M)
ALL_TYPES = TUNED + COVERAGE
TYPE_NAME = {O.Q4_K: "q4_K", O.Q8_0: "q8_0", O.Q4_0: "q4_0", O.Q4_1: "q4_1", O.Q5_K: "q5_K", O.Q6_K: "q6_K", O.Q2_K: "q2_K", O.Q3_K: "q3_K", O.Q5_0: "q5_0", O.Q5_1: "q5_1",
             O.IQ4_NL: "iq4_nl", O.MXFP4: "mxfp4", O.IQ4_XS: "iq4_xs", O.TQ1_0: "tq1_0", O.TQ2_0: "tq2_0", O.IQ2_XXS: "iq2_xxs", O.IQ2_XS: "iq2_xs", O.IQ2_S: "iq2_s",
             O.IQ3_XXS: "iq3_xxs", O.IQ3_S: "iq3_s", O.IQ1_S: "iq1_s", O.IQ1_M: "iq1_m"}
N_CU_MODEL = 256                                  # what the CPU tests plan with (the GPU tests ask cllm_device_info)
MAX_PAIRS = 65535                                 # (slot, token) pairs of one multi-token MUL_MAT_ID: the grid's y extent


# ---- (1) the plans ----------------------------------------------------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "grid kfull nrem npre capped")
LDS_MAX = 160 * 1024                              # a CU's LDS: what mmvq.hip compares with
DEC_LDS_MAX = 160 * 1024 - 256                    # K_GEMV_DEC_MAX_DYN_LDS (gemv_decode_kernel.h): the k_gemv_dec launchers leave room for the norm prologues' static LDS
Q4K_CHAIN_BYTES = 8 * 192 + 64                    # q4k.h
Q32_CHAIN_BYTES = 9 * 272 + 512                   # q32.h
MMVQ_WG, MMVQ_OCC = 256, 8                        # options.def


def _a16(x):
    return (x + 15) & ~15


def act_row_bytes(K, kind):
    """common.h: qs[K] | d[K / kind] | s[K / 32], every plane 16-byte aligned"""
    return _a16(K) + _a16(K // kind * 4) + _a16(K // 32 * 4)


def _kind(t):
    return 256 if t == O.Q4_K else 32


def _chain(t):
    return Q4K_CHAIN_BYTES if t == O.Q4_K else Q32_CHAIN_BYTES


def npre_of(K):
    return 1 if K <= 4096 else 4 if K <= 16384 else 8


def _rows_too_many(t, K, nrows):
    return nrows * O.row_size(t, K) >= 1 << 32


def _deal(units, cap):
    grid = (units + 15) // 16
    capped = grid > cap
    grid = min(grid, cap)
    return grid, units // (grid * 16), units % (grid * 16), capped


def plan_decode_id(t, K, nrows, n_slots, epi, n_cu):
    """launch_gemv_decode_id: MUL_MAT_ID of one token, slot = blockIdx.y; epi 1: gate / up row pairs, a unit = one feature"""
    kind = _kind(t)
    if t not in TUNED or K % kind or K > 32768 or nrows <= 0 or n_slots < 1 or n_slots > 64 or _rows_too_many(t, K, nrows):
        return None
    if act_row_bytes(K, kind) + 16 * Q32_CHAIN_BYTES > DEC_LDS_MAX:
        return None
    if epi != 0 and (epi != 1 or nrows % 2 or (nrows // 2) % 8):
        return None
    units = nrows // 2 if epi == 1 else nrows
    g = _deal(units, max(n_cu // n_slots, 1))
    return Plan(*g[:3], npre_of(K), g[3])


def plan_combine(t, K, nrows, n_cu, n_used=2):
    """cllm_op_mul_mat_id_combine -> launch_gemv_decode_id_combine: two slots, a unit = the two experts' row r; no slot division of the grid"""
    kind = _kind(t)
    if n_used != 2 or t not in TUNED or K % kind or K > 32768 or nrows <= 0 or _rows_too_many(t, K, nrows):
        return None
    if 2 * act_row_bytes(K, kind) + 16 * Q32_CHAIN_BYTES > DEC_LDS_MAX:
        return None
    g = _deal(nrows, n_cu)
    return Plan(*g[:3], npre_of(K), g[3])


def plan_router(t, K, ne, k):
    """launch_moe_router: one workgroup, a unit = one expert's router row"""
    kind = _kind(t)
    if t not in TUNED or K % kind or K % 4 or K > 16384 or ne < 1 or ne > 64 or k < 1 or k > ne:
        return None
    if act_row_bytes(K, kind) + 16 * Q32_CHAIN_BYTES > DEC_LDS_MAX:
        return None
    return Plan(1, ne // 16, ne % 16, 1 if K <= 4096 else 4, False)


def plan_router_silu(t, K, nrows, ne, k, n_cu):
    """launch_gemv_decode_id_router_silu: the router redone by every workgroup, then slot blockIdx.y < k of the gate / up pack (nrows = 2 F)"""
    kind = _kind(t)
    if t not in TUNED or K % kind or K % 4 or K > 16384 or ne < 1 or ne > 64 or k < 1 or k > ne or nrows <= 0 or nrows % 2 or (nrows // 2) % 8 or _rows_too_many(t, K, nrows):
        return None
    if act_row_bytes(K, kind) + 16 * Q32_CHAIN_BYTES + 3 * 64 * 4 > DEC_LDS_MAX:
        return None
    g = _deal(nrows // 2, max(n_cu // k, 1))
    return Plan(*g[:3], 1 if K <= 4096 else 4, g[3])


def plan_mmvq_id(t, K, nrows, n_used, n_tok, n_cu):
    """launch_mmvq_id -> launch_one: 4 waves per workgroup, one grid slice per (slot, token), the grid capped at 8 workgroups per CU over all slices; npre 0: no prologue"""
    kind, wpw = _kind(t), MMVQ_WG // 64
    if t not in TUNED or K % kind or act_row_bytes(K, kind) > LDS_MAX or n_used * n_tok > MAX_PAIRS or n_used * n_tok < 1:
        return None
    if act_row_bytes(K, kind) + wpw * _chain(t) > LDS_MAX:
        return None
    grid = (nrows + wpw - 1) // wpw
    cap = max(n_cu * MMVQ_OCC // (n_used * n_tok), 1)
    capped, grid = grid > cap, min(grid, cap)
    return Plan(grid, nrows // (grid * wpw), nrows % (grid * wpw), 0, capped)


def plan_kq_id(t, K, nrows, n_used, n_tok):
    """launch_gemv_kq_id: 8 lanes per row, 32 rows per workgroup, no cap: every row has its lanes (kfull 0, nrem = the rows of the last workgroup)"""
    if t not in COVERAGE or K % O.BLCK[t] or nrows <= 0 or nrows > 1 << 28 or n_used <= 0 or n_used * n_tok > MAX_PAIRS:
        return None
    return Plan((nrows * 8 + 255) // 256, 0, nrows % 32, 0, False)


def expert_stride_ok(t, K, nrows, pad=0):
    """the one-token entry points take expert matrices a multiple of 16 bytes apart (capi.hip: as->nb[2] % 16), dense ones included"""
    return (nrows * O.row_size(t, K) + pad) % 16 == 0


def mul_mat_id_path(t, K, nrows, n_used, n_tok, n_cu, w_pad=0):
    """-> (name, Plan) of the launcher cllm_op_mul_mat_id ends in for dense or 16-byte padded b / dst; (None, None): an error"""
    if n_tok == 1 and t in TUNED and expert_stride_ok(t, K, nrows, w_pad):
        p = plan_decode_id(t, K, nrows, n_used, 0, n_cu)
        if p:
            return "decode_id", p
    if t in COVERAGE:
        p = plan_kq_id(t, K, nrows, n_used, n_tok)
        return ("kq_id", p) if p else (None, None)
    p = plan_mmvq_id(t, K, nrows, n_used, n_tok, n_cu)
    return ("mmvq_id", p) if p else (None, None)


def dealt_units(grid, kfull, nrem, waves=16):
    """the units k_gemv_dec's waves take under (grid, kfull, nrem), as the kernel deals them (gemv_decode_kernel.h): in a full round wave (b, w) takes unit
    round * nwaves + 16 b + w, the last, partial round is dealt workgroup-interleaved (w * grid + b) -> the sorted list of every unit some wave computes and stores"""
    nwaves, out = grid * waves, []
    for b in range(grid):
        for w in range(waves):
            lin, alt = b * waves + w, w * grid + b
            nmine = kfull + (1 if alt < nrem else 0)
            out += [k * nwaves + (lin if k < kfull else alt) for k in range(nmine)]
    return sorted(out)


class Want(dict):
    """what a case is there for; never changed after the case list is built, so it may sit in a hashable case"""
    def __hash__(self):
        return hash(tuple(sorted((k, str(v)) for k, v in self.items())))


def holds(plan, want):
    """does a Plan have what a case's `want` names?  keys: kfull (exact), kfull_ge, nrem (exact), nrem_ne0, nrem_mod16_ne0, npre, capped, grid"""
    if plan is None:
        return False
    ok = True
    for key, v in want.items():
        if key == "kfull":
            ok &= plan.kfull == v
        elif key == "kfull_ge":
            ok &= plan.kfull >= v
        elif key == "nrem":
            ok &= plan.nrem == v
        elif key == "nrem_ne0":
            ok &= plan.nrem != 0
        elif key == "nrem_mod16_ne0":
            ok &= plan.nrem % 16 != 0
        elif key in ("npre", "capped", "grid"):
            ok &= getattr(plan, key) == v
        elif key not in ("path", "fused"):
            raise KeyError(key)
    return bool(ok)


# ---- (2) the oracle chains ----------------------------------------------------------------------------------------------------------------
def _t(a, ne, nb=None, offset=0):
    return O.tensor(a, O.I32 if a.dtype == np.int32 else O.F32, ne, nb, offset)


def ref_mul_mat_id(t, N, w, x, ids):
    """w: the blocks of [K, N, E] (uint8 [E * N, row bytes]), x f32 [T, 1 | U, K], ids i32 [T, U] -> f32 [T, U, N]"""
    x, ids = np.ascontiguousarray(x, f32), np.ascontiguousarray(ids, np.int32)
    (T, nb1, K), U = x.shape, ids.shape[1]
    out = np.zeros((T, U, N), f32)
    O.mul_mat_id(O.tensor(w, t, [K, N, w.size // O.row_size(t, K) // N]), _t(x, [K, nb1, T]), _t(ids, [U, T]), _t(out, [N, U, T]))
    return out


mmid = ref_mul_mat_id


def ref_silu_mul(t, F, wg, wu, x, ids):
    """MUL_MAT_ID(gate), MUL_MAT_ID(up), SILU, MUL (MultiMLP::forward) -> f32 [T, U, F]"""
    g, u = mmid(t, F, wg, x, ids), mmid(t, F, wu, x, ids)
    s, out = np.zeros_like(g), np.zeros_like(g)
    ne = [F, g.shape[1], g.shape[0]]
    O.silu(_t(g, ne), _t(s, ne))
    O.mul(_t(s, ne), _t(u, ne), _t(out, ne))
    return out


def ref_router(t, wr, x, gw, k, eps=EPS):
    """RMS_NORM, MUL, MUL_MAT(router), SOFT_MAX, TOP_K of one token -> xnorm [K], probs [E], ids [k], logits [E]"""
    x, gw = np.ascontiguousarray(x, f32).reshape(-1), np.ascontiguousarray(gw, f32).reshape(-1)
    K = x.size
    E = wr.size // O.row_size(t, K)
    n1, xn, lg, pr, ids = np.zeros(K, f32), np.zeros(K, f32), np.zeros(E, f32), np.zeros(E, f32), np.zeros(k, np.int32)
    O.rms_norm(_t(x, [K]), _t(n1, [K]), eps)
    O.mul(_t(n1, [K]), _t(gw, [K]), _t(xn, [K]))
    O.mul_mat(O.tensor(wr, t, [K, E]), _t(xn, [K]), _t(lg, [E]))
    O.soft_max(_t(lg, [E]), None, _t(pr, [E]))
    O.top_k(_t(pr, [E]), _t(ids, [k]))
    return xn, pr, ids, lg


def ref_combine(experts, probs, ids, resid=None):
    """GET_ROWS(probs, ids), SUM_ROWS, DIV, MUL, ADD of the slot views in slot order (, ADD of the residual): experts f32 [T, k, H], probs [T, E], ids [T, k],
    resid [T, H] -> [T, H].  One DIV per slot by the float sum; the slot sum starts from slot 0's product (no zero in front)"""
    experts, probs, ids = np.ascontiguousarray(experts, f32), np.ascontiguousarray(probs, f32), np.ascontiguousarray(ids, np.int32)
    (T, k, H), E = experts.shape, probs.shape[1]
    w, s, wn, y = np.zeros((T, k, 1), f32), np.zeros((T, 1), f32), np.zeros((T, k), f32), np.zeros_like(experts)
    O.get_rows(_t(probs, [1, E, T]), _t(ids, [k, T]), _t(w, [1, k, T]))
    O.sum_rows(_t(w, [k, T]), _t(s, [1, T]))
    O.div(_t(w, [k, T]), _t(s, [1, T]), _t(wn, [k, T]))
    O.mul(_t(experts, [H, k, T]), _t(wn, [1, k, T]), _t(y, [H, k, T]))
    acc = np.ascontiguousarray(y[:, 0])
    for j in range(1, k):
        nxt = np.zeros((T, H), f32)
        O.add(_t(acc, [H, T]), _t(y, [H, T], nb=[4, 4 * H * k, 4 * H * k * T], offset=4 * H * j), _t(nxt, [H, T]))
        acc = nxt
    if resid is not None:
        nxt = np.zeros((T, H), f32)
        O.add(_t(acc, [H, T]), _t(np.ascontiguousarray(resid, f32), [H, T]), _t(nxt, [H, T]))
        acc = nxt
    return acc


def ref_block(t, F, wr, wg, wu, wd, x, gw, k, eps=EPS):
    """one token's whole sparse-MoE block on the residual stream x [K]: router, gate / up / SiLU / MUL of the k picked experts, down + combine + residual.
    -> dict of every intermediate; out [K] is what the block leaves in place of x"""
    K = x.size
    xn, pr, ids, lg = ref_router(t, wr, x, gw, k, eps)
    g = ref_silu_mul(t, F, wg, wu, xn.reshape(1, 1, K), ids.reshape(1, k))                  # [1, k, F]
    d = mmid(t, K, wd, g, ids.reshape(1, k))                                               # [1, k, K]
    out = ref_combine(d, pr.reshape(1, -1), ids.reshape(1, k), np.asarray(x, f32).reshape(1, K))
    return {"xnorm": xn, "logits": lg, "probs": pr, "ids": ids, "g": g[0], "down": d[0], "out": out[0]}


def router_weights(t, E, K, rng, x, gw):
    """router rows whose logits over (x, gw) have a spread of about 2: a soft-max with every probability a normal float, none of them negligible.  The quants are drawn
    once; the fp16 block scales are redrawn at the size the first draw's logits ask for"""
    state = rng.bit_generator.state
    lg = ref_router(t, rand_blocks(t, E, K, rng, d_scale=0.01), x, gw, 1)[3]
    rng.bit_generator.state = state
    return rand_blocks(t, E, K, rng, d_scale=0.01 * 2.0 / max(float(np.std(lg.astype(np.float64))), 1e-3))


def interleave_rows(wg, wu, E):
    """the per-expert gate / up pack cllm_pack_rows(interleave) makes on the device: rows 2u = gate_u, 2u + 1 = up_u inside every expert"""
    F, rs = wg.shape[0] // E, wg.shape[1]
    p = np.zeros((E, F, 2, rs), np.uint8)
    p[:, :, 0], p[:, :, 1] = wg.reshape(E, F, rs), wu.reshape(E, F, rs)
    return p.reshape(E * 2 * F, rs)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _blk(t, mult32, mult256=1):
    """a K of `mult` blocks: 256-weight types count super-blocks"""
    return 256 * mult256 if O.BLCK[t] == 256 else 32 * mult32


# ---- (3a) one token: cllm_op_mul_mat_id (epi 0) and cllm_op_mul_mat_id_silu_mul (epi 1) ----------------------------------------------------
#   N: rows of an expert (epi 1: FEATURES; the pack has 2 N rows);  b: "bcast" ne[1] = 1 | "slot" one row per slot | "slot_pad" rows 4 K + 64 bytes apart;
#   dst_pad: floats between the slots' rows of dst (sentinel);  w_pad: bytes between experts (nb[2] = N * row size + w_pad);  ids: "rand" | "same" | "edges"
#   want: path "decode_id" (the fused one-token kernel) | "mmvq_id" (the general path) | "nodes" (the fused entry refuses: the caller's node sequence), + holds() keys
OneTok = collections.namedtuple("OneTok", "name t K N E U epi b dst_pad w_pad ids want")


def _one(name, t, K, N, E, U, epi=0, b="slot", dst_pad=0, w_pad=0, ids="rand", **want):
    want.setdefault("path", "decode_id")
    return OneTok(f"{name}-{TYPE_NAME[t]}-K{K}-N{N}-E{E}-U{U}-epi{epi}", t, K, N, E, U, epi, b, dst_pad, w_pad, ids, Want(want))


def _one_tok_cases():
    c = []
    for i, t in enumerate(TUNED):
        k1 = _blk(t, 2)                                                             # one 256-block / two 32-blocks: NPRE 1
        # no full round, a ragged last one; b broadcast or per slot; ids on the first and the last expert
        c.append(_one("kfull0", t, k1, 40, 8, 2, b="bcast", ids="edges", kfull=0, nrem=40, nrem_mod16_ne0=True, npre=1, capped=False))
        c.append(_one("kfull0", t, _blk(t, 3, 2), 104, 8, 3, b="slot_pad", ids="same", dst_pad=3, kfull=0, nrem=104, nrem_mod16_ne0=True, npre=1, capped=False))
        # 8 slots: cap = CUs / 8; two or more full rounds and 40 rows over (2 * 16 * 32 + 40 at 256 CUs); padded dst, padded expert stride
        c.append(_one("cap8", t, k1, 1064, 8, 8, dst_pad=(5, 0, 1, 8)[i], w_pad=(0, 48, 16, 0)[i], kfull_ge=2, nrem_ne0=True, npre=1, capped=True))
        c.append(_one("cap8", t, k1, 1064, 8, 8, epi=1, b="bcast", dst_pad=(0, 7, 0, 2)[i], w_pad=(32, 0, 0, 16)[i], kfull_ge=2, nrem_ne0=True, npre=1, capped=True))
        # NPRE 4 / 8: the smallest K above 4096 / 16384; the largest K, and one block more (the general path)
        c.append(_one("npre4", t, 4096 + O.BLCK[t], 40, 4, 2, b="bcast", kfull=0, nrem=40, npre=4))
        c.append(_one("npre4", t, 4096 + O.BLCK[t], 24, 4, 2, epi=1, kfull=0, nrem=24, npre=4))
        c.append(_one("npre8", t, 16384 + O.BLCK[t], 24, 2, 2, ids="edges", kfull=0, nrem=24, npre=8))
        c.append(_one("npre8", t, 16384 + O.BLCK[t], 8, 2, 2, epi=1, b="bcast", kfull=0, nrem=8, npre=8))
        c.append(_one("kmax", t, 32768, 24, 2, 2, b=("bcast", "slot", "slot_pad", "slot")[i], kfull=0, nrem=24, npre=8))
        c.append(_one("kover", t, 32768 + O.BLCK[t], 24, 2, 2, path="mmvq_id"))
        c.append(_one("kover", t, 32768 + O.BLCK[t], 8, 2, 2, epi=1, path="nodes"))
    # the slot counts: cap = CUs / n_slots, every one with a full round and a remainder; 65 slots: the general path
    c.append(_one("slots", O.Q4_K, 256, 4136, 2, 1, kfull_ge=1, nrem=40, npre=1, capped=True))
    c.append(_one("slots", O.Q8_0, 64, 2088, 4, 2, b="bcast", kfull_ge=1, nrem=40, npre=1, capped=True))
    c.append(_one("slots", O.Q4_0, 64, 1400, 8, 3, dst_pad=8, kfull_ge=1, nrem_ne0=True, npre=1, capped=True))
    c.append(_one("slots", O.Q4_1, 64, 104, 8, 64, b="slot_pad", w_pad=16, kfull_ge=1, nrem_ne0=True, npre=1, capped=True))
    c.append(_one("slots", O.Q4_K, 256, 104, 8, 64, b="bcast", kfull_ge=1, nrem_ne0=True, npre=1, capped=True))
    c.append(_one("slots", O.Q4_0, 64, 104, 8, 64, epi=1, b="bcast", kfull_ge=1, nrem_ne0=True, npre=1, capped=True))
    c.append(_one("slots", O.Q4_K, 256, 104, 8, 65, b="bcast", path="mmvq_id"))
    c.append(_one("slots", O.Q4_0, 64, 104, 8, 65, dst_pad=4, path="mmvq_id"))
    c.append(_one("slots", O.Q8_0, 64, 104, 8, 65, epi=1, path="nodes"))
    # epi 1 with features that are no multiple of 8: the fused entry refuses (the SiLU tail is libm's), the four nodes match
    c.append(_one("f20", O.Q4_K, 256, 20, 4, 2, epi=1, path="nodes"))
    c.append(_one("f20", O.Q8_0, 64, 20, 4, 2, epi=1, b="bcast", path="nodes"))
    return c


ONE_TOK = _one_tok_cases()


def pick_ids(kind, E, U, rng, T=1):
    if kind == "same":
        return np.full((T, U), min(3, E - 1), np.int32)
    ids = rng.integers(0, E, (T, U)).astype(np.int32)
    if kind == "edges":
        ids[:, 0], ids[:, -1] = E - 1, 0
        if U == 1:
            ids[:, 0] = E - 1
    return ids


@functools.lru_cache(maxsize=None)
def one_tok_data(case):
    """-> dict w (epi 0) | wg, wu, w (epi 1: w the interleaved pack), x [1, 1 | U, K], ids [1, U], want [1, U, N].  Computed once, read-only"""
    c, rng = case, _rng(case.name)
    x = rng.standard_normal((1, 1 if c.b == "bcast" else c.U, c.K)).astype(f32)
    ids = pick_ids(c.ids, c.E, c.U, rng)
    if c.epi == 0:
        w = rand_blocks(c.t, c.N * c.E, c.K, rng)
        return _frozen({"w": w, "x": x, "ids": ids, "want": mmid(c.t, c.N, w, x, ids)})
    wg, wu = rand_blocks(c.t, c.N * c.E, c.K, rng), rand_blocks(c.t, c.N * c.E, c.K, rng)
    return _frozen({"wg": wg, "wu": wu, "w": interleave_rows(wg, wu, c.E), "x": x, "ids": ids, "want": ref_silu_mul(c.t, c.N, wg, wu, x, ids)})


def one_tok_plan(c, n_cu):
    """-> (path, Plan): what the case's entry point does with it"""
    if c.epi == 1:
        p = plan_decode_id(c.t, c.K, 2 * c.N, c.U, 1, n_cu) if expert_stride_ok(c.t, c.K, 2 * c.N, c.w_pad) else None
        return ("decode_id", p) if p else ("nodes", None)
    return mul_mat_id_path(c.t, c.K, c.N, c.U, 1, n_cu, c.w_pad)


# ---- (3b) cllm_op_mul_mat_id_combine (and cllm_op_moe_combine behind the refusals) ------------------------------------------------------------
#   ids: "top2" TOP_K of the probabilities | "same" both slots one expert | "edges";  probs: "soft" a soft-max row | "binades" the two picked ones 2^20 apart;
#   resid: "none" | "yes" | "inplace";  U: slots (2: the fused launch; 1, 4, 8: refused, nothing written, the two calls match)
Comb = collections.namedtuple("Comb", "name t K H E U ids probs resid want")


def _comb(name, t, K, H, E, U=2, ids="top2", probs="soft", resid="yes", **want):
    want.setdefault("fused", True)
    return Comb(f"{name}-{TYPE_NAME[t]}-K{K}-H{H}-E{E}-U{U}-{ids}-{probs}-{resid}", t, K, H, E, U, ids, probs, resid, Want(want))


def _comb_cases():
    c = []
    for i, t in enumerate(TUNED):
        k1 = _blk(t, 2)
        c.append(_comb("npre1", t, k1, 40, 8, ids="same", resid=("yes", "none", "inplace", "yes")[i], kfull=0, nrem=40, npre=1))
        c.append(_comb("binades", t, _blk(t, 3, 2), 104, 8, probs="binades", resid=("inplace", "yes", "none", "inplace")[i], kfull=0, nrem=104, npre=1))
        c.append(_comb("npre4", t, 4096 + O.BLCK[t], 40, 4, resid=("none", "inplace", "yes", "none")[i], kfull=0, nrem=40, npre=4))
        c.append(_comb("npre8", t, 16384 + O.BLCK[t], 24, 3, ids="edges", resid="inplace", kfull=0, nrem=24, npre=8))
        c.append(_comb("kmax", t, 32768, 24, 2, probs="binades", kfull=0, nrem=24, npre=8))
        c.append(_comb("kover", t, 32768 + O.BLCK[t], 24, 2, fused=False))
        # H: every CU's 16 waves take one full round or more, 40 rows over
        c.append(_comb("rounds", t, k1, 4136, 4, resid=("inplace", "none", "yes", "inplace")[i], kfull_ge=1, nrem=40, npre=1, capped=True))
    for U, t in ((1, O.Q4_K), (4, O.Q8_0), (8, O.Q4_0), (4, O.Q4_1)):
        c.append(_comb("slots", t, _blk(t, 2), 72, 8, U=U, resid="yes" if U != 4 else "inplace", fused=False))
    return c


COMBINE = _comb_cases()


def sum_rounding_shows(p0, p1):
    """SUM_ROWS rounds p0 + p1 to float before DIV: does one of the two weights differ from the quotient by the double sum?"""
    s = np.float64(p0) + np.float64(p1)
    return bool(f32(p0 / f32(s)) != f32(np.float64(p0) / s) or f32(p1 / f32(s)) != f32(np.float64(p1) / s))


def soft_row(rng, E):
    p = rng.standard_normal(E).astype(np.float64)
    return (np.exp(p) / np.exp(p).sum()).astype(f32)


@functools.lru_cache(maxsize=None)
def combine_data(case):
    """-> dict w [E * H rows], x [1, U, K], probs [1, E], ids [1, U], resid [1, H] | None, down [1, U, H] (MUL_MAT_ID alone), want [1, H]"""
    c, rng = case, _rng(case.name)
    w = rand_blocks(c.t, c.H * c.E, c.K, rng)
    x = rng.standard_normal((1, c.U, c.K)).astype(f32)
    pr = soft_row(rng, c.E).reshape(1, c.E)
    if c.ids == "top2":
        ids = np.zeros((1, c.U), np.int32)
        O.top_k(_t(pr, [c.E, 1]), _t(ids, [c.U, 1]))
    else:
        ids = pick_ids(c.ids, c.E, c.U, rng)
    if c.probs == "binades":                              # w_1 = p_1 / (p_0 + p_1) ~ 2^-20: the float sum p_0 + p_1 loses p_1's low bits, the division shows which sum was taken
        if ids[0, 0] == ids[0, -1]:
            raise ValueError("binades needs two experts")
        p0, p1 = f32(0.62109375 + 2.0 ** -22), f32(1.3718 * 2.0 ** -20)
        while not sum_rounding_shows(p0, p1):               # the next float, until a weight computed with the unrounded double sum has other bits
            p1 = np.nextafter(p1, f32(1.0))
        pr[0, ids[0, 0]], pr[0, ids[0, -1]] = p0, p1
    resid = None if c.resid == "none" else rng.standard_normal((1, c.H)).astype(f32)
    down = mmid(c.t, c.H, w, x, ids)
    return _frozen({"w": w, "x": x, "probs": pr, "ids": ids, "resid": resid, "down": down, "want": ref_combine(down, pr, ids, resid)})


# ---- (3c) cllm_op_moe_router and cllm_op_moe_router_gate_up --------------------------------------------------------------------------------
#   F: the experts' features of the gate / up launch (0: the router alone);  ties: router rows duplicated, so that equal probabilities meet TOP_K's lower-index-first rule
Rout = collections.namedtuple("Rout", "name t K E k F ties want")


def _rout(name, t, K, E, k, F=16, ties=False, **want):
    want.setdefault("fused", True)
    return Rout(f"{name}-{TYPE_NAME[t]}-K{K}-E{E}-k{k}-F{F}{'-ties' if ties else ''}", t, K, E, k, F, ties, Want(want))


def _router_cases():
    c = []
    shapes = [(2, 1), (2, 2), (7, 2), (7, 7), (16, 8), (16, 16), (33, 1), (33, 8), (33, 33), (64, 2), (64, 8), (64, 64)]
    for i, (E, k) in enumerate(shapes):
        t = TUNED[i % 4]
        c.append(_rout("experts", t, _blk(t, 2), E, k, F=24 if k < 33 else 8, ties=E >= 7 and i % 2 == 0, npre=1))
    for t in TUNED:
        c.append(_rout("npre4", t, 4096 + O.BLCK[t], 8, 2, F=24, ties=t in (O.Q4_K, O.Q4_0), kfull=0, nrem=24, npre=4))
        c.append(_rout("kmax", t, 16384, 7, 2, F=8, kfull=0, nrem=8, npre=4))
        c.append(_rout("kover", t, 16384 + O.BLCK[t], 8, 2, F=8, fused=False))
        # k = 8 slots: cap = CUs / 8 workgroups per slot; two or more full rounds of features and 40 over
        c.append(_rout("cap8", t, _blk(t, 2), 8, 8, F=1064, kfull_ge=2, nrem_ne0=True, npre=1, capped=True))
    c.append(_rout("e65", O.Q4_K, 256, 65, 2, fused=False))
    c.append(_rout("e65", O.Q8_0, 64, 65, 8, fused=False))
    c.append(_rout("f20", O.Q4_0, 64, 8, 2, F=20, fused=False))               # the router alone still runs fused; the gate / up launch refuses features % 8
    return c


ROUTER = _router_cases()


@functools.lru_cache(maxsize=None)
def router_data(case):
    """-> dict wr [E rows], wg, wu [E * F rows], x [K], gw [K], and the oracle's xnorm, probs, ids, logits, g [k, F]"""
    c, rng = case, _rng(case.name)
    x, gw = (rng.standard_normal(c.K) * 1.7).astype(f32), (1.0 + 0.1 * rng.standard_normal(c.K)).astype(f32)
    wr = router_weights(c.t, c.E, c.K, rng, x, gw)
    if c.ties:                                            # equal rows -> equal logits -> equal probabilities, bit for bit
        wr[c.E - 2], wr[c.E // 2] = wr[1], wr[0]
    wg, wu = rand_blocks(c.t, c.F * c.E, c.K, rng), rand_blocks(c.t, c.F * c.E, c.K, rng)
    k_ref = min(c.k, c.E)
    xn, pr, ids, lg = ref_router(c.t, wr, x, gw, k_ref)
    g = ref_silu_mul(c.t, c.F, wg, wu, xn.reshape(1, 1, c.K), ids.reshape(1, k_ref))[0]
    return _frozen({"wr": wr, "wg": wg, "wu": wu, "x": x, "gw": gw, "xnorm": xn, "probs": pr, "ids": ids, "logits": lg, "g": g})


# ---- (3d) many tokens: cllm_op_mul_mat_id through launch_mmvq_id (the tuned types) / launch_gemv_kq_id (the coverage types) -----------------------
#   b1: b.ne[1] (1 | U);  ids_pad: ints between the tokens' id rows;  dst_pad: (floats between slot rows, floats between tokens)
Multi = collections.namedtuple("Multi", "name t K N E U T b1 ids_pad dst_pad want")
# the wants hold at 256 and at 64 compute units alike (cap = 8 CUs / pairs: 62 | 15, 31 | 7, 7 | 1, 20 | 5, 10 | 2, 2 | 1, 6 | 1, 1 | 1 workgroups per pair)
MULTI_SHAPES = [                                                                    # (name, N, U, T, b1 per slot?, ids_pad, dst_pad, want of the tuned types)
    ("t33", 40, 1, 33, False, 0, (0, 0), dict(capped=False)),
    ("t33", 24, 2, 33, True, 3, (0, 0), dict(capped=False)),
    ("t33", 42, 8, 33, False, 0, (3, 5), dict(capped=True, nrem_ne0=True)),
    ("t100", 20, 1, 100, False, 1, (0, 0), dict(capped=False)),
    ("t100", 41, 2, 100, False, 2, (1, 7), dict(capped=True)),
    ("t100", 40, 8, 100, True, 0, (0, 0), dict(capped=True)),
    ("t40", 30, 8, 40, True, 0, (0, 0), dict(capped=True)),                          # 320 pairs: 6 workgroups per pair at 256 CUs
    ("cap1", 10, 8, 130, False, 0, (0, 2), dict(grid=1, kfull=2, nrem=2, capped=True)),      # 1040 pairs > 8 * 256 / 2: ONE workgroup of four waves walks the ten rows
]


def _multi_cases():
    c = []
    for t in ALL_TYPES:
        for name, N, U, T, per_slot, ids_pad, dst_pad, want in MULTI_SHAPES:
            K = _blk(t, 3)
            w = dict(want) if t in TUNED else {"nrem": N % 32}
            w["path"] = "mmvq_id" if t in TUNED else "kq_id"
            c.append(Multi(f"{name}-{TYPE_NAME[t]}-K{K}-N{N}-U{U}-T{T}-b{U if per_slot else 1}", t, K, N, 8, U, T, U if per_slot else 1, ids_pad, dst_pad, Want(w)))
    return c


MULTI = _multi_cases()
PAIRS_AT_LIMIT = Multi("pairs65535-q8_0-K32-N8-U3-T21845-b1", O.Q8_0, 32, 8, 4, 3, 21845, 1, 0, (0, 0), Want(path="mmvq_id", grid=1, kfull=2, nrem=0, capped=True))
PAIRS_OVER = Multi("pairs65536-q8_0-K32-N8-U2-T32768-b1", O.Q8_0, 32, 8, 4, 2, 32768, 1, 0, (0, 0), Want(path=None))


@functools.lru_cache(maxsize=None)
def multi_data(case):
    c, rng = case, _rng(case.name)
    w = rand_blocks(c.t, c.N * c.E, c.K, rng)
    x = rng.standard_normal((c.T, c.b1, c.K)).astype(f32)
    ids = pick_ids("rand", c.E, c.U, rng, c.T)
    ids[0, 0], ids[-1, -1] = c.E - 1, 0
    return _frozen({"w": w, "x": x, "ids": ids, "want": mmid(c.t, c.N, w, x, ids)})


# ---- (3e) one token's whole block ------------------------------------------------------------------------------------------------------------
Block = collections.namedtuple("Block", "name t K F E k")
BLOCKS = [Block("mixtral-width-q4_K-K4096-F1024-E8-k2", O.Q4_K, 4096, 1024, 8, 2), Block("small-q8_0-K128-F64-E4-k2", O.Q8_0, 128, 64, 4, 2)]


@functools.lru_cache(maxsize=None)
def block_data(case):
    """-> dict wr, wg, wu [E * F rows of K], wd [E * K rows of F], x, gw [K] and ref = ref_block(...)"""
    c, rng = case, _rng(case.name)
    x, gw = (rng.standard_normal(c.K) * 1.7).astype(f32), (1.0 + 0.1 * rng.standard_normal(c.K)).astype(f32)
    wr = router_weights(c.t, c.E, c.K, rng, x, gw)
    wg, wu, wd = rand_blocks(c.t, c.F * c.E, c.K, rng), rand_blocks(c.t, c.F * c.E, c.K, rng), rand_blocks(c.t, c.K * c.E, c.F, rng)
    d = {"wr": wr, "wg": wg, "wu": wu, "wd": wd, "x": x, "gw": gw}
    d["ref"] = _frozen(ref_block(c.t, c.F, wr, wg, wu, wd, x, gw, c.k))
    return _frozen(d)


# ---- host-side layouts for the GPU test: a dense [n2, n1, n0] array inside a sentinel-filled buffer with padded strides -------------------------
SENTINEL = 0xA5


def padded(a, pad1=0, pad2=0):
    """-> (buffer uint8, nb in bytes, mask bool: the bytes of the buffer that belong to the tensor).  a: [n2, n1, n0] of a 4-byte type; pad1 / pad2: elements between
    rows / after every plane; the padding holds SENTINEL"""
    n2, n1, n0 = a.shape
    row, plane = n0 + pad1, (n0 + pad1) * n1 + pad2
    buf = np.full((n2, plane), SENTINEL * 0x01010101, np.uint32)
    mask = np.zeros((n2, plane), bool)
    body = buf[:, :row * n1].reshape(n2, n1, row)
    body[:, :, :n0] = np.ascontiguousarray(a).view(np.uint32)
    mask[:, :row * n1].reshape(n2, n1, row)[:, :, :n0] = True
    return buf.reshape(-1).view(np.uint8), [4, 4 * row, 4 * plane, 4 * plane * n2], np.repeat(mask.reshape(-1), 4)


def padded_experts(w, E, pad):
    """expert matrices `pad` bytes apart -> (buffer uint8, nb[2])"""
    rows, rs = w.shape[0] // E, w.shape[1]
    buf = np.full((E, rows * rs + pad), SENTINEL, np.uint8)
    buf[:, :rows * rs] = w.reshape(E, rows * rs)
    return buf.reshape(-1), rows * rs + pad
