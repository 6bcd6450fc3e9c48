"""Why the GPU tests of the sparse-MoE kernels (test_gpu_moe.py) can be trusted (no GPU): every case of moe_model's lists has the launch geometry it is named for -- at
256 compute units and at 64, so no case leans on one device --, the plan functions give the launchers' numbers at shapes worked out by hand, the documented LDS refusals
sit behind the K bounds, the oracle chains have the node order of GenericSparseMLP::forward (an independent numpy restatement agrees bit for bit, a restatement with
another order does not), and, where the reference build is there, a whole block agrees with it node by node."""
import ctypes as C

import numpy as np
import pytest

import moe_model as M
import oracle as O

f32, f64 = np.float32, np.float64
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
name_of = lambda c: c.name  # noqa: E731
N_CUS = (M.N_CU_MODEL, 64)


def show(c, n_cu, path, p):
    print(f"\n{c.name} @ {n_cu} CUs: {path}" + (f" grid {p.grid} kfull {p.kfull} nrem {p.nrem} npre {p.npre} capped {p.capped}" if p else ""))


# ---- every case has the geometry it is there for ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cu", N_CUS)
@pytest.mark.parametrize("case", M.ONE_TOK, ids=name_of)
def test_one_token_case_geometry(case, n_cu):
    path, p = M.one_tok_plan(case, n_cu)
    show(case, n_cu, path, p)
    assert path == case.want["path"]
    if path == "decode_id":
        assert M.holds(p, case.want), (p, dict(case.want))
        units = case.N
        assert p.kfull * p.grid * 16 + p.nrem == units and p.nrem < p.grid * 16 and p.grid * case.U <= max(n_cu, case.U)
    # the layouts stay inside what the one-token entry points take: expert matrices a multiple of 16 bytes apart, padded or not
    assert M.expert_stride_ok(case.t, case.K, case.N * (2 if case.epi else 1), case.w_pad), "the case would go down the general path for its layout, not its shape"


@pytest.mark.parametrize("n_cu", N_CUS)
@pytest.mark.parametrize("case", M.COMBINE, ids=name_of)
def test_combine_case_geometry(case, n_cu):
    p = M.plan_combine(case.t, case.K, case.H, n_cu, case.U)
    show(case, n_cu, "fused" if p else "refused: the two calls", p)
    assert (p is not None) == case.want["fused"]
    if p:
        assert M.holds(p, case.want), (p, dict(case.want))
        assert p.kfull * p.grid * 16 + p.nrem == case.H
    assert M.expert_stride_ok(case.t, case.K, case.H)


@pytest.mark.parametrize("n_cu", N_CUS)
@pytest.mark.parametrize("case", M.ROUTER, ids=name_of)
def test_router_case_geometry(case, n_cu):
    p = M.plan_router_silu(case.t, case.K, 2 * case.F, case.E, case.k, n_cu)
    r = M.plan_router(case.t, case.K, case.E, case.k)
    show(case, n_cu, "fused" if p else "refused: the nodes", p)
    assert (p is not None) == case.want["fused"]
    if p:
        assert M.holds(p, case.want), (p, dict(case.want))
        assert r is not None and r.kfull * 16 + r.nrem == case.E and r.npre == p.npre
        assert M.expert_stride_ok(case.t, case.K, 2 * case.F)
    else:
        assert r is None or case.F % 8                      # the router alone refuses too, except where only the features are at fault
    if case.ties:
        d = M.router_data(case)
        pr = d["probs"].view(np.uint32)
        assert pr[case.E - 2] == pr[1] and pr[case.E // 2] == pr[0]


def test_router_ties_reach_the_picks():
    """a tied pair inside the k picked experts, or one in and one out: TOP_K's lower-index-first rule decides the ids"""
    inside = straddle = 0
    for c in M.ROUTER:
        if c.ties and c.want["fused"]:
            ids = set(M.router_data(c)["ids"].tolist())
            for a, b in ((1, c.E - 2), (0, c.E // 2)):
                inside += a in ids and b in ids
                straddle += (a in ids) != (b in ids)
                assert not (b in ids and a not in ids), c.name              # never the higher index alone
    print(f"\ntied pairs inside the picks: {inside}, split by the k-th pick: {straddle}")
    assert inside >= 4


@pytest.mark.parametrize("n_cu", N_CUS)
@pytest.mark.parametrize("case", M.MULTI + [M.PAIRS_AT_LIMIT, M.PAIRS_OVER], ids=name_of)
def test_many_token_case_geometry(case, n_cu):
    path, p = M.mul_mat_id_path(case.t, case.K, case.N, case.U, case.T, n_cu)
    show(case, n_cu, path, p)
    assert path == case.want["path"]
    if p is not None:
        assert M.holds(p, case.want), (p, dict(case.want))
    if case.name.startswith("cap1"):
        assert p.grid == 1 and (case.N % 4 if case.t in M.TUNED else case.N % 32)      # one workgroup walks every row; rows no multiple of its waves


def test_the_lists_cover_what_they_are_for():
    one = M.ONE_TOK
    for t in M.TUNED:
        for epi in (0, 1):
            mine = [c for c in one if c.t == t and c.epi == epi and c.want["path"] == "decode_id"]
            assert {c.want.get("npre") for c in mine} >= {1, 4, 8}
            assert any(c.want.get("kfull_ge", 0) >= 1 and (c.want.get("nrem_ne0") or c.want.get("nrem")) for c in mine)
            assert any(c.want["path"] != "decode_id" for c in one if c.t == t and c.epi == epi)
        comb = [c for c in M.COMBINE if c.t == t]
        assert {c.want.get("npre") for c in comb if c.want["fused"]} >= {1, 4, 8} and any(c.want.get("kfull_ge") for c in comb) and any(not c.want["fused"] for c in comb)
        assert {c.resid for c in comb} == {"none", "yes", "inplace"}
        rout = [c for c in M.ROUTER if c.t == t]
        assert {c.want.get("npre") for c in rout if c.want["fused"]} >= {1, 4} and any(c.want.get("kfull_ge") for c in rout) and any(not c.want["fused"] for c in rout)
    assert {c.U for c in one if c.epi == 0} >= {1, 2, 3, 8, 64, 65}
    assert {c.b for c in one} == {"bcast", "slot", "slot_pad"} and any(c.dst_pad for c in one) and any(c.w_pad for c in one) and {c.ids for c in one} == {"rand", "same", "edges"}
    assert {c.U for c in M.COMBINE if not c.want["fused"]} >= {1, 4, 8}
    assert {c.E for c in M.ROUTER} >= {2, 7, 16, 33, 64, 65} and {c.k for c in M.ROUTER} >= {1, 2, 8} and all(any(c.k == c.E == e for c in M.ROUTER) for e in (2, 7, 16, 33, 64))
    assert {c.t for c in M.MULTI} == set(M.ALL_TYPES) and len(M.ALL_TYPES) == 22
    assert {(c.T, c.U) for c in M.MULTI} >= {(33, 1), (33, 2), (33, 8), (100, 1), (100, 2), (100, 8), (40, 8)}
    assert M.PAIRS_AT_LIMIT.U * M.PAIRS_AT_LIMIT.T == 65535 and M.PAIRS_OVER.U * M.PAIRS_OVER.T == 65536


# ---- the plan functions against the launchers' arithmetic done by hand ------------------------------------------------------------------------
def test_plans_follow_the_launchers():
    Pl = M.Plan
    # Mixtral's gate / up of one token: 14336 features, 2 slots: cap 128 workgroups, 2048 waves, 7 full rounds
    assert M.plan_decode_id(O.Q4_K, 4096, 28672, 2, 1, 256) == Pl(128, 7, 0, 1, True)
    assert M.plan_router_silu(O.Q4_K, 4096, 28672, 8, 2, 256) == Pl(128, 7, 0, 1, True)
    assert M.plan_combine(O.Q4_K, 14336, 4096, 256) == Pl(256, 1, 0, 4, False)
    assert M.plan_decode_id(O.Q8_0, 64, 40, 2, 0, 256) == Pl(3, 0, 40, 1, False)
    assert M.plan_decode_id(O.Q8_0, 64, 1064, 8, 0, 256) == Pl(32, 2, 40, 1, True) and M.plan_decode_id(O.Q8_0, 64, 1064, 8, 0, 64) == Pl(8, 8, 40, 1, True)
    assert M.plan_decode_id(O.Q4_0, 64, 104, 64, 0, 256) == Pl(4, 1, 40, 1, True) and M.plan_decode_id(O.Q4_0, 64, 104, 65, 0, 256) is None
    assert M.plan_decode_id(O.Q4_0, 64, 104, 300, 0, 256) is None and M.plan_decode_id(O.Q4_0, 64, 104, 64, 0, 32) == Pl(1, 6, 8, 1, True)        # cap < 1 -> 1
    assert M.plan_decode_id(O.Q4_K, 4096, 8, 2, 0, 256).npre == 1 and M.plan_decode_id(O.Q4_K, 4352, 8, 2, 0, 256).npre == 4
    assert M.plan_decode_id(O.Q4_K, 16384, 8, 2, 0, 256).npre == 4 and M.plan_decode_id(O.Q4_K, 16640, 8, 2, 0, 256).npre == 8
    assert M.plan_decode_id(O.Q4_K, 32768, 8, 2, 0, 256).npre == 8 and M.plan_decode_id(O.Q4_K, 33024, 8, 2, 0, 256) is None
    assert M.plan_decode_id(O.Q4_K, 4096 + 32, 8, 2, 0, 256) is None and M.plan_decode_id(O.Q4_0, 4096 + 32, 8, 2, 0, 256).npre == 4              # K % block
    assert M.plan_decode_id(O.Q4_K, 256, 40, 2, 1, 256) is None and M.plan_decode_id(O.Q4_K, 256, 41, 2, 1, 256) is None                           # (nrows / 2) % 8, nrows % 2
    assert M.plan_decode_id(O.Q4_K, 256, 48, 2, 1, 256) == Pl(2, 0, 24, 1, False) and M.plan_decode_id(O.Q4_K, 256, 48, 2, 2, 256) is None
    assert M.plan_decode_id(O.Q5_K, 256, 48, 2, 0, 256) is None
    assert M.plan_combine(O.Q4_1, 64, 4136, 256) == Pl(256, 1, 40, 1, True) and M.plan_combine(O.Q4_1, 64, 4136, 256, n_used=4) is None
    assert M.plan_combine(O.Q4_1, 32768, 8, 256).npre == 8 and M.plan_combine(O.Q4_1, 32800, 8, 256) is None
    assert M.plan_router(O.Q4_K, 4096, 8, 2) == Pl(1, 0, 8, 1, False) and M.plan_router(O.Q8_0, 8192, 33, 4) == Pl(1, 2, 1, 4, False)
    assert M.plan_router(O.Q4_K, 16384, 64, 64) == Pl(1, 4, 0, 4, False) and M.plan_router(O.Q4_K, 16640, 64, 8) is None
    assert M.plan_router(O.Q4_K, 256, 65, 2) is None and M.plan_router(O.Q4_K, 256, 8, 9) is None and M.plan_router(O.Q4_K, 256, 8, 0) is None
    assert M.plan_router_silu(O.Q4_0, 64, 2128, 8, 8, 256) == Pl(32, 2, 40, 1, True) and M.plan_router_silu(O.Q4_0, 64, 40, 8, 2, 256) is None
    assert M.plan_router_silu(O.Q4_0, 16384, 16, 8, 2, 256).npre == 4 and M.plan_router_silu(O.Q4_0, 16416, 16, 8, 2, 256) is None
    assert M.plan_router_silu(O.Q4_0, 64, 16, 65, 2, 256) is None
    # the general path: 4 waves per workgroup, 8 workgroups per CU over all (slot, token) slices
    assert M.plan_mmvq_id(O.Q4_K, 512, 40, 2, 3, 256) == Pl(10, 1, 0, 0, False)                   # test_gpu_ops.test_mul_mat_id's shape
    assert M.plan_mmvq_id(O.Q4_K, 256, 30, 8, 40, 256) == Pl(6, 1, 6, 0, True)
    assert M.plan_mmvq_id(O.Q4_K, 256, 10, 8, 130, 256) == Pl(1, 2, 2, 0, True)
    assert M.plan_mmvq_id(O.Q8_0, 32, 8, 3, 21845, 256) == Pl(1, 2, 0, 0, True) and M.plan_mmvq_id(O.Q8_0, 32, 8, 2, 32768, 256) is None
    assert M.plan_kq_id(O.Q6_K, 256, 40, 8, 100) == Pl(2, 0, 8, 0, False) and M.plan_kq_id(O.Q6_K, 256, 40, 8, 8192) is None and M.plan_kq_id(O.Q6_K, 128, 40, 8, 1) is None
    assert M.mul_mat_id_path(O.Q4_K, 256, 40, 2, 1, 256)[0] == "decode_id" and M.mul_mat_id_path(O.Q4_K, 256, 40, 2, 2, 256)[0] == "mmvq_id"
    assert M.mul_mat_id_path(O.Q8_0, 96, 100, 2, 1, 256)[0] == "mmvq_id" and M.mul_mat_id_path(O.Q8_0, 96, 104, 2, 1, 256)[0] == "decode_id"       # 100 rows of 102 bytes: no multiple of 16
    assert M.mul_mat_id_path(O.IQ4_NL, 64, 40, 2, 1, 256)[0] == "kq_id" and M.mul_mat_id_path(O.Q4_K, 256, 40, 65, 1, 256)[0] == "mmvq_id"
    assert M.act_row_bytes(4096, 256) == 4096 + 64 + 512 and M.act_row_bytes(96, 32) == 96 + 16 + 16


def test_a_plan_deals_every_unit_once_and_swapped_counts_do_not():
    """the kernel's dealing under the plan's (grid, kfull, nrem) covers units 0 .. n - 1 once each.  With kfull and nrem swapped at the launcher it does not: units are
    left out or lie past the last row -- stores outside dst, which is why that mutant is judged here and never launched"""
    seen = 0
    for c in M.ONE_TOK:
        for n_cu in N_CUS:
            path, p = M.one_tok_plan(c, n_cu)
            if path == "decode_id":
                assert M.dealt_units(p.grid, p.kfull, p.nrem) == list(range(c.N)), c.name
                if p.kfull != p.nrem:
                    bad = M.dealt_units(p.grid, p.nrem, p.kfull)
                    assert bad != list(range(c.N)) and (max(bad) >= c.N or len(bad) < c.N), c.name
                    seen += 1
    for c in M.COMBINE:
        p = M.plan_combine(c.t, c.K, c.H, M.N_CU_MODEL, c.U)
        if p:
            assert M.dealt_units(p.grid, p.kfull, p.nrem) == list(range(c.H)), c.name
    for c in M.ROUTER:
        p = M.plan_router_silu(c.t, c.K, 2 * c.F, c.E, c.k, M.N_CU_MODEL)
        if p:
            assert M.dealt_units(p.grid, p.kfull, p.nrem) == list(range(c.F)), c.name
    assert seen >= len(M.TUNED) * 8


def test_lds_refusals_sit_behind_the_k_bounds():
    """the 160 KB checks of the one-token launchers: never the reason below their K bounds (so `one case past the limit` is the case one block past K 32768)"""
    worst = 0
    for t in M.TUNED:
        kind = 256 if t == O.Q4_K else 32
        for K in range(kind, 32768 + 1, kind):
            arb = M.act_row_bytes(K, kind)
            worst = max(worst, 2 * arb + 16 * M.Q32_CHAIN_BYTES)
            assert arb + 16 * M.Q32_CHAIN_BYTES + 3 * 64 * 4 <= M.DEC_LDS_MAX
    assert worst == 129280 and worst <= M.DEC_LDS_MAX


# ---- the oracle chains have the reference's node order --------------------------------------------------------------------------------------
def _combine_numpy(e, pr, ids, resid, variant="", divisor_ids=None):
    """GET_ROWS, SUM_ROWS (double, from 0, in slot order, rounded to float), one float DIV per slot, float MUL, float ADDs in slot order, float ADD of the residual"""
    T, k, H = e.shape
    out = np.zeros((T, H), f32)
    for t in range(T):
        w = pr[t, ids[t]].astype(f32)
        s = f64(0.0)
        for j in range(k):
            s = s + f64(w[j] if divisor_ids is None else pr[t, divisor_ids[j]])
        if variant == "double_divisor":
            wn = (w.astype(f64) / s).astype(f32)
        elif variant == "reciprocal":
            wn = w * (f32(1.0) / f32(s))
        else:
            wn = w / f32(s)
        order = range(k - 1, -1, -1) if variant == "reverse" else range(k)
        acc = None
        for j in order:
            y = e[t, j] * wn[j]
            acc = y if acc is None else acc + y
        if variant == "residual_first":
            acc = None
            for j in order:
                acc = (resid[t] + e[t, j] * wn[j]) if acc is None else acc + e[t, j] * wn[j]
        elif resid is not None:
            acc = acc + resid[t]
        out[t] = acc
    return out


@pytest.mark.parametrize("T,k,H,E", [(1, 2, 512, 8), (3, 2, 100, 8), (2, 1, 64, 4), (2, 4, 257, 16), (2, 8, 129, 64)])
def test_ref_combine_is_the_node_order(T, k, H, E):
    rng = np.random.default_rng([T, k, H, E])
    e = rng.standard_normal((T, k, H)).astype(f32)
    pr = np.stack([M.soft_row(rng, E) for _ in range(T)])
    ids = np.stack([rng.choice(E, k, replace=False) for _ in range(T)]).astype(np.int32)
    r = rng.standard_normal((T, H)).astype(f32)
    for resid in (None, r):
        got = M.ref_combine(e, pr, ids, resid)
        assert np.array_equal(got.view(np.uint32), _combine_numpy(e, pr, ids, resid).view(np.uint32))
    got = M.ref_combine(e, pr, ids, r).view(np.uint32)
    differ = {v: int(np.sum(got != _combine_numpy(e, pr, ids, r, v).view(np.uint32))) for v in ("double_divisor", "reciprocal", "reverse", "residual_first")}
    print(f"\nwords that another order changes: {differ}")
    if k >= 2:
        assert differ["reciprocal"] and differ["residual_first"]
    if k >= 3:
        assert differ["reverse"]


def test_ref_combine_shows_a_wrong_divisor():
    """the `binades` cases: p_1 / (p_0 + p_1) with p_1 ~ 2^-20 p_0 -- a divisor taken from other experts, or the double sum used unrounded, changes the bits"""
    hit, others_seen = 0, False
    for c in M.COMBINE:
        if c.probs == "binades":
            d = M.combine_data(c)
            pr, ids = d["probs"], d["ids"]
            assert np.array_equal(_combine_numpy(d["down"], pr, ids, d["resid"]).view(np.uint32), d["want"].view(np.uint32))
            others = [i for i in range(c.E) if i not in ids[0]]
            if len(others) >= 2:
                wrong = _combine_numpy(d["down"], pr, ids, d["resid"], divisor_ids=others[:2])
                assert not np.array_equal(wrong.view(np.uint32), d["want"].view(np.uint32))
                others_seen = True
            w0, w1 = pr[0, ids[0, 0]], pr[0, ids[0, 1]]
            hit += f32(w1 / f32(f64(w0) + f64(w1))) != f32(f64(w1) / (f64(w0) + f64(w1)))
            assert w0 / w1 > 2.0 ** 18
    assert others_seen
    assert hit == sum(c.probs == "binades" for c in M.COMBINE)      # rounding the sum to float before the division shows in every one


def _act_step_bound(x, w_abs, blk):
    """|W . x - W . dequant(quant(x))| <= sum over blocks of (amax / 254) * sum |w|: the Q8 activation rounds every value to a step of amax / 127"""
    amax = np.abs(x).reshape(-1, blk).max(1)
    return (w_abs.reshape(w_abs.shape[0], -1, blk).sum(2) * (amax / 254.0)).sum(1)


@pytest.mark.parametrize("t", M.TUNED, ids=[M.TYPE_NAME[t] for t in M.TUNED])
def test_ref_router_is_the_node_order(t):
    """against float64: xnorm to float rounding, the logits inside the activation quantizer's step bound, SOFT_MAX of the oracle's own logits to float rounding, and the ids
    = the k largest probabilities"""
    rng = np.random.default_rng(t)
    K, E, k = 512, 16, 4
    x, gw = (rng.standard_normal(K) * 1.7).astype(f32), (1.0 + 0.1 * rng.standard_normal(K)).astype(f32)
    wr = M.router_weights(t, E, K, rng, x, gw)
    xn, pr, ids, lg = M.ref_router(t, wr, x, gw, k)
    assert 0.5 < np.std(lg) < 8 and pr.min() > 1e-20
    x64 = x.astype(f64)
    xn64 = x64 / np.sqrt(np.mean(x64 * x64) + f64(f32(M.EPS))) * gw.astype(f64)
    assert np.max(np.abs(xn - xn64) / np.abs(xn64)) < 4 * 2.0 ** -24
    W = np.stack([O.dequantize(t, wr[e], K) for e in range(E)]).astype(f64)
    lg64 = W @ xn.astype(f64)
    bound = _act_step_bound(xn.astype(f64), np.abs(W), 256 if t == O.Q4_K else 32) + 1e-5 * np.abs(W) @ np.abs(xn.astype(f64))
    if t == O.Q4_1:                                         # the minimum's term uses s = fp16(d * sum q): relative 2^-11 of every block's |m * s|
        bound = bound + 2.0 ** -10 * np.abs(W) @ np.abs(xn.astype(f64)) + 1e-3
    assert np.all(np.abs(lg - lg64) <= bound), float(np.max(np.abs(lg - lg64) / bound))
    p64 = np.exp(lg.astype(f64) - lg.astype(f64).max())
    p64 /= p64.sum()
    assert np.max(np.abs(pr - p64) / p64) < 1e-6
    assert set(ids.tolist()) == set(np.argsort(-pr, kind="stable")[:k].tolist())


# ---- a whole block, node by node, against the reference build ------------------------------------------------------------------------------------
@pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref not built")
@pytest.mark.parametrize("case", M.BLOCKS, ids=name_of)
def test_ref_block_equals_the_reference_build_node_by_node(case):
    c, d, R = case, M.block_data(case), O.ref()
    ref, K, F, E, k = d["ref"], case.K, case.F, case.E, case.k
    i64 = C.c_int64
    same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32).reshape(-1), np.ascontiguousarray(b).view(np.uint32).reshape(-1))  # noqa: E731
    x, gw = np.array(d["x"]), np.array(d["gw"])
    n1, xn, lg, pr, ids = np.zeros(K, f32), np.zeros(K, f32), np.zeros(E, f32), np.zeros(E, f32), np.zeros(k, np.int32)
    assert R.ref_unary(0, i64(K), i64(1), i64(1), P(x), P(n1), C.c_float(M.EPS), C.c_int(0)) == 0
    assert R.ref_binary(1, i64(K), i64(1), i64(1), P(n1), i64(K), i64(1), i64(1), P(gw), P(xn)) == 0
    assert same(xn, ref["xnorm"])
    assert R.ref_mul_mat(c.t, i64(K), i64(E), i64(1), i64(1), i64(1), P(d["wr"]), P(xn), P(lg)) == 0
    assert same(lg, ref["logits"])
    assert R.ref_unary(2, i64(E), i64(1), i64(1), P(lg), P(pr), C.c_float(0), C.c_int(0)) == 0
    assert same(pr, ref["probs"])
    assert R.ref_top_k(i64(E), i64(1), i64(1), P(pr), C.c_int(k), P(ids)) == 0
    assert np.array_equal(ids, ref["ids"])
    g, u, s, gu = (np.zeros((k, F), f32) for _ in range(4))
    assert R.ref_mul_mat_id(c.t, i64(K), i64(F), i64(E), i64(1), i64(k), i64(1), P(d["wg"]), P(xn), P(ids), P(g)) == 0
    assert R.ref_mul_mat_id(c.t, i64(K), i64(F), i64(E), i64(1), i64(k), i64(1), P(d["wu"]), P(xn), P(ids), P(u)) == 0
    assert R.ref_unary(1, i64(F), i64(k), i64(1), P(g), P(s), C.c_float(0), C.c_int(0)) == 0
    assert R.ref_binary(1, i64(F), i64(k), i64(1), P(s), i64(F), i64(k), i64(1), P(u), P(gu)) == 0
    assert same(gu, ref["g"])
    down = np.zeros((k, K), f32)
    assert R.ref_mul_mat_id(c.t, i64(F), i64(K), i64(E), i64(k), i64(k), i64(1), P(d["wd"]), P(gu), P(ids), P(down)) == 0
    assert same(down, ref["down"])
    w, sm, wn, y = np.zeros(k, f32), np.zeros(1, f32), np.zeros(k, f32), np.zeros((k, K), f32)
    assert R.ref_get_rows(O.F32, i64(1), i64(E), P(pr), i64(k), P(ids), P(w)) == 0
    assert R.ref_sum_rows(i64(k), i64(1), i64(1), P(w), P(sm)) == 0
    assert R.ref_binary(2, i64(k), i64(1), i64(1), P(w), i64(1), i64(1), i64(1), P(sm), P(wn)) == 0
    assert R.ref_binary(1, i64(K), i64(k), i64(1), P(down), i64(1), i64(k), i64(1), P(wn), P(y)) == 0
    acc = np.ascontiguousarray(y[0])
    for j in range(1, k):
        nxt = np.zeros(K, f32)
        assert R.ref_binary(0, i64(K), i64(1), i64(1), P(acc), i64(K), i64(1), i64(1), P(np.ascontiguousarray(y[j])), P(nxt)) == 0
        acc = nxt
    out = np.zeros(K, f32)
    assert R.ref_binary(0, i64(K), i64(1), i64(1), P(acc), i64(K), i64(1), i64(1), P(x), P(out)) == 0
    assert same(out, ref["out"])
