"""Why the bounds of tests/tier_model.py can be trusted (no GPU): the decoders are pinned to the oracle, the reference's own result passes, a subtly wrong kernel
(a dropped block, a neighbour's scale, a skipped K tail) fails at every mutated element, and the max-norm checks these bounds replace would have let it through.
Everything runs over the case list the GPU tests use (tier_model.FAST_CASES, FUSED_CASES, F16_CASES, FREE_CASES)."""
import functools

import numpy as np
import pytest

import oracle as O
import tier_model as TM

WTYPES = (TM.Q4_0, TM.Q4_1, TM.Q8_0, TM.Q4_K)
# every shape of section 3 as a plain product: the fast-mode list, the fused forms' shapes, the free-order list (one column)
PRODUCT_CASES = list(dict.fromkeys(TM.FAST_CASES + [(t, K, N, M, 1, 1) for t, K, N, M in TM.FUSED_CASES] + [(t, K, N, 1, 1, 1) for t, K, N in TM.FREE_CASES]))
ids = lambda c: "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=2)
def product(case):
    """per batch slice i12 of a case: (weight rows, activation rows, block terms T [M, N, n_t]); and the oracle's result [ne12, M, N]"""
    t, K, N, M, ne02, ne12 = case
    w, x = TM.case_inputs(*case)
    want = np.zeros((ne12, M, N), np.float32)
    O.mul_mat(O.tensor(w, t, [K, N, ne02]), O.tensor(x, O.F32, [K, M, ne12]), O.tensor(want, O.F32, [N, M, ne12]))
    out = []
    for i in range(ne12):
        i02 = i // (ne12 // ne02)
        wr, ar = w[i02 * N:(i02 + 1) * N], TM.act_rows(O, t, x[i])
        out.append((wr, ar, TM.terms_matrix(t, wr, ar)))
    return out, want


# ---- the decoders are the oracle's ----------------------------------------------------------------------------------
@pytest.mark.parametrize("t", WTYPES)
def test_weight_decoders_equal_dequantize_word_for_word(t):
    """float32(dequant64) == dequantize_row_* for every weight row of every case: all four types, Q4_K included -- d sc, dmin mn and (d sc) nib are exact in
    fp32 (11 x 6 x 4 bits), so the reference rounds once, at the subtraction, and so does the conversion of the exact float64 value"""
    for case in PRODUCT_CASES:
        if case[0] != t:
            continue
        w, _ = TM.case_inputs(*case)
        K = case[1]
        got = TM.dequant64(t, w).astype(np.float32)
        for r in range(0, w.shape[0], max(1, w.shape[0] // 16)):
            assert np.array_equal(got[r].view(np.uint32), O.dequantize(t, w[r], K).view(np.uint32)), (case, r)
        assert np.array_equal(got[-1].view(np.uint32), O.dequantize(t, w[-1], K).view(np.uint32)), case


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=ids)
def test_integer_block_sums_equal_vec_dot(case):
    """the decoded integer products, summed, are vec_dot's exact int32 sums (Q4_K: per super-block sum_b sc[b] s_b and sum_b mn[b] bsum[b]); the activation
    decoders' side fields are what the formats say (Q8_1: s = d sum q to fp16 precision; Q8_K: bsums = sums of 16 quants)"""
    t, K, N, M = case[:4]
    (wr, ar, _), = product(case)[0][:1]
    s = TM.block_isums(t, wr, ar)
    a = TM.ACT_DECODE[t](ar)
    if t == TM.Q4_1:
        ds = a["d"] * a["q"].sum(-1)                 # s = fp16(d sum q) of the UNROUNDED fp32 d (quantize_row_q8_1): two fp16 roundings from the decoded d
        assert np.all(np.abs(a["s"] - ds) <= 2.0 ** -10 * np.abs(ds) + 2.0 ** -25 * np.abs(a["q"].sum(-1)) + 2.0 ** -24)      # (+ subnormal fp16 d and s)
    if t == TM.Q4_K:
        assert np.array_equal(a["bsums"], a["q"].reshape(M, -1, 16, 16).sum(-1))
        w4 = TM.decode_q4_K(wr)
    for m, n in {(0, 0), (M - 1, N - 1), (M // 2, N // 3), (M // 3, N // 2)}:
        _, want = O.vec_dot(t, K, wr[n], ar[m])
        if t == TM.Q4_K:
            bs32 = a["bsums"][m].reshape(-1, 8, 2).sum(-1)
            got = np.stack([(w4["sc"][n] * s[m, n].reshape(-1, 8)).sum(-1), (w4["mn"][n] * bs32).sum(-1)], axis=-1).reshape(-1)
        else:
            got = s[m, n]
        assert np.array_equal(got.astype(np.int64), want.astype(np.int64)), (m, n)


def test_terms_of_one_element_are_the_matrix_terms():
    for case in [(TM.Q4_1, 96, 10, 33, 1, 1), (TM.Q4_K, 768, 129, 65, 1, 1)]:
        (wr, ar, T), = product(case)[0]
        assert np.array_equal(TM.terms(case[0], wr[7], ar[5]), T[5, 7])
        lanes = TM.terms_matrix(case[0], wr[7:8], ar[5:6], lanes=True)[0, 0]
        nb = TM.n_blocks32(case[0], T)
        assert np.allclose(lanes[:8 * nb].reshape(nb, 8).sum(-1), T[5, 7, :nb], rtol=1e-13, atol=0)


# ---- the reference passes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PRODUCT_CASES, ids=ids)
def test_the_reference_passes_the_bound(case):
    """O.mul_mat's result (the reference's AVX2 order) satisfies (n_t + 8) 2^-24 S at every element of every case -- over the terms the reference FORMS: it
    adds the eight int32 lanes of a block dot product separately (fmaf(d_w d_x, float(lane), acc[lane])), so its terms are the lane parts of T_b
    (tier_model.terms_matrix(lanes=True)).  Over whole-block terms the reference does NOT pass at one-block rows (K = 32: |got - R| up to 21 x the bound for
    Q4_0, 4 x for Q8_0): where the lane parts cancel, |T_b| is far below what its accumulators rounded.  The kernels under test convert the WHOLE block sum
    exactly and are held to the tighter block-term bound"""
    t, K, N, M, ne02, ne12 = case
    slices, want = product(case)
    worst = 0.0
    for i, (wr, ar, T) in enumerate(slices):
        R, _ = TM.fast_bound(T)
        Rl, bound = TM.fast_bound(TM.terms_matrix(t, wr, ar, lanes=True))
        assert np.all(np.abs(R - Rl) <= 1e-13 * np.abs(T).sum(-1))            # the same sum, split finer
        ratio = np.abs(want[i].astype(np.float64) - Rl) / bound
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (i, float(ratio.max()))
        if K >= 96:                                                          # with three blocks or more the reference is inside the block-term bound as well
            assert np.all(np.abs(want[i].astype(np.float64) - R) <= TM.fast_bound(T)[1])
    print(f"reference |got - R| / bound: {worst:.3f} {ids(case)}")


# ---- a wrong kernel fails ------------------------------------------------------------------------------------------------
def pick_at_least_median(mag):
    """along the last axis: the index of the SMALLEST entry that is >= the median of the axis (the mutation hardest to see among those the rule allows)"""
    med = np.median(mag, axis=-1, keepdims=True)
    return np.argmin(np.where(mag >= med, mag, np.inf), axis=-1)


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=ids)
def test_mutants_violate_the_fast_bound(case):
    """three wrong kernels, built in float64 from the exact terms.  One rule picks what is mutated: the CHANGE a mutation makes to an element is at least the
    median |T| of that element (a change far below a term -- a block whose integer sum happens to be 0, a neighbour whose scale is the same fp16 number --
    leaves the very same float and no check can see it).  Every mutated element must then be OUTSIDE the bound: 0 undetected.
    (a) one term dropped, at every element: the SMALLEST of the terms with |T_i| >= median |T|;
    (b) one block's scale term taken with the NEXT weight row's scale d' (the previous row's for the last row; a case with one row has no neighbour): of the
        blocks with |T_b| >= median |T| the one whose neighbour scale differs most, at every element where that is |d' / d - 1| >= 1 / 8 (most of them: rand_blocks
        draws d uniformly from a range of 1 : 4);
    (c) K % 256 != 0: the K tail (the blocks from 256 (K // 256) on, scale and min terms) left out of one whole column (token 0): every element of it whose tail
        amounts to a median term or more"""
    t, K, N, M, ne02, ne12 = case
    slices, _ = product(case)
    for wr, ar, T in slices:
        R, bound = TM.fast_bound(T)
        mag, med = np.abs(T), np.median(np.abs(T), axis=-1)
        nb = TM.n_blocks32(t, T)
        # (a)
        ia = pick_at_least_median(mag)
        Ta = np.take_along_axis(T, ia[..., None], -1)[..., 0]
        assert np.all(np.abs(Ta) >= med) and np.all(np.abs(Ta) > bound), float(np.mean(np.abs(Ta) <= bound))
        # (b)
        if N > 1:
            bs = TM.W_BLOCK_BYTES[t]
            blk = wr.reshape(N, -1, bs).copy()
            nxt = np.concatenate([np.arange(1, N), [N - 2]])
            blk[:, :, 0:2] = blk[nxt][:, :, 0:2]
            delta = np.abs(TM.terms_matrix(t, blk.reshape(N, -1), ar)[..., :nb] - T[..., :nb])
            dist = np.abs(TM.W_DECODE[t](blk.reshape(N, -1))["d"] / TM.W_DECODE[t](wr)["d"] - 1.0)              # [N, blocks]
            dist = np.broadcast_to(np.repeat(dist, nb // dist.shape[-1], axis=-1)[None], delta.shape)
            ib = np.argmax(np.where(mag[..., :nb] >= med[..., None], dist, -1.0), axis=-1)
            has = np.take_along_axis(dist, ib[..., None], -1)[..., 0] >= 0.125
            db = np.take_along_axis(delta, ib[..., None], -1)[..., 0]
            assert np.mean(has) >= 0.5 or has.size < 16, float(np.mean(has))      # (a handful of elements may all have near-equal neighbours)
            assert np.all(db[has] > bound[has]), float(np.mean(db[has] <= bound[has]))
        # (c)
        if K % 256 and t != TM.Q4_K:
            b0 = (K // 256) * 8
            tail = np.abs(T[0, :, b0:nb].sum(-1) + (T[0, :, nb + b0:].sum(-1) if t == TM.Q4_1 else 0.0))
            has = tail >= med[0]
            assert np.mean(has) >= 0.25, float(np.mean(has))
            assert np.all(tail[has] > bound[0][has]), float(np.min(tail[has] / bound[0][has]))


def test_residual_and_bias_are_one_more_term_each():
    case = (TM.Q8_0, 544, 8, 1, 1, 1)
    (wr, ar, T), = product(case)[0]
    r = np.random.default_rng(5).standard_normal(8)
    R0, b0 = TM.fast_bound(T)
    R1, b1 = TM.fast_bound(T, extra=[r[None, :]])
    assert np.allclose(R1, R0 + r) and np.allclose(b1, (T.shape[-1] + 9) * TM.U32 * (np.abs(T).sum(-1) + np.abs(r)))


# ---- the f16 mode ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def f16_product(case):
    t, K, N, M = case
    w, x = TM.case_inputs(t, K, N, M, quiet=TM.QUIET_F16)
    return w, x[0]


@pytest.mark.parametrize("case", TM.F16_CASES, ids=ids)
def test_f16_weights_are_the_dequantized_ones_rounded(case):
    """the mirror of dense_f16.hip's staging stays within the fp16 roundings it makes of the oracle's dequantized weight: one (Q4_0, Q8_0, Q4_1: 2^-11 relative of
    the result) or, Q4_K, three (d sc, dmin mn, the fma: 2^-11 of |d sc nib| + |dmin mn| + |w|) -- and equals float16(dequantize) outright for Q4_0 / Q8_0 / Q4_1"""
    t, K, N, M = case
    w, _ = f16_product(case)
    w16, w64 = TM.f16_weights(t, w), TM.dequant64(t, w)
    assert np.array_equal(w16, w16.astype(np.float16).astype(np.float64))
    if t != TM.Q4_K:
        assert np.array_equal(w16, w64.astype(np.float16).astype(np.float64))
    else:
        d = TM.decode_q4_K(w)
        mags = ((d["d"][..., None] * d["sc"])[..., None] * d["q"] + (d["dmin"][..., None] * d["mn"])[..., None]).reshape(w64.shape)
        assert np.all(np.abs(w16 - w64) <= 2.0 ** -11 * (mags + np.abs(w64)) + 2.0 ** -24)


@pytest.mark.parametrize("case", TM.F16_CASES, ids=ids)
def test_f16_mutant_violates_the_bound(case):
    """a 32-element chunk of K dropped, at every element: the FIRST chunk in K order whose contribution is >= the element's median chunk -- outside
    2 K 2^-24 sum |w16 x16|.  K <= 4352: a median chunk is still above the bound, by a factor that shrinks with K (Q4_K, whose weights are not centred,
    at K = 4352: down to 0.9 at the worst element -- so the hardest pick, the smallest chunk above the median, is not what this test asks for)"""
    t, K, N, M = case
    assert K <= 4352
    w, x = f16_product(case)
    R, bound = TM.f16_bound(t, w, x)
    w16 = TM.f16_weights(t, w).reshape(N, K // 32, 32)
    x16 = x.astype(np.float16).astype(np.float64).reshape(M, K // 32, 32)
    C = np.einsum("mbk,nbk->mnb", x16, w16)
    assert np.all(np.abs(C.sum(-1) - R) <= 1e-12 * np.abs(C).sum(-1))
    ic = np.argmax(np.abs(C) >= np.median(np.abs(C), axis=-1, keepdims=True), axis=-1)
    Cc = np.take_along_axis(C, ic[..., None], -1)[..., 0]
    assert np.all(np.abs(Cc) > bound), (float(np.mean(np.abs(Cc) <= bound)), float(np.min(np.abs(Cc) / bound)))


# ---- the checks these bounds replace would have missed it ---------------------------------------------------------------------
def test_the_old_max_norm_checks_miss_a_dropped_block():
    """mutant (a) at an element of the quiet token: the old checks -- max |delta| / max |ref| < 1e-5 (fast mode), max |delta| <= 1.5e-3 max |ref| (f16 mode) --
    pass, the component-wise bound fails"""
    case = (TM.Q4_0, 4128, 130, 129, 1, 1)
    (wr, ar, T), = product(case)[0]
    R, bound = TM.fast_bound(T)
    m, n = case[3] - 1, 77
    i = int(pick_at_least_median(np.abs(T[m, n])))
    mutant = R.copy()
    mutant[m, n] -= T[m, n, i]
    assert np.max(np.abs(mutant - R)) / np.max(np.abs(R)) < 1e-5                     # tests/test_gpu_ops.py rel_err(got, want) < T1
    assert np.abs(mutant[m, n] - R[m, n]) > bound[m, n]
    assert np.sum(np.abs(mutant - R) > bound) == 1

    t, K, N, M = fcase = (TM.Q4_0, 4128, 130, 129)
    w, x = f16_product(fcase)
    R, bound = TM.f16_bound(t, w, x)
    w16, x16 = TM.f16_weights(t, w), x.astype(np.float16).astype(np.float64)
    C = (x16[m] * w16[n]).reshape(K // 32, 32).sum(-1)
    c = C[int(pick_at_least_median(np.abs(C)))]
    assert abs(c) <= 1.5e-3 * np.max(np.abs(R))                                      # test_mul_mat_quant_dense_f16_mode's bound
    assert abs(c) > bound[m, n]
