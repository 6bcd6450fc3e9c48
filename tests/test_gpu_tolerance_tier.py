"""The tolerance-tier product kernels, element by element, against the float64 error model of tests/tier_model.py (tests/test_tier_model.py shows on the CPU that
its bounds pass the reference and fail a subtly wrong kernel): k_mmq (mmq.hip, prefill mode 0) with its fused forms, k_mmd (dense_f16.hip, the f16 mode, both tiles)
and the free-order decode mat-vec (gemv_free32.hip).  Through the C ABI, like tests/test_gpu_ops.py.  Each test prints its largest |got - R| / bound."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import tier_model as TM
from conftest import prefill_mode

pytestmark = pytest.mark.gpu
ids = lambda c: "-".join(str(v) for v in c)
bits = lambda a: np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def check_fast(tag, case, got, w, x, ne02=1, extra=None):
    """every element of got [ne12, M, N] inside (n_t + 8) 2^-24 S of the float64 sum of its block terms"""
    t, K, N, M = case[:4]
    ne12 = x.shape[0]
    worst = 0.0
    for i in range(ne12):
        i02 = i // (ne12 // ne02)
        T = TM.terms_matrix(t, w[i02 * N:(i02 + 1) * N], TM.act_rows(O, t, x[i]))
        R, bound = TM.fast_bound(T, extra=extra)
        ratio = np.abs(got[i].astype(np.float64) - R) / bound
        worst = max(worst, float(ratio.max()))
    print(f"TIER_RATIO {tag} {ids(case)} {worst:.4f}")
    assert np.all(np.isfinite(got)) and worst <= 1.0, worst
    return worst


# ---- fast mode: the plain product -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TM.FAST_CASES, ids=ids)
def test_fast_mode_product_is_inside_the_bound_at_every_element(gpu, case):
    """k_mmq at its edges: K % 256 != 0 (the guarded last step of its K walk), one-block rows, fewer rows than one 16-row patch, one weight row, several token and
    row tiles, batched / broadcast operands, a quiet last token -- every output element against its own bound; at K >= 4096 the result also differs from the
    exact mode's in some word (or the switch changed nothing and this test checks nothing)"""
    t, K, N, M, ne02, ne12 = case
    w, x = TM.case_inputs(*case)
    dw, dx = gpu.Tensor.from_numpy(w, t, [K, N, ne02]), gpu.Tensor.from_numpy(x)
    with prefill_mode(gpu, 0):
        got = gpu.ops.mul_mat(dw, dx).numpy().reshape(ne12, M, N)
    check_fast("fast", case, got, w, x, ne02)
    if K >= 4096:
        assert not np.array_equal(bits(got), bits(gpu.ops.mul_mat(dw, dx).numpy()))


def test_fast_mode_product_into_a_strided_dst_keeps_the_padding(gpu):
    """dst is a view whose rows are 7 floats wider than N: the product lands inside the bound, the padding keeps its fill pattern"""
    case = t, K, N, M, _, _ = (TM.Q4_1, 288, 129, 65, 1, 1)
    w, x = TM.case_inputs(*case)
    fill = (np.arange(M * (N + 7), dtype=np.uint32) | 0x7fc00000).view(np.float32).reshape(M, N + 7)      # NaNs with the index as payload
    buf = gpu.Tensor.from_numpy(fill)
    with prefill_mode(gpu, 0):
        gpu.ops.mul_mat(gpu.Tensor.from_numpy(w, t, [K, N]), gpu.Tensor.from_numpy(x), dst=buf.view([N, M], [4, (N + 7) * 4]))
    out = buf.numpy()
    assert np.array_equal(out[:, N:].view(np.uint32), fill[:, N:].view(np.uint32))
    check_fast("fast-strided", case, np.ascontiguousarray(out[:, :N])[None], w, x)


# ---- fast mode: the fused forms of cllm_op_mul_mat_ex --------------------------------------------------------------------
@pytest.mark.parametrize("case", TM.FUSED_CASES, ids=ids)
def test_fast_mode_fused_forms_equal_the_node_sequences(gpu, case):
    """cllm_op_mul_mat_ex under prefill mode 0 (launch_mmq with a residual / the SiLU * up epilogue; the quantizer prologues 1 / 3 / 4 / 5): bit for bit the same
    mode's plain mul_mat over separately computed activations, then ops.add / ops.mul(ops.silu(gate), up) -- the same kernel, the same order, one more node.
    The SiLU * up epilogue takes ggml_vec_silu_f32's branch per feature (polynomial body below (N / 2) & ~7, libm tail above) exactly as ops.silu does on
    the contiguous [N / 2, M] gate: no disagreement between the two was found at these shapes"""
    t, K, N, M = case
    ops, T = gpu.ops, gpu.Tensor
    r_ = np.random.default_rng([7, t, K, N, M])
    wb, xh = TM.case_inputs(t, K, N, M)
    w = T.from_numpy(wb, t, [K, N])
    x = T.from_numpy(xh[0]); g = T.from_numpy((1.0 + 0.1 * r_.standard_normal(K)).astype(np.float32))
    with prefill_mode(gpu, 0):
        plain = ops.mul_mat(w, x)
        check_fast("fast-fused-shape", case, plain.numpy()[None], wb, xh)
        # RMS_NORM -> MUL -> MUL_MAT
        want = ops.mul_mat(w, ops.rms_norm_mul(x, g, 1e-5))
        assert np.array_equal(bits(ops.mul_mat_ex(w, x, pro=1, norm_w=g, eps=1e-5).numpy()), bits(want.numpy()))
        # ... -> ADD(resid): out of place, and in place on the residual
        rh = r_.standard_normal((M, N)).astype(np.float32)
        r = T.from_numpy(rh)
        want_r = ops.add(plain, r)
        assert np.array_equal(bits(ops.mul_mat_ex(w, x, resid=r).numpy()), bits(want_r.numpy()))
        r2 = T.from_numpy(rh)
        ops.mul_mat_ex(w, x, resid=r2, dst=r2)
        assert np.array_equal(bits(r2.numpy()), bits(want_r.numpy()))
        check_fast("fast-resid", case, r2.numpy()[None], wb, xh, extra=[rh.astype(np.float64)])
        # rows alternate gate_u, up_u: MUL_MAT -> (even, odd) -> SILU -> MUL in the epilogue, plain and with the norm prologue in front
        for pro, y in ((0, plain), (1, want)):
            gate = y.view([N // 2, M], [8, y.nb[1]], offset=0); up = y.view([N // 2, M], [8, y.nb[1]], offset=4)
            want_s = ops.mul(ops.silu(ops.cont(gate)), ops.cont(up))
            got_s = ops.mul_mat_ex(w, x, pro=pro, norm_w=g if pro else None, eps=1e-5, epi=1)
            assert np.array_equal(bits(got_s.numpy()), bits(want_s.numpy())), pro
        # UNARY(SILU)(gate) -> MUL(up) -> MUL_MAT with separate gate / up tensors (pro 4), + the residual
        gt = T.from_numpy(r_.standard_normal((M, K)).astype(np.float32)); ut = T.from_numpy(r_.standard_normal((M, K)).astype(np.float32))
        want_4 = ops.add(ops.mul_mat(w, ops.mul(ops.silu(gt), ut)), r)
        assert np.array_equal(bits(ops.mul_mat_ex(w, gt, pro=4, norm_w=ut, resid=r).numpy()), bits(want_4.numpy()))
        # a second projection of the same activation reuses the act rows of the previous call (pro 5)
        w2 = T.from_numpy(TM.case_inputs(t, K, N + 2, M)[0][:N], t, [K, N])
        ops.mul_mat_ex(w, x, pro=1, norm_w=g, eps=1e-5)
        assert np.array_equal(bits(ops.mul_mat_ex(w2, x, pro=5).numpy()), bits(ops.mul_mat(w2, ops.rms_norm_mul(x, g, 1e-5)).numpy()))
        # the SiLU * up quantizer prologue (interleaved pairs in src1)
        x2 = T.from_numpy(r_.standard_normal((M, 2 * K)).astype(np.float32))
        ge = x2.view([K, M], [8, x2.nb[1]], offset=0); ue = x2.view([K, M], [8, x2.nb[1]], offset=4)
        want_p = ops.mul_mat(w, ops.mul(ops.silu(ops.cont(ge)), ops.cont(ue)))
        assert np.array_equal(bits(ops.mul_mat_ex(w, x2, pro=3).numpy()), bits(want_p.numpy()))
    # the mode was what computed all of the above: at K >= 256 the fast product is not the exact mode's
    if K >= 256:
        assert not np.array_equal(bits(plain.numpy()), bits(ops.mul_mat(w, x).numpy()))


# ---- f16 mode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("case", TM.F16_CASES, ids=ids)
def test_f16_mode_product_is_inside_the_bound_at_every_element(gpu, case, tile):
    """k_mmd at both workgroup tiles: every element within 2 K 2^-24 sum_k |w16 x16| of the float64 product of the fp16 weights its staging forms (mirrored step by
    step in tier_model.f16_weights) with the fp16-rounded activations"""
    t, K, N, M = case
    w, x = TM.case_inputs(t, K, N, M, quiet=TM.QUIET_F16)
    lib = C.CDLL(gpu.lib.SO_PATH)
    lib.cllm_debug_set_prefill_f16(1)
    lib.cllm_debug_set_mmd_tile(tile)
    try:
        with prefill_mode(gpu, 0):
            got = gpu.ops.mul_mat(gpu.Tensor.from_numpy(w, t, [K, N]), gpu.Tensor.from_numpy(x)).numpy().reshape(M, N)
    finally:
        lib.cllm_debug_set_prefill_f16(0)
        lib.cllm_debug_set_mmd_tile(0)
    R, bound = TM.f16_bound(t, w, x[0])
    ratio = np.abs(got.astype(np.float64) - R) / bound
    print(f"TIER_RATIO f16-{tile} {ids(case)} {float(ratio.max()):.4f}")
    assert np.all(np.isfinite(got)) and np.all(ratio <= 1.0), float(ratio.max())


# ---- the free-order decode tier ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TM.FREE_CASES, ids=ids)
def test_free_order_mat_vec_is_inside_the_bound_at_every_element(gpu, case):
    """cllm_set_decode_free_order(1): the one-column mul_mat, cllm_op_mul_mat_vec_fused with prologue 1 (RMS norm: the activation is the oracle's rms_norm and
    mul) and with prologue 2 + the residual (the C ABI's fused op has no bias slot: the residual is the one extra addend) -- every element inside the fast-mode
    bound; the same calls with the tier off equal the oracle word for word (the switch is what changed the path), and at K >= 4096 the tier's result differs from
    the exact one in some word (or the tier was never entered)"""
    t, K, N = case
    ops, T, L = gpu.ops, gpu.Tensor, gpu.lib.get()
    wb, xh = TM.case_inputs(t, K, N, 1)
    r_ = np.random.default_rng([11, t, K, N])
    gh = (1.0 + 0.1 * r_.standard_normal(K)).astype(np.float32)
    rh = r_.standard_normal(N).astype(np.float32)
    w, x, g, r = T.from_numpy(wb, t, [K, N]), T.from_numpy(xh[0]), T.from_numpy(gh.reshape(1, K)), T.from_numpy(rh.reshape(1, N))
    cw = w.c()

    def fused(pro, resid):
        out = T(gpu.F32, [N, 1])
        gpu.lib.check(L.cllm_op_mul_mat_vec_fused(None, C.byref(cw), pro, x.data_ptr(), g.data_ptr() if pro == 1 else None, 1e-5, 0,
                                                  r.data_ptr() if resid else None, out.data_ptr()), "fused")
        return out.numpy().reshape(1, 1, N)

    def forms():
        return ops.mul_mat(w, x).numpy().reshape(1, 1, N), fused(1, False), fused(2, True)

    # the oracle: the plain product, RMS_NORM -> MUL -> MUL_MAT, MUL_MAT -> ADD
    xn = np.zeros_like(xh[0])
    O.rms_norm(O.tensor(xh[0], O.F32, [K, 1]), O.tensor(xn, O.F32, [K, 1]), 1e-5)
    xn = (xn * gh).reshape(1, 1, K)
    want, want_n = np.zeros(N, np.float32), np.zeros(N, np.float32)
    O.mul_mat(O.tensor(wb, t, [K, N]), O.tensor(xh[0], O.F32, [K, 1]), O.tensor(want, O.F32, [N, 1]))
    O.mul_mat(O.tensor(wb, t, [K, N]), O.tensor(xn, O.F32, [K, 1]), O.tensor(want_n, O.F32, [N, 1]))
    L.cllm_set_decode_free_order(1)
    try:
        free = forms()
    finally:
        L.cllm_set_decode_free_order(0)
    exact = forms()
    for got, ref in zip(exact, (want, want_n, want + rh)):
        assert np.array_equal(bits(got), bits(ref))
    c4 = (t, K, N, 1)
    check_fast("free-plain", c4, free[0], wb, xh)
    check_fast("free-norm", c4, free[1], wb, xn)
    check_fast("free-resid", c4, free[2], wb, xh, extra=[rh.astype(np.float64)[None, :]])
    if K >= 4096:
        for a, b in zip(free, exact):
            assert not np.array_equal(bits(a), bits(b))
