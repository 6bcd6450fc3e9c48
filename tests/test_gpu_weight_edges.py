"""Every weight format on the device at the scale fields of tests/weight_edge_cases.py -- negative, fp16-subnormal, zero and maximal scales, saturated quants,
activations that push the scale products and sums of the Q8_K-activation formats into the fp32 subnormals (the Q8_0 / Q8_1-activation formats put out +-0
there: weight_edge_cases.tiny_activations) -- against the CPU oracle, which tests/test_weight_edge_model.py holds word for word against the
reference build on the same blocks.  That module also shows that no expected word here is a NaN (and that infinities occur in MXFP4's `large` GET_ROWS alone), so
every exact comparison is np.array_equal on the uint32 view of the whole result, no exemption.

  GET_ROWS            all 22 block types and F16
  MUL_MAT             all 22 types at 1, 5 and 40 columns (decode mat-vec; column chunks and the kq kernels' any-column form; mmx.hip for the four tuned types)
  side-by-side / team Q4_0 / Q4_1 / Q8_0, one column, each rows32 and team32 form at shapes those launchers take (K = 1024 for the teams: a team of 5 wants K >= 800)
  fused mat-vec       RMS-norm prologue + residual in one launch == the node sequence, the four tuned types
  MUL_MAT_ID          one token, 4 experts, 2 slots, all 22 types
  tolerance tiers     k_mmq (fast prefill), the free-order mat-vec and k_mmd (f16 prefill, both tiles), element by element inside tier_model's bounds as they stand.
                      `large` is left out of the f16 mode: the fp16 weight d * q overflows by construction (dense_f16.hip's header); `tiny` is left out of all
                      tiers: the bounds are relative and do not model underflow.  The free-order tier has no Q4_K form (gemv_free32.hip).

One case is one launch (or one launch and its node sequence)."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import tier_model as TM
import weight_edge_cases as W
from conftest import prefill_mode

pytestmark = pytest.mark.gpu
tname = lambda t: W.TYPE_NAME[t]  # noqa: E731
MM_SHAPES = [(t, K, N) for t in W.ALL_TYPES for K, N in W.shapes_of(t)]
shape_id = lambda c: f"{tname(c[0])}-{c[1]}x{c[2]}"  # noqa: E731
TUNED_SHAPES = [c for c in MM_SHAPES if c[0] in W.TUNED]
Q32_SHAPES = [c for c in MM_SHAPES if c[0] in TM.Q32_TYPES]
EXACT3 = ("signed", "subnormal", "zero")


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def same_words(got, want, what):
    g, w = words(got), words(want)
    assert g.size == w.size, (what, g.size, w.size)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} differing words of {w.size}; (index, device, oracle): " + str([(int(i), hex(g[i]), hex(w[i])) for i in bad[:6]])


_want = {}


def oracle_mul_mat(t, profile, K, N, M):
    """the oracle's product of a case, computed once and shared, read-only"""
    key = (t, profile, K, N, M)
    if key not in _want:
        w, x = W.mat_mul_case(*key)
        y = np.zeros((M, N), np.float32)
        O.mul_mat(O.tensor(w, t, [K, N]), O.tensor(x, O.F32, [K, M]), O.tensor(y, O.F32, [N, M]))
        y.setflags(write=False)
        _want[key] = y
    return _want[key]


@pytest.fixture()
def rows32_mode(gpu):
    """gemv_rows32.hip's form: 0 = k_gemv_dec takes the launch, 2 / 4 = that many rows per wave, 1 = the launcher's pick"""
    L = gpu.lib.get()

    def set_mode(m):
        L.cllm_debug_set_gemv_rows32(int(m))
    yield set_mode
    L.cllm_debug_set_gemv_rows32(1)


@pytest.fixture()
def team32_mode(gpu):
    """gemv_team32.hip: 0 = off, 4 / 5 = that many waves per team of 8 rows, 1 = the launcher's pick"""
    L = gpu.lib.get()

    def set_mode(m):
        L.cllm_debug_set_gemv_team32(int(m))
    yield set_mode
    L.cllm_debug_set_gemv_team32(1)
    assert L.cllm_debug_gemv_team32_error() == 0, "a hand-off between the waves of a team timed out"


# ---- GET_ROWS ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", W.GET_ROWS_PROFILES)
@pytest.mark.parametrize("t,n0", [(t, n0) for t in W.ALL_TYPES + (W.F16,) for n0 in W.get_rows_widths(t)], ids=lambda v: tname(v) if v < 64 else str(v))
def test_get_rows(gpu, t, n0, profile):
    rows, n = W.GET_ROWS_SHAPE
    table, ids = W.get_rows_case(t, profile, n0)
    want = np.zeros((n, n0), np.float32)
    O.get_rows(O.tensor(table, t, [n0, rows]), O.tensor(ids, O.I32, [n]), O.tensor(want, O.F32, [n0, n]))
    assert not np.isnan(want).any()
    got = gpu.ops.get_rows(gpu.Tensor.from_numpy(table, t, [n0, rows]), gpu.Tensor.from_numpy(ids)).numpy()
    same_words(got, want, f"get_rows {tname(t)} {profile} n0 {n0}")


# ---- MUL_MAT --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", W.M_VALUES)
@pytest.mark.parametrize("profile", W.PROFILES)
@pytest.mark.parametrize("case", MM_SHAPES, ids=shape_id)
def test_mul_mat(gpu, case, profile, M):
    t, K, N = case
    w, x = W.mat_mul_case(t, profile, K, N, M)
    want = oracle_mul_mat(t, profile, K, N, M)
    got = gpu.ops.mul_mat(gpu.Tensor.from_numpy(w, t, [K, N]), gpu.Tensor.from_numpy(x)).numpy()
    same_words(got, want, f"mul_mat {tname(t)} {profile} K {K} N {N} M {M}")


# (rows32 mode, team32 mode, K, N): k_gemv_dec with both switches off at every shape; the forced forms at shapes THEIR launchers take (weight_edge_cases.ROWS32_SHAPES /
# TEAM32_SHAPES; at any other shape launch_gemv_rows32 / launch_gemv_team32 decline and k_gemv_dec would run in their name)
FORMS = [(0, 0, K, N) for K, N in W.shapes_of(W.Q4_0)] + [(r, 0, K, N) for r in (2, 4) for K, N in W.ROWS32_SHAPES] + [(0, m, K, N) for m in (4, 5) for K, N in W.TEAM32_SHAPES]


def test_the_forced_forms_have_shapes_their_launchers_take():
    """gemv_rows32.hip:183-192 (rows % rows-per-wave == 0, rows of whole dwords) and gemv_team32.hip:385-398 (rows % 8 == 0, K >= 256, (K / 32 + 7) / 8 >= team - 1)"""
    for r, m, K, N in FORMS:
        for t in TM.Q32_TYPES:
            assert (O.TYPE_SIZE[t] * (K // 32)) % 4 == 0 or (r, m) == (0, 0)
        assert r == 0 or N % r == 0
        assert m == 0 or (N % 8 == 0 and K >= 256 and (K // 32 + 7) // 8 >= m - 1)


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"rows{f[0]}-team{f[1]}-{f[2]}x{f[3]}")
@pytest.mark.parametrize("profile", W.PROFILES)
@pytest.mark.parametrize("t", TM.Q32_TYPES, ids=tname)
def test_mat_vec_every_rows32_and_team32_form(gpu, rows32_mode, team32_mode, t, profile, form):
    """one column through k_gemv_dec (both switches off), 2 / 4 rows side by side (k_gemv_rows32), and teams of 4 / 5 waves (k_gemv_team32)"""
    r, m, K, N = form
    rows32_mode(r)
    team32_mode(m)
    w, x = W.mat_mul_case(t, profile, K, N, 1)
    got = gpu.ops.mul_mat(gpu.Tensor.from_numpy(w, t, [K, N]), gpu.Tensor.from_numpy(x)).numpy()
    same_words(got, oracle_mul_mat(t, profile, K, N, 1), f"mat-vec {tname(t)} {profile} K {K} N {N} rows32 {r} team32 {m}")


# ---- the fused mat-vec -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", EXACT3)
@pytest.mark.parametrize("case", TUNED_SHAPES, ids=shape_id)
def test_fused_mat_vec_equals_the_node_sequence(gpu, case, profile):
    """RMS_NORM * weight -> quantize -> mat-vec + residual in one launch (cllm_op_mul_mat_vec_fused, prologue 1) == RMS_NORM -> MUL -> MUL_MAT -> ADD, and both the
    oracle's chain"""
    t, K, N = case
    ops, T = gpu.ops, gpu.Tensor
    wb, xh = W.mat_mul_case(t, profile, K, N, 1)
    r_ = np.random.default_rng(W.seed_of(t, profile, K, N, "fused"))
    gh, rh = (1.0 + 0.1 * r_.standard_normal(K)).astype(np.float32), r_.standard_normal(N).astype(np.float32)
    w, x, g, r = T.from_numpy(wb, t, [K, N]), T.from_numpy(xh), T.from_numpy(gh.reshape(1, K)), T.from_numpy(rh.reshape(1, N))
    nodes = ops.add(ops.mul_mat(w, ops.rms_norm_mul(x, T.from_numpy(gh), 1e-5)), r).numpy()
    out = T(gpu.F32, [N, 1])
    cw = w.c()
    gpu.lib.check(gpu.lib.get().cllm_op_mul_mat_vec_fused(None, C.byref(cw), 1, x.data_ptr(), g.data_ptr(), 1e-5, 0, r.data_ptr(), out.data_ptr()), "fused")
    xn = np.zeros_like(xh)
    O.rms_norm(O.tensor(xh, O.F32, [K, 1]), O.tensor(xn, O.F32, [K, 1]), 1e-5)
    xn = xn * gh
    want = np.zeros(N, np.float32)
    O.mul_mat(O.tensor(wb, t, [K, N]), O.tensor(xn, O.F32, [K, 1]), O.tensor(want, O.F32, [N, 1]))
    want = want + rh
    same_words(nodes, want, f"node sequence {tname(t)} {profile} K {K} N {N}")
    same_words(out.numpy(), want, f"fused mat-vec {tname(t)} {profile} K {K} N {N}")


# ---- MUL_MAT_ID --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", EXACT3)
@pytest.mark.parametrize("t", W.ALL_TYPES, ids=tname)
def test_mul_mat_id_one_token(gpu, t, profile):
    """one token, 4 experts, 2 slots: expert 0 (whose rows 0 and 1 are the all-zero ones of `zero`) and one other"""
    K, N, E = 512, 20, 4
    rng = np.random.default_rng(W.seed_of(t, profile, "id"))
    wb = W.edge_blocks(t, N * E, K, rng, profile)
    xh = rng.standard_normal((1, 1, K)).astype(np.float32)
    ids = np.array([[2, 0]], np.int32)
    want = np.zeros((1, 2, N), np.float32)
    O.mul_mat_id(O.tensor(wb, t, [K, N, E]), O.tensor(xh, O.F32, [K, 1, 1]), O.tensor(ids, O.I32, [2, 1]), O.tensor(want, O.F32, [N, 2, 1]))
    assert not np.isnan(want).any()
    got = gpu.ops.mul_mat_id(gpu.Tensor.from_numpy(wb, t, [K, N, E]), gpu.Tensor.from_numpy(xh), gpu.Tensor.from_numpy(ids)).numpy()
    same_words(got, want, f"mul_mat_id {tname(t)} {profile}")


# ---- the tolerance tiers -----------------------------------------------------------------------------------------------------------------------------
def inside(tag, got, R, bound):
    """|got - R| <= bound at every element (a bound of 0 -- an all-zero row -- demands a zero); prints the largest ratio"""
    err = np.abs(got.astype(np.float64) - R)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"TIER_RATIO {tag} {ratio:.4f}")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (tag, ratio)


@pytest.mark.parametrize("profile", EXACT3 + ("large",))
@pytest.mark.parametrize("case", TUNED_SHAPES, ids=shape_id)
def test_fast_prefill_is_inside_the_bound_at_every_element(gpu, case, profile):
    """k_mmq (prefill mode 0) at 40 columns: (n_t + 8) 2^-24 S over the float64 block terms"""
    t, K, N = case
    w, x = W.mat_mul_case(t, profile, K, N, 40)
    with prefill_mode(gpu, 0):
        got = gpu.ops.mul_mat(gpu.Tensor.from_numpy(w, t, [K, N]), gpu.Tensor.from_numpy(x)).numpy().reshape(40, N)
    R, bound = TM.fast_bound(TM.terms_matrix(t, w, TM.act_rows(O, t, x)))
    inside(f"fast {shape_id(case)} {profile}", got, R, bound)


@pytest.mark.parametrize("profile", EXACT3 + ("large",))
@pytest.mark.parametrize("case", Q32_SHAPES, ids=shape_id)
def test_free_order_mat_vec_is_inside_the_bound_at_every_element(gpu, case, profile):
    """cllm_set_decode_free_order(1), one column (Q4_0 / Q4_1 / Q8_0: the tier has no Q4_K form): the same bound"""
    t, K, N = case
    L = gpu.lib.get()
    w, x = W.mat_mul_case(t, profile, K, N, 1)
    L.cllm_set_decode_free_order(1)
    try:
        got = gpu.ops.mul_mat(gpu.Tensor.from_numpy(w, t, [K, N]), gpu.Tensor.from_numpy(x)).numpy().reshape(1, N)
    finally:
        L.cllm_set_decode_free_order(0)
    R, bound = TM.fast_bound(TM.terms_matrix(t, w, TM.act_rows(O, t, x)))
    inside(f"free {shape_id(case)} {profile}", got, R, bound)


@pytest.mark.parametrize("tile", [128, 256])
@pytest.mark.parametrize("profile", EXACT3)                          # not `large`: d * q passes 65504 and the fp16 weight is +-inf by construction
@pytest.mark.parametrize("case", TUNED_SHAPES, ids=shape_id)
def test_f16_prefill_is_inside_the_bound_at_every_element(gpu, case, profile, tile):
    """k_mmd at both tiles, 40 columns: 2 K 2^-24 sum |w16 x16| around the float64 product of the mirrored fp16 weights (tier_model.f16_weights: numpy's fp16
    arithmetic keeps subnormals; the device's packed-half staging and its matrix-core inputs keep them too, or `subnormal` would miss this bound)"""
    t, K, N = case
    w, x = W.mat_mul_case(t, profile, K, N, 40)
    lib = C.CDLL(gpu.lib.SO_PATH)
    lib.cllm_debug_set_prefill_f16(1)
    lib.cllm_debug_set_mmd_tile(tile)
    try:
        with prefill_mode(gpu, 0):
            got = gpu.ops.mul_mat(gpu.Tensor.from_numpy(w, t, [K, N]), gpu.Tensor.from_numpy(x)).numpy().reshape(40, N)
    finally:
        lib.cllm_debug_set_prefill_f16(0)
        lib.cllm_debug_set_mmd_tile(0)
    R, bound = TM.f16_bound(t, w, x)
    inside(f"f16-{tile} {shape_id(case)} {profile}", got, R, bound)
