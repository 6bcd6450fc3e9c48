"""CPU: the oracle (oracle/ggml_oracle.c) against the reference build (oracle/_ref) on the blocks of tests/weight_edge_cases.py -- negative, fp16-subnormal, zero and
maximal scale fields, saturated quants, and activations so small that the scale products are fp32 subnormals -- for all 22 block formats: dequantize, vec_dot,
mul_mat at 1, 5 and 40 columns and get_rows, word for word.  Skipped where oracle/_ref is not built.

It also asserts what tests/test_gpu_weight_edges.py rests on: NO word of any reference output here is a NaN, and infinities occur only in MXFP4's `large` GET_ROWS
table (exponent bytes up to 255) -- so the device tests compare whole buffers as uint32 with no exemption.  And it checks its own inputs: per profile the bytes
built hold negative, subnormal, zero and maximal fields; under `tiny` a tenth of the reference's own output words of every Q8_K-activation case are nonzero fp32
subnormals (the formats with fp16 activation scales put out +-0 only: the scale rounds to zero), and a tenth of a type's float64 products lie below 2^-126."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import tier_model as TM
import weight_edge_cases as W

pytestmark = pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref not built")

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
tname = lambda t: W.TYPE_NAME[t]  # noqa: E731
MM_PROFILES = W.PROFILES

# the oracle's restatement of the reference build's (x86, AVX2) dot product of each type
VEC_DOT = {W.Q4_0: "orc_vec_dot_q4_0_q8_0_avx2", W.Q8_0: "orc_vec_dot_q8_0_q8_0_avx2", W.Q4_1: "orc_vec_dot_q4_1_q8_1_avx2", W.Q4_K: "orc_vec_dot_q4_K_q8_K_avx2",
           W.Q5_K: "orc_vec_dot_q5_K_q8_K_avx2", W.Q6_K: "orc_vec_dot_q6_K_q8_K_avx2", W.Q5_0: "orc_vec_dot_q5_0_q8_0_avx2", W.Q5_1: "orc_vec_dot_q5_1_q8_1_avx2",
           W.IQ4_NL: "orc_vec_dot_iq4_nl_q8_0_avx2", W.MXFP4: "orc_vec_dot_mxfp4_q8_0_avx2", W.Q2_K: "orc_vec_dot_q2_K_q8_K_avx2", W.Q3_K: "orc_vec_dot_q3_K_q8_K_avx2",
           W.IQ4_XS: "orc_vec_dot_iq4_xs_q8_K_avx2", W.TQ1_0: "orc_vec_dot_tq1_0_q8_K_avx2", W.TQ2_0: "orc_vec_dot_tq2_0_q8_K_avx2",
           W.IQ1_S: "orc_vec_dot_iq1_s_q8_K_avx2", W.IQ1_M: "orc_vec_dot_iq1_m_q8_K_avx2"}
GRID = (W.IQ2_XXS, W.IQ2_XS, W.IQ2_S, W.IQ3_XXS, W.IQ3_S)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def same_words(got, ref, what):
    g, r = words(got), words(ref)
    bad = np.flatnonzero(g != r)
    assert bad.size == 0, f"{what}: {bad.size} differing words of {r.size}; (index, oracle, reference): " + str([(int(i), hex(g[i]), hex(r[i])) for i in bad[:6]])


def finite(ref, what, inf_ok=False):
    assert not np.isnan(ref).any(), f"{what}: the reference's output holds a NaN"
    assert inf_ok or not np.isinf(ref).any(), f"{what}: the reference's output holds an infinity"


def act_row(t, x):
    return O.quantize_q8_K(x) if O.BLCK[t] == 256 else O.quantize_q8_1(x) if t in (W.Q4_1, W.Q5_1) else O.quantize_q8_0(x)


def oracle_vec_dot(t, K, w, a):
    f = getattr(O.lib(), VEC_DOT.get(t, "orc_vec_dot_iq_grid_q8_K_avx2"))
    f.restype = C.c_float
    f.argtypes = ([C.c_int] if t in GRID else []) + [C.c_int64, C.c_void_p, C.c_void_p] + ([C.c_int] if t == W.IQ4_NL else [])
    args = ([C.c_int(t)] if t in GRID else []) + [C.c_int64(K), P(w), P(a)] + ([C.c_int(0)] if t == W.IQ4_NL else [])
    return np.float32(f(*args))


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", W.ALL_TYPES, ids=tname)
def test_only_the_scale_fields_differ_from_rand_blocks(t):
    """edge_blocks is rand_blocks with other scale fields (saturated: the same scale fields, other bytes); the field table reads back what rand_blocks wrote"""
    K, rows = 512, 7
    base = W.rand_blocks(t, rows, K, np.random.default_rng(5))
    f0 = W.get_fields(t, base, K)
    if t != W.MXFP4:
        assert np.all(f0[..., 0] >= 0x1800) and np.all(f0[..., 0] < 0x2400), "rand_blocks' d is a positive normal fp16 number around 0.01"
    for profile in W.PROFILES:
        e = W.edge_blocks(t, rows, K, np.random.default_rng(5), profile)
        assert e.shape == base.shape and e.dtype == np.uint8
        if profile == "saturated":
            assert np.array_equal(W.get_fields(t, e, K), f0)
            continue
        back = e.copy()
        W.put_fields(t, back, K, f0)
        assert np.array_equal(back, base), profile


@pytest.mark.parametrize("profile", W.PROFILES)
@pytest.mark.parametrize("t", W.ALL_TYPES, ids=tname)
def test_a_profile_holds_what_it_is_named_for(t, profile):
    for K, N in W.shapes_of(t):
        w, _ = W.mat_mul_case(t, profile, K, N, 1)
        nb = K // O.BLCK[t]
        v = W.get_fields(t, w, K)
        if t == W.MXFP4:
            if profile in ("subnormal", "tiny"):
                assert np.all(v <= 3) and all(np.all((v[:, :, 0] == e).any(1)) for e in (0, 1, 3))
            if profile == "large":
                assert np.all(v[:, 0, 0] == 200) and v.max() == 200 and v.min() >= 124
            continue
        neg, mag = v >> 15, v & 0x7fff
        if profile == "signed":
            assert np.all(neg[:, 0] == 0) and np.all(neg[:, 1] == 1)                        # both signs in every row and in its first pair of blocks
            assert np.all(mag >= 0x1800) or t in (W.Q4_1, W.Q5_1)
        if profile in ("subnormal", "tiny"):
            assert ((mag > 0) & (mag < 0x400)).any() and neg.any()
            for r in range(N if profile == "subnormal" else 0):
                near = [r] if nb >= 3 else list(range(min(r, N - 3), min(r, N - 3) + 3))          # two blocks a row: any three neighbouring rows
                have = set(int(m) for m in mag[near].reshape(-1))
                assert set(W.FORCED_SUB) <= have, (r, sorted(have)[:4])
            if profile == "subnormal":
                normal = float((mag >= 0x400).mean())
                assert 0.25 <= normal <= 0.8 or nb == 3, normal                              # about half of the blocks keep a normal scale (K = 96: the three forced ones)
            else:
                assert np.all(mag[0::3] <= 3) and np.all(mag[0::3] >= 1)
        if profile == "zero":
            assert np.all(mag[0] == 0) and np.all(mag[1, : nb - 1] == 0) and np.all(mag[1, nb - 1] != 0)
            assert ((v == 0).sum() > 0) and ((v == 0x8000).sum() > 0) and 0.45 <= float((mag == 0).mean()) <= 0.9
            if W.n_fields(t) == 2:
                assert np.any((mag[..., 0] == 0) & (mag[..., 1] != 0)) and np.any((mag[..., 0] != 0) & (mag[..., 1] == 0))
        if profile == "large":
            assert np.all(v[:, 0] == 0x7bff) and np.all(v[:, 1] == 0xfbff) and mag.max() == 0x7bff and mag.min() >= 0x6400
    # the F16 tables of GET_ROWS
    if t == W.ALL_TYPES[0] and profile in W.GET_ROWS_PROFILES:
        tab = W.get_rows_case(W.F16, profile, 512)[0].view(np.uint16)
        m = tab & 0x7fff
        assert not np.any(m >= 0x7c00)
        assert {"signed": (tab >> 15).any(), "subnormal": ((m > 0) & (m < 0x400)).any() and (m == 0x400).any(), "zero": (tab == 0).any() and (tab == 0x8000).any(),
                "large": (tab == 0x7bff).any() and (tab == 0xfbff).any(), "saturated": (m == 0x7bff).any()}[profile]


@pytest.mark.parametrize("t", W.ALL_TYPES, ids=tname)
def test_saturated_blocks_decode_to_the_largest_integers(t):
    """what `saturated` promises, read off the oracle's dequantized rows: with the scale fields set to 1.0 (MXFP4: 2^0) every |weight| of a block is one value, the
    format's largest (blocks in turn where two patterns exist) -- and every Q8 quant of the activations is +-127"""
    K = 512
    w = W.edge_blocks(t, 4, K, np.random.default_rng(3), "saturated").copy()
    one = np.full((4, K // O.BLCK[t], W.n_fields(t)), 0x3c00 if t != W.MXFP4 else 127, np.uint16)
    if W.n_fields(t) == 2:
        one[..., 1] = 0                                           # the minimum off: the integer times d alone
    W.put_fields(t, w, K, one)
    want = {W.Q4_0: (7, 8), W.Q4_1: (15,), W.Q5_0: (15, 16), W.Q5_1: (31,), W.Q8_0: (127, 128), W.Q4_K: (15 * 63,), W.Q5_K: (31 * 63,), W.Q2_K: (3 * 15,),
            W.Q3_K: (3 * 31, 4 * 32), W.Q6_K: (31 * 128, 31 * 127, 32 * 128, 32 * 127), W.IQ4_NL: (113, 127), W.IQ4_XS: (113 * 31, 127 * 32), W.MXFP4: (6,), W.TQ1_0: (1,), W.TQ2_0: (1,)}
    for r in range(4):
        y = np.abs(O.dequantize(t, w[r], K)).reshape(-1, 16 if t == W.Q6_K else O.BLCK[t])
        if t in want:
            assert set(np.unique(y).tolist()) <= set(float(v) for v in want[t]), (np.unique(y)[:6], want[t])
        assert np.all(y > 0)
    x = W.activations(t, 3, K, np.random.default_rng(4), "saturated")
    for row in x:
        a = act_row(t, row)
        q = (TM.decode_q8_K(a) if O.BLCK[t] == 256 else TM.decode_q8_1(a) if t in (W.Q4_1, W.Q5_1) else TM.decode_q8_0(a))["q"]
        assert np.all(np.abs(q) == 127)                           # (Q8_K's quants are all -127: its block scale carries the sign)
    if t == W.Q4_K:                                               # the super-block's integer sum sum_b sc[b] s_b, from the bytes built: past 2^24
        wd, ad = TM.decode_q4_K(w), TM.decode_q8_K(np.stack([act_row(t, row) for row in x]))
        isum = np.einsum("nsbj,msbj->mns", wd["q"] * wd["sc"][..., None], ad["q"].reshape(3, -1, 8, 32))
        assert np.all(np.abs(isum) == 256 * 15 * 127 * 63) and 256 * 15 * 127 * 63 > 2 ** 24


# ---- dequantize ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", W.GET_ROWS_PROFILES)
@pytest.mark.parametrize("t", W.ALL_TYPES, ids=tname)
def test_dequantize(t, profile):
    R = O.ref()
    for K, N in W.shapes_of(t):
        w, _ = W.mat_mul_case(t, profile, K, N, 1)
        for r in range(N):
            ref = np.zeros(K, np.float32)
            assert R.ref_dequantize(t, P(w[r]), P(ref), C.c_int64(K)) == 0
            finite(ref, f"dequantize {tname(t)} {profile}")
            same_words(O.dequantize(t, w[r], K), ref, f"dequantize {tname(t)} {profile} K {K} row {r}")


# ---- vec_dot -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", MM_PROFILES)
@pytest.mark.parametrize("t", W.ALL_TYPES, ids=tname)
def test_vec_dot(t, profile):
    R = O.ref()
    s = C.c_float()
    for K, N in W.shapes_of(t):
        w, x = W.mat_mul_case(t, profile, K, N, 1)
        a = act_row(t, x[0])
        for r in range(N):
            assert R.ref_vec_dot(t, C.c_int64(K), P(w[r]), P(a), C.byref(s)) == 0
            ref = np.float32(s.value)
            finite(np.array([ref]), f"vec_dot {tname(t)} {profile}")
            got = oracle_vec_dot(t, K, w[r], a)
            assert got.view(np.uint32) == ref.view(np.uint32), (tname(t), profile, K, r, float(got), float(ref))


# ---- mul_mat ---------------------------------------------------------------------------------------------------------------------------------------
def float64_product(t, w, x, K):
    wf = TM.dequant64(t, w) if t in W.TUNED else np.stack([O.dequantize(t, r, K) for r in w]).astype(np.float64)
    return x.astype(np.float64) @ wf.T


@pytest.mark.parametrize("profile", MM_PROFILES)
@pytest.mark.parametrize("t", W.ALL_TYPES, ids=tname)
def test_mul_mat(t, profile):
    R = O.ref()
    below = total = 0
    for K, N in W.shapes_of(t):
        for M in W.M_VALUES:
            w, x = W.mat_mul_case(t, profile, K, N, M)
            ref = np.zeros((M, N), np.float32)
            assert R.ref_mul_mat(t, C.c_int64(K), C.c_int64(N), C.c_int64(M), C.c_int64(1), C.c_int64(1), P(w), P(x), P(ref)) == 0
            finite(ref, f"mul_mat {tname(t)} {profile} {K} {N} {M}")
            got = np.zeros((M, N), np.float32)
            O.mul_mat(O.tensor(w, t, [K, N]), O.tensor(x, O.F32, [K, M]), O.tensor(got, O.F32, [N, M]))
            same_words(got, ref, f"mul_mat {tname(t)} {profile} K {K} N {N} M {M}")
            if profile == "tiny":
                v = np.abs(float64_product(t, w, x, K))
                below += int((v < 2.0 ** -126).sum())
                total += v.size
                assert np.all(v < 2.0 ** -100)
                # what the reference actually put out, not the float64 value: nonzero fp32 subnormals in a tenth of the words of EVERY case where the
                # activation scale is an fp32 (Q8_K); all +-0 where it is an fp16 that rounds to zero (weight_edge_cases.tiny_activations)
                a = np.abs(ref)
                if t in W.ACT_FP16_SCALE:
                    assert np.all(a == 0), (tname(t), K, N, M, float(a.max()))
                else:
                    sub = int(((a > 0) & (a < 2.0 ** -126)).sum())
                    assert sub * 10 >= a.size, (tname(t), K, N, M, sub, a.size)
    if profile == "tiny":
        assert below * 10 >= total, (below, total)


# ---- get_rows ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", W.GET_ROWS_PROFILES)
@pytest.mark.parametrize("t", W.ALL_TYPES + (W.F16,), ids=tname)
def test_get_rows(t, profile):
    R = O.ref()
    rows, n = W.GET_ROWS_SHAPE
    for n0 in W.get_rows_widths(t):
        table, ids = W.get_rows_case(t, profile, n0)
        ref = np.zeros((n, n0), np.float32)
        assert R.ref_get_rows(t, C.c_int64(n0), C.c_int64(rows), P(table), C.c_int64(n), P(ids), P(ref)) == 0
        finite(ref, f"get_rows {tname(t)} {profile}", inf_ok=(t == W.MXFP4 and profile == "large"))
        if t == W.MXFP4 and profile == "large":
            assert np.isinf(ref).any() and (ref == np.inf).any() and (ref == -np.inf).any()
        got = np.zeros_like(ref)
        O.get_rows(O.tensor(table, t, [n0, rows]), O.tensor(ids, O.I32, [n]), O.tensor(got, O.F32, [n0, n]))
        same_words(got, ref, f"get_rows {tname(t)} {profile} n0 {n0}")
