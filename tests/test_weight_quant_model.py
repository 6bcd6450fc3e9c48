"""Settles, on the CPU and before any kernel runs, the bytes the weight quantizers must write (from_float_ref of Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q4_K and F16:
what cllm_op_quantize_rows promises) on the cases of tests/weight_quant_cases.py: the oracle (oracle/ggml_oracle.c, orc_quantize_row_ref) against the reference
build, an independent numpy float32 mirror of the five 32-weight quantizers against the oracle, and assertions that the catalogue reaches the branches it names.
Skipped where oracle/_ref has not been built (the mirror and coverage tests need only the oracle and run everywhere).

What it found.  The reference converts with (int8_t)(x * id + 8.5f), (uint8_t)(x * id + 0.5f) and an implicit float -> int8_t of roundf(x * id).  id = 1 / d is
inf for every block whose scale is below 2^-128 in magnitude (Q8_0: a block maximum below 3.73e-37; Q4_0: below 2.35e-38; Q5_0: below 4.70e-38; Q4_1 / Q5_1: a
range below 4.41e-38 / 9.11e-38), the products are then +-inf and, for the block's zeros and its minimum, NaN, and C leaves those conversions to the compiler.
The reference build (gcc, x86-64-v3) truncates with cvttss2si / cvttps2dq to int32 and keeps the low byte: NaN and +-inf give 0x80000000, low byte 0.  So EVERY
quant of such a block is 0 -- Q8_0: 32 bytes 0x00; Q4_0 / Q4_1: 16 bytes 0x00 (not the 0x88 of an all-zero Q4_0 block); Q5_0 / Q5_1: qh 00 00 00 00 and 16
bytes 0x00 -- behind a stored scale of fp16 +-0 (0x8000 where Q4_0 / Q5_0 divide a positive maximum by -8 / -16) and, for the offset formats, the fp16 of the
minimum.  The same holds where max - min overflows (+-3e38 in one block of Q4_1 / Q5_1): d = inf, id = 0, (x - min) * 0 is NaN for the infinite differences
and 0 for the rest, all quants 0, stored d 0x7c00.  The oracle agreed already, through the same conversion of its own compiler; it now spells the conversion out
(cast_i8 / cast_u8).  An all-zero block stores d = -0.0 for Q4_0 / Q5_0 (0.0f / -8).

F16: the oracle's conversion equals numpy's and the reference's on every non-NaN float tried (all halves, all midpoints and their neighbours, the thresholds).
For NaNs the reference build writes 0x7e00 with the sign, whatever the payload; the oracle keeps the top ten payload bits and sets the quiet bit (9 of the 2058
NaNs of the catalogue agree).  The contract asked of the device is only `a NaN of the same sign`, which is what this file asks of both."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import weight_quant_cases as W

F = np.float32
needs_ref = pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref not built")
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
ids = lambda t: W.NAME[t]  # noqa: E731


def ref_quantize(t, x):
    x = np.ascontiguousarray(x, F)
    y = np.full(O.TYPE_SIZE[t] * (x.size // O.BLCK[t]), 0xA5, np.uint8)
    assert O.ref().ref_quantize_ref(t, P(x), P(y), C.c_int64(x.size)) == 0
    return y


def all_cases(t):
    """[(name, float32[rows, K])]: the special blocks and every geometry at every scale"""
    if t == O.F16:
        return [(k, v.reshape(1, -1)) for k, v in W.f16_cases().items() if k != "nan"]
    out = [("special", W.special_case(t)[1])]
    for nb, layout in W.geometry_ids(t):
        for s in W.SCALES:
            out.append((f"{nb}_{layout}_{s:g}", W.geometry(t, nb, layout, s)[0]))
    return out


def first_difference(t, got, want, names=None):
    bad = np.flatnonzero(got != want)
    if not bad.size:
        return None
    b, o = divmod(int(bad[0]), O.TYPE_SIZE[t])
    return f"{bad.size} bytes differ; first: block {b}{' (' + names[b] + ')' if names else ''} offset {o}: got {got[bad[0]]:#04x} want {want[bad[0]]:#04x}"


def same_sign_nans(halves, x):
    h = np.ascontiguousarray(halves).view(np.uint16)
    return bool(((h & 0x7c00) == 0x7c00).all() and ((h & 0x03ff) != 0).all() and np.array_equal(h >> 15, x.view(np.uint32) >> 31))


# ---- the numpy mirror -----------------------------------------------------------------------------------------------------------------
def mirror(t, x, first_max=True, clamp=True):
    """from_float_ref of the 32-weight types and F16 in numpy float32, one rounding per written operation, np.float16 for the stored fields; a conversion of a
    non-finite product gives quant 0 (the reference build's bytes, see the module docstring).  first_max=False: the LAST element of largest magnitude decides
    (amax <= a); clamp=False: without MIN(15, .) / MIN(31, .) -- both only to show that the catalogue tells them apart"""
    if t == O.F16:
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(x, F).reshape(-1).astype(np.float16).view(np.uint8)
    x = np.ascontiguousarray(x, F).reshape(-1, 32)
    n = len(x)
    out = np.zeros((n, O.TYPE_SIZE[t]), np.uint8)
    signed = t in W.SIGNED_TYPES
    with np.errstate(all="ignore"):
        if signed:
            amax, mx = np.zeros(n, F), np.zeros(n, F)
            for j in range(32):
                a = np.abs(x[:, j])
                up = amax < a if first_max else amax <= a
                amax, mx = np.where(up, a, amax), np.where(up, x[:, j], mx)
            d = amax / F(127) if t == O.Q8_0 else mx / F(-8) if t == O.Q4_0 else mx / F(-16)
            sub = x
        else:
            mn, hi = np.full(n, np.finfo(F).max, F), np.full(n, -np.finfo(F).max, F)
            for j in range(32):
                mn, hi = np.where(x[:, j] < mn, x[:, j], mn), np.where(x[:, j] > hi, x[:, j], hi)
            d = (hi - mn) / F(15 if t == O.Q4_1 else 31)
            sub = x - mn[:, None]
            out[:, 2:4] = mn.astype(np.float16).view(np.uint8).reshape(n, 2)
        ident = np.where(d != 0, F(1) / d, F(0)).astype(F)
        out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(n, 2)
        v = sub * ident[:, None]
        assert v.dtype == F
        if t == O.Q8_0:
            r = np.trunc(v)
            r = r + np.where(np.abs(v - r) >= F(0.5), np.sign(v), F(0))          # roundf: halves away from zero (v - r is exact)
            q = np.where(np.isfinite(v), r, F(0)).astype(np.int32)
            out[:, 2:] = (q & 0xff).astype(np.uint8)
            return out.reshape(-1)
        five = t in (O.Q5_0, O.Q5_1)
        v = v + F((16.5 if five else 8.5) if signed else 0.5)
        q = np.where(np.isfinite(v), np.trunc(v), F(0)).astype(np.int32)
        if clamp and t != O.Q5_1:
            q = np.minimum(q, 31 if five else 15)
        q0, q1 = q[:, :16], q[:, 16:]
        o = 2 if signed else 4
        if five:
            bit = ((q >> 4) & 1).astype(np.uint32)
            qh = (bit << np.arange(32, dtype=np.uint32)).sum(axis=1).astype(np.uint32)
            out[:, o:o + 4] = qh.view(np.uint8).reshape(n, 4)
            out[:, o + 4:] = ((q0 & 0xF) | ((q1 & 0xF) << 4)).astype(np.uint8)
        else:
            out[:, o:] = ((q0 | (q1 << 4)) & 0xff).astype(np.uint8)              # xi0 | xi1 << 4 as the reference writes it: no mask
    return out.reshape(-1)


def scale_and_class(t, x):
    """per block: (d as the type computes it, whether 1 / d overflows, the block maximum or range) -- the overflow class, decided without any quantizer"""
    x = np.ascontiguousarray(x, F).reshape(-1, 32)
    with np.errstate(all="ignore"):
        if t in W.SIGNED_TYPES:
            size = np.abs(x).max(axis=1)
        else:
            size = x.max(axis=1) - x.min(axis=1)
        d = size / F(W.DIVISOR[t])
        return d, (d != 0) & np.isinf(F(1) / d), size


# ---- the oracle against the reference ---------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("t", W.TYPES, ids=ids)
def test_oracle_equals_the_reference(t):
    names = W.special_case(t)[0] if t != O.F16 else None
    for name, x in all_cases(t):
        got, want = O.quantize_ref(t, x), ref_quantize(t, x)
        diff = first_difference(t, got, want, names if name == "special" else None)
        assert diff is None, f"{W.NAME[t]} {name}: {diff}"
    if t == O.F16:
        x = W.f16_cases()["nan"]
        assert same_sign_nans(ref_quantize(t, x), x) and same_sign_nans(O.quantize_ref(t, x), x)


@needs_ref
@pytest.mark.parametrize("t", W.B32_TYPES, ids=ids)
def test_the_reference_writes_zero_quants_where_the_inverse_scale_overflows(t):
    """from the reference alone: every quant of a block with 0 < |d| and 1 / d == inf is 0 and its stored scale is fp16 +-0; one binade up the quants are ordinary.
    The same bytes where max - min overflows (Q4_1 / Q5_1)"""
    names, x = W.special_rows()
    d, ovf, size = scale_and_class(t, x)
    tiny = np.finfo(F).tiny
    assert ovf.sum() >= 3 and (size[ovf] < tiny).sum() >= 2 and (size[ovf] >= tiny).sum() >= 1
    out = ref_quantize(t, x).reshape(len(x), -1)
    o = 2 if t in W.SIGNED_TYPES else 4
    assert not out[ovf, o:].any(), [names[i] for i in np.flatnonzero(ovf) if out[i, o:].any()]
    assert ((out[ovf, 0:2].copy().view(np.uint16) & 0x7fff) == 0).all()
    control = ~ovf & (d != 0) & (size < 4 * W.THRESHOLD[t])
    assert control.sum() >= 1 and out[control, o:].any(axis=1).all(), [names[i] for i in np.flatnonzero(control)]
    issue = out[names.index("sub_issue")]
    assert issue.tobytes() == {O.Q8_0: bytes(34), O.Q4_0: b"\x00\x80" + bytes(16), O.Q5_0: b"\x00\x80" + bytes(20),
                               O.Q4_1: b"\x00\x00\x00\x80" + bytes(16), O.Q5_1: b"\x00\x00\x00\x80" + bytes(20)}[t]
    if t in (O.Q4_1, O.Q5_1):
        huge = out[names.index("huge_pm")]
        assert huge.tobytes() == b"\x00\x7c\x00\xfc" + bytes(len(huge) - 4)


# ---- the mirror against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", W.B32_TYPES + (O.F16,), ids=ids)
def test_numpy_mirror_equals_the_oracle(t):
    names = W.special_rows()[0]
    for name, x in all_cases(t):
        diff = first_difference(t, mirror(t, x), O.quantize_ref(t, x), names if name == "special" else None)
        assert diff is None, f"{W.NAME[t]} {name}: {diff}"


# ---- the catalogue reaches what it names --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", W.B32_TYPES, ids=ids)
def test_catalogue_reaches_every_branch_of_the_block_quantizers(t):
    names, x = W.special_rows()
    at = names.index
    want = mirror(t, x).reshape(len(x), -1)
    d, ovf, size = scale_and_class(t, x)
    # the overflow class: at least three blocks below the threshold (subnormal and normal), one control just above it; none of it in the Gaussian rows
    below = [n for n in names if n.startswith(f"ovf_{W.NAME[t]}_") and n.split("_")[-1] in ("below", "neg", "quarter", "at") and "above" not in n]
    assert len(below) >= 3 and all(ovf[at(n)] for n in below)
    assert not ovf[at(f"ovf_{W.NAME[t]}_above")] and not ovf[at(f"ovf_{W.NAME[t]}_above_neg")]
    blk = x[ovf]
    assert (blk > 0).any() and (blk < 0).any() and (blk == 0).any()
    # d == 0: id = 0
    assert (d == 0).sum() >= 2 and size[at("sub_smallest")] > 0 and (d[at("sub_smallest")] == 0 or t in (O.Q4_1, O.Q5_1))
    # the stored scale on every fp16 edge (and, offset formats, a minimum past fp16 next to a finite scale and the reverse)
    for i, (_, half) in enumerate(W.D_EDGES):
        got = int(want[at(f"d_edge_{W.NAME[t]}_{i}"), 0:2].copy().view(np.uint16)[0])
        assert got == half, (i, hex(got), hex(half))
    if t in (O.Q4_1, O.Q5_1):
        a, b = want[at("m_inf_d_finite")], want[at(f"d_inf_m_finite_{W.NAME[t]}")]
        assert a[2:4].tobytes() == b"\x00\xfc" and 0 < a[0:2].copy().view(np.float16)[0] <= 1.0
        assert b[0:2].tobytes() == b"\x00\x7c" and np.isfinite(b[2:4].copy().view(np.float16)[0])
    # the tie rule and the clamp (the signed 4- and 5-bit formats: Q8_0 has neither, and (x - min) * id + 0.5 of the offset formats never reaches 16 / 32)
    if t in (O.Q4_0, O.Q5_0):
        last = mirror(t, x, first_max=False).reshape(len(x), -1)
        changed = {names[i] for i in np.flatnonzero((last != want).any(axis=1))}
        ties = {f"tie_{o}_{h}" for o in ("pn", "np") for h in ("lo", "hi", "cross")} | {"clamp_neg_max"}
        assert ties <= changed
        loose = mirror(t, x, clamp=False).reshape(len(x), -1)
        changed = {names[i] for i in np.flatnonzero((loose != want).any(axis=1))}
        assert ties <= changed and "one_neg_at_0" not in changed       # the second of two opposite maxima lands on 16.5 (32.5) whichever sign came first; a lone maximum on 0.5
    else:
        assert np.array_equal(mirror(t, x, clamp=False), want.reshape(-1))
    # exact integers and exact halves
    if t == O.Q8_0:
        g = want[at("grid_q8_0_id1"), 2:].view(np.int8)
        assert g[0] == 127 and g[17] == 1 and g[15] == -1 and g[21] == 3 and g[11] == -3 and g[16] == 0      # 0.5 -> 1, -0.5 -> -1, 2.5 -> 3, -2.5 -> -3: away from zero
    if t == O.Q4_0:
        g = want[at("grid_q4_0_d1"), 2:]
        assert (g[1] & 0xF) == 1 and (g[2] & 0xF) == 1 and (g[1] >> 4) == 9          # -7.5 + 8.5 = 1 exactly; -7 + 8.5 = 1.5 -> 1; 0.5 + 8.5 = 9


def test_catalogue_reaches_the_q4_K_paths():
    names, x = W.special_case(O.Q4_K)
    at = names.index
    d, dmin, sc, m, nib = W.q4k_fields(O.quantize_ref(O.Q4_K, x))
    # a decoded scale of 0 keeps the quants of the sub-block's own search: at 0, 3 (whole-byte codes) and 4, 7 (split codes)
    for pos in W.Q4K_PATH3_POSITIONS:
        i = at(f"tiny_range_at_{pos}")
        assert d[i] > 0 and sc[i, pos] == 0 and nib[i, pos].any() and nib[i, pos].max() > 1, pos
    i = at("code63_scale_and_min")
    assert sc[i, 2] == 63 and m[i, 2] == 63 and (sc[i] == 63).sum() == 1 and (m[i] == 63).sum() == 1
    for n in ("all_pos_grid", "all_pos_gauss"):
        assert d[at(n)] > 0
    assert dmin[at("all_pos_grid")] == 0 and not m[at("all_pos_grid")].any()               # max_min == 0: inv_min == 0
    i = at("eight_const")
    assert d[i] > 0 and dmin[i] > 0
    # sum_x2 overflows
    with np.errstate(over="ignore"):
        assert np.isinf((x.reshape(-1, 32) ** 2).sum(axis=1, dtype=F)).sum() >= 3


def test_catalogue_geometries_cross_the_workgroup_boundary():
    for t in W.B32_TYPES + (O.Q4_K,):
        per = W.PER_WORKGROUP[t]
        counts = W.BLOCK_COUNTS[t]
        assert 1 in counts and {per - 1, per, per + 1} <= set(counts) and max(counts) > 2 * per
        for nb in counts:
            x, laid = W.geometry(t, nb, "rows", 1.0)
            assert x.shape == (nb, O.BLCK[t]) and 0 in laid and nb - 1 in laid
            if nb > per:
                assert {per - 1, per} <= set(laid)
            assert W.geometry(t, nb, "row", 1.0)[0].shape == (1, nb * O.BLCK[t])
    f = W.f16_cases()
    assert f["all_halves"].size == 65536 - 2046 and f["midpoints"].size == 2 * 3 * 0x7bff and np.isnan(f["nan"]).all()


# ---- dequantization ---------------------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("t", W.TYPES, ids=ids)
def test_dequantized_rows_equal_the_reference(t):
    """O.dequantize of the oracle's bytes == the reference's to_float of the same bytes, word for word (F16: numpy's exact widening stands in for the oracle,
    which has no F16 row dequantizer)"""
    for name, x in all_cases(t):
        raw = O.quantize_ref(t, x)
        got = W.dequantize_expected(t, raw, x.size)
        want = np.zeros(x.size, F)
        assert O.ref().ref_dequantize(t, P(raw), P(want), C.c_int64(x.size)) == 0
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"{W.NAME[t]} {name}: element {int(bad[0])}: {got[bad[0]]!r} != {want[bad[0]]!r}"


@pytest.mark.parametrize("t", W.TYPES, ids=ids)
def test_round_trip_rows_decode_without_nan(t):
    """the device's round trip is compared word for word, so its expected words must not depend on a processor's NaN"""
    x = W.round_trip_case(t)
    assert x.shape[0] == 3 and x.shape[1] % O.BLCK[t] == 0
    want = W.dequantize_expected(t, O.quantize_ref(t, x), x.size)
    assert np.isfinite(want).all() and np.abs(want - x.reshape(-1)).max() <= 1.0       # one quantization step at the most; the largest |d| of these rows is 1 (grid_q4_0_d1)
