"""Settles SET_ROWS (into F32, F16 and Q8_0), CPY / CONT, GET_ROWS and SOFT_MAX with a mask on the CPU, before any kernel runs: the C restatement the
other tests lean on (oracle/ggml_oracle.c: orc_set_rows, orc_cpy, orc_get_rows, orc_soft_max) against the reference's own CPU backend driven through its
public ggml API (tests/ref_ggml.py), byte for byte, at the cases tests/test_gpu_datamove.py runs on the device (tests/datamove_cases.py).  Whole
destination buffers are compared, so a store outside the addressed rows fails.  Skipped where oracle/_ref has not been built.

What it found: the reference's quantize_row_q8_0 (the x86 branch) multiplies by 127 / amax even where that quotient overflows to inf -- amax below 3.74e-37,
every subnormal included.  The products are +-inf and, for the block's zeros, NaN; _mm256_cvtps_epi32 makes 0x80000000 of all of them and the two
saturating packs make -128: the block's 32 quants are all 0x80 (its scale rounds to fp16 0).  The oracle's (int) nearbyintf gave 0 there.

The idx and the mask buffers carry a tail behind the tensor, so a restatement whose broadcast is wrong reads something, not past the buffer."""
import numpy as np
import pytest

import datamove_cases as D
import oracle as O
import ref_ggml as R

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")


def otensor(buf, view):
    ne, nb = view.final()
    return O.tensor(buf, view.type, ne, nb, view.offset)


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got).reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} differing bytes of {want.size}; (offset, got, reference): " + str([(int(i), hex(got[i]), hex(want[i])) for i in bad[:8]])


SET_ROWS = D.set_rows_cases() + D.set_rows_q8_0_cases()


@pytest.mark.parametrize("case", SET_ROWS, ids=repr)
def test_set_rows(case):
    dst0, dv, src, sv, idx, idx_buf = case.build()
    want = R.set_rows(dst0, dv, src, sv, idx)
    got, srcw, ib = np.array(dst0), np.array(src), np.array(idx_buf)
    ine = list(reversed(idx.shape))
    O.set_rows(otensor(srcw, sv), O.tensor(ib, case.idx_type, ine), otensor(got, dv))
    same_bytes(got, want, f"set_rows {case}")
    rows_written = case.src_ne[1] * case.src_ne[2] * case.src_ne[3]
    changed = int((D.gather(want, dv) != D.gather(dst0, dv)).any(axis=-1).sum())
    assert changed <= rows_written and (changed > 0 or rows_written == 0)
    mask = np.ones(dst0.size, bool)
    mask[D.gather(np.arange(dst0.size), dv).reshape(-1)] = False
    assert np.array_equal(want[mask], dst0[mask])                   # the reference itself leaves the bytes between and around the rows alone


def test_the_reference_saturates_a_block_whose_inverse_scale_overflows():
    """from the reference alone: every quant of a block with 0 < amax < 127 / FLT_MAX is -128, its stored scale 0; one binade up the quants are ordinary"""
    x = D.q8_special_blocks()
    amax = np.abs(x).max(axis=1)
    with np.errstate(over="ignore", divide="ignore"):
        tiny = (amax > 0) & np.isinf(np.float32(127.0) / amax)
    assert tiny.sum() >= 3 and (amax[tiny] < np.finfo(np.float32).tiny).sum() >= 2 and (amax[tiny] >= np.finfo(np.float32).tiny).sum() >= 1
    n = len(x)
    out = R.set_rows(np.zeros(n * 34, np.uint8), R.View(D.Q8_0, [32, n]), x, R.View(D.F32, [32, n]), np.arange(n, dtype=np.int64)).reshape(n, 34)
    assert (out[tiny, 2:] == 0x80).all() and (out[tiny, :2] == 0).all()
    assert not (out[~tiny & (amax > 0), 2:] == 0x80).all(axis=1).any()


@pytest.mark.parametrize("case", D.cpy_cases(), ids=repr)
def test_cpy(case):
    src0, sv, dst0, dv, nan = case.build()
    want = R.cpy(src0, sv, dst0, dv)
    if dv is None:                                                  # CONT: a dense destination of the permuted shape
        ne, _ = sv.final()
        dv = R.View(sv.type, ne)
        dst0 = np.zeros(want.size, np.uint8)
    # a tail behind small destinations: a restatement that decomposes the destination wrongly writes there, not past the buffer
    slack = 8 * dst0.size if dst0.size < (1 << 20) else 0
    buf, srcw = np.concatenate([dst0, np.zeros(slack, np.uint8)]), np.array(src0)
    O.cpy(otensor(srcw, sv), otensor(buf, dv))
    got = buf[:dst0.size]
    assert not buf[dst0.size:].any(), f"cpy {case}: bytes written behind the destination"
    if nan is None:
        same_bytes(got, want, f"cpy {case}")
    else:                                                           # the 2046 NaNs among the 65 536 halves: NaN in both; every other word equal
        g, w = got.view(np.float32), want.view(np.float32)
        assert int(nan.sum()) == 2046 and np.isnan(w[nan]).all() and np.isnan(g[nan]).all() and not np.isnan(w[~nan]).any()
        D.assert_same_words(g[~nan], w[~nan], None, f"cpy {case}")


def test_cont_of_a_permuted_view_is_the_numpy_transposition():
    """what the permutations mean, from the reference alone"""
    for case in D.cpy_cases():
        if not case.name.startswith("cont_f32"):
            continue
        src0, sv, _, _, _ = case.build()
        want = R.cpy(src0, sv, None, None).view(np.float32)
        a = src0.view(np.float32).reshape(2, 3, 4, 8)
        axes = (1, 0, 2, 3) if sv.axes == "transpose" else sv.axes
        order = [3 - axes.index(d) for d in (3, 2, 1, 0)]           # numpy axis of the source that becomes result dimension d
        assert np.array_equal(want, np.ascontiguousarray(a.transpose(order)).reshape(-1)), case


@pytest.mark.parametrize("case", D.get_rows_cases(), ids=repr)
def test_get_rows(case):
    table, ibuf, iv = case.build()
    want = R.get_rows(table, case.type, case.ne, ibuf, iv)
    ine, _ = iv.final()
    got = np.zeros_like(want)
    tw, iw = np.array(table), np.array(ibuf)
    O.get_rows(O.tensor(tw, case.type, case.ne), otensor(iw, iv), O.tensor(got, O.F32, [case.ne[0], ine[0], ine[1], ine[2]]))
    assert np.isfinite(want).all()
    D.assert_same_words(got, want, None, f"get_rows {case}")


@pytest.mark.parametrize("case", D.soft_max_cases(), ids=repr)
def test_soft_max_with_a_mask(case):
    x, mask, mask_buf = case.build()
    dead = case.dead_rows()
    want = R.soft_max_ext(x, mask, case.scale)
    # the F16 and the F32 mask, out of place and in place: one expected result
    for mk in (mask, mask.astype(np.float16)):
        for inplace in (False, True):
            assert np.array_equal(R.soft_max_ext(x, mk, case.scale, inplace).view(np.uint32), want.view(np.uint32)), (mk.dtype, inplace)
    assert np.isnan(want[dead]).all() and not np.isnan(want[~dead]).any() and dead.any()
    m1, m2, m3 = case.mask_ne
    for mtype, buf in ((O.F32, np.array(mask_buf)), (O.F16, mask_buf.astype(np.float16))):
        got = np.zeros_like(x)
        O.soft_max(O.tensor(np.array(x), O.F32, [case.n0] + D.SOFT_X_NE), O.tensor(buf, mtype, [case.n0, m1, m2, m3]), O.tensor(got, O.F32, [case.n0] + D.SOFT_X_NE), scale=case.scale)
        D.assert_same_words(got[~dead], want[~dead], None, f"soft_max {case} mask type {mtype}")
        assert np.isnan(got[dead]).all()
