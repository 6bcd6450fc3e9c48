"""SET_ROWS (into F32, F16 and Q8_0), CPY / CONT, GET_ROWS (batched) and SOFT_MAX with a mask tensor on the device, through the C ABI via the Python mirror,
against the reference's own CPU backend (tests/ref_ggml.py) at the cases of tests/datamove_cases.py: index broadcasts, strided sources, destination views at
an offset, every launch geometry of k_set_rows_q8_0, the second trip of every grid-stride loop.  The WHOLE destination buffer is compared, byte for byte, so a
store outside the addressed rows fails; 0 differing bytes are allowed.  The two exceptions, both named by the cases and not read off the output: the 2046 NaNs
among the 65 536 halves of the F16 -> F32 copy and the soft_max rows whose every column is masked are compared as `NaN in both`.
tests/test_datamove_model.py settles the same cases on the CPU.  Reads oracle/_ref only."""
import numpy as np
import pytest

import datamove_cases as D
import ref_ggml as R

pytestmark = pytest.mark.gpu

CLLM_E_INVALID, CLLM_E_UNSUPPORTED = -1, -2
_ref_cache = {}


def reference(key, compute):
    """the reference's result, computed once per case and shared"""
    if key not in _ref_cache:
        y = compute()
        y.setflags(write=False)
        _ref_cache[key] = y
    return _ref_cache[key]


def device(gpu, raw, view):
    """the buffer `raw` on the device and the (permuted) view of it as a tensor; the view's extent is checked against the buffer first"""
    raw = np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    ne, nb = view.final()
    size, blck = R._BLOCK[view.type]
    last = view.offset + sum((ne[i] - 1) * nb[i] for i in range(4) if blck == 1 or i) + (size if blck == 1 else R.row_bytes(view.type, ne[0]))
    assert view.offset >= 0 and last <= raw.nbytes, f"{view} reaches byte {last} of {raw.nbytes}"
    t = gpu.Tensor.from_strided(raw, view.type, ne, nb)
    t.offset = view.offset
    return t


def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got).reshape(-1).view(np.uint8), np.ascontiguousarray(want).reshape(-1).view(np.uint8)
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} differing bytes of {want.size}; (offset, got, reference): " + str([(int(i), hex(got[i]), hex(want[i])) for i in bad[:8]])


# ---- SET_ROWS --------------------------------------------------------------------------------------------------------------------------------
def run_set_rows(gpu, case):
    dst0, dv, src, sv, idx, _ = case.build()
    want = reference(("set_rows", case.name), lambda: R.set_rows(dst0, dv, src, sv, idx))
    d = device(gpu, dst0, dv)
    gpu.ops.set_rows(d, device(gpu, src, sv), gpu.Tensor.from_numpy(idx))
    same_bytes(d.raw()[:dst0.size], want, f"set_rows {case}")


@pytest.mark.parametrize("case", D.set_rows_cases(), ids=repr)
def test_set_rows(gpu, case):
    run_set_rows(gpu, case)


@pytest.mark.parametrize("case", D.set_rows_q8_0_cases(), ids=repr)
def test_set_rows_q8_0(gpu, case):
    """the bytes of the reference's from_float, the x86 quantize_row_q8_0: ties to even, the block scale as fp16 (inf above 65504 * 127), 34-byte blocks"""
    nblk = case.src_ne[0] // 32 * case.src_ne[1] * case.src_ne[2] * case.src_ne[3]
    if case.name == "q8_0_past_one_trip":
        assert nblk == 262272 > 8192 * 32
    if case.name == "q8_0_past_one_trip_partial_last_wave":
        assert nblk > 8192 * 32 and (nblk - 8192 * 32) % 8 == 1
    run_set_rows(gpu, case)


# ---- CPY / CONT ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.cpy_cases(), ids=repr)
def test_cpy(gpu, case):
    src0, sv, dst0, dv, nan = case.build()
    want = reference(("cpy", case.name), lambda: R.cpy(src0, sv, dst0, dv))
    s = device(gpu, src0, sv)
    if dv is None:
        got = gpu.ops.cont(s).raw()[:want.size]
    else:
        d = device(gpu, dst0, dv)
        gpu.ops.cpy(s, d)
        got = d.raw()[:dst0.size]
    if nan is None:
        same_bytes(got, want, f"cpy {case}")
    else:                                                           # 2046 of the 65 536 halves are NaNs: NaN in both; every other word equal
        g, w = got.view(np.float32), want.view(np.float32)
        assert int(nan.sum()) == 2046 and np.isnan(w[nan]).all() and np.isnan(g[nan]).all()
        D.assert_same_words(g[~nan], w[~nan], None, f"cpy {case}")
    assert np.array_equal(s.raw()[:src0.size], src0)


# ---- GET_ROWS --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.get_rows_cases(), ids=repr)
def test_get_rows(gpu, case):
    table, ibuf, iv = case.build()
    want = reference(("get_rows", case.name), lambda: R.get_rows(table, case.type, case.ne, ibuf, iv))
    got = gpu.ops.get_rows(gpu.Tensor.from_numpy(table, case.type, case.ne), device(gpu, ibuf, iv)).numpy()
    D.assert_same_words(got, want, None, f"get_rows {case}")


# ---- SOFT_MAX with a mask ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.soft_max_cases(), ids=repr)
def test_soft_max_with_a_mask(gpu, case):
    x, mask, _ = case.build()
    dead = case.dead_rows()
    want = reference(("soft_max", case.name), lambda: R.soft_max_ext(x, mask, case.scale))
    want16 = reference(("soft_max16", case.name), lambda: R.soft_max_ext(x, mask.astype(np.float16), case.scale))
    assert np.array_equal(want16.view(np.uint32), want.view(np.uint32))          # the mask's values are exact in fp16: one expected result
    assert np.isnan(want[dead]).all() and not np.isnan(want[~dead]).any()
    for mk in (mask, mask.astype(np.float16)):
        for inplace in (False, True):
            t, m = gpu.Tensor.from_numpy(x), gpu.Tensor.from_numpy(mk)
            out = gpu.ops.soft_max_ext(t, m, case.scale, 0.0, dst=t if inplace else None)
            got = out.numpy().reshape(x.shape)
            what = f"soft_max {case} mask {mk.dtype} {'in place' if inplace else 'out of place'}"
            D.assert_same_words(got[~dead], want[~dead], None, what)
            assert np.isnan(got[dead]).all(), what
            assert np.array_equal(m.numpy().reshape(-1).view(np.uint8), mk.reshape(-1).view(np.uint8))
            if not inplace:
                assert np.array_equal(t.numpy().reshape(-1).view(np.uint32), x.reshape(-1).view(np.uint32))


# ---- what is declined ----------------------------------------------------------------------------------------------------------------------
def declined(gpu, call, dst, rc, word):
    before = dst.raw().copy()
    with pytest.raises(gpu.lib.CllmError) as e:
        call()
    assert e.value.rc == rc and word in str(e.value), str(e.value)
    assert np.array_equal(dst.raw(), before)


def test_set_rows_declines_a_q8_0_row_that_is_not_whole_blocks_and_a_misaligned_source(gpu):
    T = gpu.Tensor
    idx = T.from_numpy(np.array([1, 0], np.int64))
    # ne0 % 32 != 0: 48 floats a row into rows of 34 * 48 / 32 = 51 bytes
    src = T.from_numpy(np.ones((2, 48), np.float32))
    dst = T.from_strided(np.full(4 * 51, 7, np.uint8), gpu.Q8_0, [32, 4], [34, 51])
    dst.ne[0] = 48
    declined(gpu, lambda: gpu.ops.set_rows(dst, src, idx), dst, CLLM_E_INVALID, "shape")
    # a source 4 bytes into its buffer: aligned for a float, not for the kernel's 16-byte loads
    parent = T.from_numpy(np.ones(2 * 64 + 4, np.float32))
    dst = T.from_numpy(np.full(4 * 68, 7, np.uint8), gpu.Q8_0, [64, 4])
    declined(gpu, lambda: gpu.ops.set_rows(dst, parent.view([64, 2], [4, 256], 4), idx), dst, CLLM_E_UNSUPPORTED, "alignment")
    declined(gpu, lambda: gpu.ops.set_rows(dst, parent.view([64, 2], [4, 260], 0), idx), dst, CLLM_E_UNSUPPORTED, "alignment")


def test_cpy_declines_a_quantizing_copy_and_quantized_rows_of_another_length(gpu):
    T = gpu.Tensor
    f32 = T.from_numpy(np.ones((4, 64), np.float32))
    q = T.from_numpy(np.full(4 * 68, 7, np.uint8), gpu.Q8_0, [64, 4])
    declined(gpu, lambda: gpu.ops.cpy(f32, q), q, CLLM_E_UNSUPPORTED, "type")
    q2 = T.from_numpy(np.full(2 * 136, 9, np.uint8), gpu.Q8_0, [128, 2])          # the same 256 elements, rows twice as long
    declined(gpu, lambda: gpu.ops.cpy(q, q2), q2, CLLM_E_UNSUPPORTED, "whole")


def test_get_rows_declines_i64_ids(gpu):
    T = gpu.Tensor
    table = T.from_numpy(np.ones((6, 32), np.float32))
    dst = T.from_numpy(np.full((3, 32), 7.0, np.float32))
    declined(gpu, lambda: gpu.ops.get_rows(table, T.from_numpy(np.array([0, 5, 2], np.int64)), dst=dst), dst, CLLM_E_UNSUPPORTED, "type")


def test_soft_max_declines_a_mask_with_too_few_rows_and_alibi(gpu):
    T = gpu.Tensor
    x = T.from_numpy(np.ones((2, 5, 16), np.float32))
    dst = T.from_numpy(np.full((2, 5, 16), 7.0, np.float32))
    declined(gpu, lambda: gpu.ops.soft_max_ext(x, T.from_numpy(np.zeros((4, 16), np.float32)), 1.0, 0.0, dst=dst), dst, CLLM_E_INVALID, "mask shape")
    declined(gpu, lambda: gpu.ops.soft_max_ext(x, T.from_numpy(np.zeros((5, 16), np.float32)), 1.0, 8.0, dst=dst), dst, CLLM_E_UNSUPPORTED, "ALiBi")
