"""cllm_op_quantize_rows (csrc/quantize_w.hip: the loader's on-device re-quantizer) on the cases of tests/weight_quant_cases.py, byte for byte against the CPU
oracle, which tests/test_weight_quant_model.py holds against the reference build and a numpy mirror on the same cases: special blocks (zeros, ties of the block
maximum, the clamp, exact halves, stored scales on the fp16 edges, blocks whose inverse scale overflows, huge values), Q4_K's zero-code and code-63 paths, every
launch geometry around the 256-thread workgroup, destinations at odd 2-byte offsets, the F16 conversion of every half and every midpoint, the round trip through
cllm_dequantize_row, and every decline.

The destination always lies inside a buffer filled with POISON, GUARD bytes of it before and after the rows: the whole buffer is compared, so a store outside
the rows and a byte of the rows left unwritten both fail."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import weight_quant_cases as W

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xC3, 512
ids = lambda t: W.NAME[t]  # noqa: E731
_expected = {}


def expected(t, key, x):
    """the oracle's bytes, computed once per case"""
    if (t, key) not in _expected:
        _expected[t, key] = O.quantize_ref(t, x)
    return _expected[t, key]


class Run:
    """one call of cllm_op_quantize_rows into a poisoned buffer: rc, the whole buffer read back, where the rows lie in it"""

    def __init__(self, gpu, t, x, shift=0, x_shift=0, k=None, nrows=None, null_x=False, null_y=False):
        L = gpu.lib.get()
        x = np.ascontiguousarray(x, np.float32)
        self.t, self.n, self.lo = t, O.TYPE_SIZE[t] * (x.size // O.BLCK[t]), GUARD + shift
        total = (self.lo + self.n + GUARD + 3) // 4 * 4
        self.buf = gpu.Tensor.from_numpy(np.full(total, POISON, np.uint8).view(np.int32))
        pad = np.zeros(4, np.float32)
        self.dx = gpu.Tensor.from_numpy(np.concatenate([x.reshape(-1), pad]))
        assert self.buf.data_ptr().value % 16 == 0 and self.dx.data_ptr().value % 16 == 0
        self.y = C.c_void_p(None if null_y else self.buf.data_ptr().value + self.lo)
        xp = C.c_void_p(None if null_x else self.dx.data_ptr().value + x_shift)
        rows, kk = x.shape
        self.rc = L.cllm_op_quantize_rows(None, t, xp, self.y, kk if k is None else k, rows if nrows is None else nrows)
        self.error = L.cllm_last_error() or b""
        gpu.lib.check(L.cllm_stream_sync(None), "sync")
        self.whole = self.buf.raw()[:total]

    def rows(self):
        return self.whole[self.lo: self.lo + self.n]

    def guards_intact(self):
        return bool((self.whole[: self.lo] == POISON).all() and (self.whole[self.lo + self.n:] == POISON).all())

    def untouched(self):
        return bool((self.whole == POISON).all())


def assert_bytes(run, want, case, names=None):
    got, bs = run.rows(), O.TYPE_SIZE[run.t]
    assert run.rc == 0, f"{case}: rc {run.rc}: {run.error.decode()}"
    bad = np.flatnonzero(got != want)
    if bad.size:
        b, o = divmod(int(bad[0]), bs)
        label = names.get(b) if isinstance(names, dict) else names[b] if names else None
        blk = slice(b * bs, b * bs + bs)
        raise AssertionError(f"{W.NAME[run.t]} {case}: {bad.size} bytes differ; first: block {b}{' (' + label + ')' if label else ''} offset {o}: "
                             f"got {got[bad[0]]:#04x} want {want[bad[0]]:#04x}\n  got  {got[blk].tobytes().hex()}\n  want {want[blk].tobytes().hex()}")
    before, after = np.flatnonzero(run.whole[: run.lo] != POISON), np.flatnonzero(run.whole[run.lo + run.n:] != POISON)
    assert not before.size and not after.size, f"{W.NAME[run.t]} {case}: bytes written outside the rows: {before.size} before (last at -{run.lo - int(before[-1]) if before.size else 0}), {after.size} after (first at +{int(after[0]) if after.size else 0})"


# ---- bytes against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", W.B32_TYPES + (O.Q4_K,), ids=ids)
def test_special_blocks(gpu, t):
    """every special block (Q4_K: every special super-block), one per row"""
    names, x = W.special_case(t)
    assert_bytes(Run(gpu, t, x), expected(t, "special", x), "special", names)


@pytest.mark.parametrize("nb,layout", [g for g in W.geometry_ids(O.Q8_0)], ids=lambda v: str(v))
@pytest.mark.parametrize("t", W.B32_TYPES, ids=ids)
def test_block_geometries(gpu, t, nb, layout):
    """1, 255, 256, 257 and 513 blocks (one thread each, 256 per workgroup) as one row and as one row per block, at three magnitudes"""
    for s in W.SCALES:
        x, laid = W.geometry(t, nb, layout, s)
        assert_bytes(Run(gpu, t, x), expected(t, (nb, layout, s), x), f"{nb} blocks as {layout}, scale {s:g}", laid)


@pytest.mark.parametrize("nb,layout", W.geometry_ids(O.Q4_K), ids=lambda v: str(v))
def test_q4_K_geometries(gpu, nb, layout):
    """1, 7, 31, 32, 33 and 65 super-blocks (eight lanes each, 32 per workgroup): dead lane groups of the last workgroup take part in the exchanges and store nothing"""
    for s in W.SCALES:
        x, laid = W.geometry(O.Q4_K, nb, layout, s)
        assert_bytes(Run(gpu, O.Q4_K, x), expected(O.Q4_K, (nb, layout, s), x), f"{nb} super-blocks as {layout}, scale {s:g}", laid)


@pytest.mark.parametrize("shift", [2, 6])
@pytest.mark.parametrize("t", W.B32_TYPES, ids=ids)
def test_destination_at_a_2_byte_offset(gpu, t, shift):
    """the 32-weight kernels store 16-bit words: y at +2 and +6 bytes from a 16-byte boundary (the source stays 16-byte aligned)"""
    x, laid = W.geometry(t, 257, "row", 1.0)
    run = Run(gpu, t, x, shift=shift)
    assert run.y.value % 16 == shift
    assert_bytes(run, expected(t, (257, "row", 1.0), x), f"257 blocks, y at +{shift}", laid)


# ---- F16 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["all_halves", "midpoints", "extremes", "n_1", "n_255", "n_256", "n_257"])
def test_f16_equals_numpy_and_the_oracle(gpu, case):
    """every half's float converts back to that half; every midpoint of adjacent halves goes to the even one and its float neighbours to their sides; 65520 and
    everything above become inf, 2^-25 becomes 0 and the float above it the smallest subnormal"""
    x = W.f16_cases()[case].reshape(1, -1)
    with np.errstate(over="ignore"):
        want = x.reshape(-1).astype(np.float16).view(np.uint8)
    assert np.array_equal(want, expected(O.F16, case, x))
    assert_bytes(Run(gpu, O.F16, x), want, case)
    if x.size % 2:                                       # F16's block is one element: any k > 0 is a whole number of blocks, also as rows of odd length
        assert_bytes(Run(gpu, O.F16, x, k=1, nrows=x.size), want, case + " as rows of 1")


def test_f16_nan_stays_a_nan_of_the_same_sign(gpu):
    """quiet and signalling NaNs of both signs, every half NaN's float among them: the device writes a NaN of the same sign, which is all that is asserted.
    What the hardware conversion (v_cvt_f16_f32) was seen to produce on gfx950: the sign, the top ten payload bits and the quiet bit set -- 512 distinct
    magnitudes over this case, for all 2058 inputs the half the oracle's conversion writes.  The reference build writes 0x7e00 / 0xfe00 for every NaN, which
    the device equals only where the top ten payload bits are zero.  The census is printed, not asserted: f2h is not written for payloads"""
    x = W.f16_cases()["nan"].reshape(1, -1)
    run = Run(gpu, O.F16, x)
    assert run.rc == 0 and run.guards_intact()
    got = run.rows().view(np.uint16)
    orc = expected(O.F16, "nan", x).view(np.uint16)
    vals, counts = np.unique(got & 0x7fff, return_counts=True)
    print(f"F16 NaN payloads on the device: {len(vals)} distinct magnitudes, most frequent {[(hex(v), int(c)) for v, c in sorted(zip(vals, counts), key=lambda p: -p[1])[:4]]}; "
          f"{int((got == orc).sum())} of {got.size} equal the oracle's half")
    assert ((got & 0x7c00) == 0x7c00).all() and ((got & 0x03ff) != 0).all()
    assert np.array_equal(got >> 15, (x.reshape(-1).view(np.uint32) >> 31).astype(np.uint16))


# ---- the round trip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", W.TYPES, ids=ids)
def test_round_trip_through_dequantize_row(gpu, t):
    """cllm_dequantize_row over the rows the device quantized == the oracle's dequantize_row over the oracle's bytes, word for word"""
    L = gpu.lib.get()
    x = W.round_trip_case(t)
    want_bytes = expected(t, "round_trip", x)
    run = Run(gpu, t, x)
    assert_bytes(run, want_bytes, "round trip")
    assert run.y.value % 16 == 0
    out = gpu.Tensor.from_numpy(np.full(x.size + 64, np.float32(-777.0), np.float32))
    gpu.lib.check(L.cllm_dequantize_row(None, t, run.y, out.data_ptr(), x.size), "dequantize_row")
    gpu.lib.check(L.cllm_stream_sync(None), "sync")
    got = out.numpy()
    want = W.dequantize_expected(t, want_bytes, x.size)
    bad = np.flatnonzero(got[: x.size].view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{W.NAME[t]}: {bad.size} words differ; first: element {int(bad[0])}: got {got[bad[0]]!r} want {want[bad[0]]!r}"
    assert (got[x.size:] == np.float32(-777.0)).all()


# ---- declines ---------------------------------------------------------------------------------------------------------------------------
def declined(run, message):
    assert run.rc != 0 and message in run.error, (run.rc, run.error)
    assert run.untouched(), "a declined call wrote to the destination"


@pytest.mark.parametrize("t", W.TYPES, ids=ids)
def test_declines(gpu, t):
    """every refusal returns non-zero with its message and leaves the destination as it was"""
    bs = O.BLCK[t]
    x = np.ones((2, 2 * bs if bs > 1 else 64), np.float32)
    k = x.shape[1]
    align = b"not a multiple of the block"                                # one message for the block size and for the operand alignment
    if bs > 1:
        for bad_k in (bs + 1, bs - 1, bs // 2, bs + 32 if bs == 256 else 3 * bs // 2):
            assert bad_k % bs
            declined(Run(gpu, t, x, k=bad_k, nrows=1), align)
    for bad_k, bad_rows in ((0, 2), (-bs, 2), (k, 0), (k, -1)):
        declined(Run(gpu, t, x, k=bad_k, nrows=bad_rows), b"quantize_rows: arguments")
    declined(Run(gpu, t, x, null_x=True), b"quantize_rows: arguments")
    declined(Run(gpu, t, x, null_y=True), b"quantize_rows: arguments")
    declined(Run(gpu, t, x, x_shift=4, nrows=1), align)
    declined(Run(gpu, t, x, shift=1), align)
    if t == O.Q4_K:
        for shift in (2, 8):
            declined(Run(gpu, t, x, shift=shift), b"Q4_K rows must be 16-byte aligned")
    # more blocks than one call takes: k = 2^41 with enough rows to pass 2^31 * 32 blocks; refused before anything is launched
    big_k, limit = 1 << 41, 0x7fffffff * 32
    big_rows = 2 if bs <= 32 else 64
    assert big_k % bs == 0 and big_k * big_rows // bs > limit
    declined(Run(gpu, t, x, k=big_k, nrows=big_rows), b"too many blocks in one call")


@pytest.mark.parametrize("t", [O.Q5_K, O.Q6_K, O.Q2_K, O.Q3_K, O.IQ4_NL, O.MXFP4, O.Q8_1, O.Q8_K, O.F32], ids=lambda t: f"type{t}")
def test_types_without_a_device_quantizer_decline(gpu, t):
    """a weight or plain type the library knows: `no device quantizer`; the activation formats Q8_1 / Q8_K are no tensor types of the library at all (block size 0)"""
    L = gpu.lib.get()
    x = np.ones((2, 512), np.float32)
    run = Run(gpu, O.Q8_0, x)                                              # a destination large enough for any of them
    assert run.rc == 0
    poisoned = Run(gpu, O.Q8_0, x, null_x=True)                            # declined: its buffer is still all POISON
    rc = L.cllm_op_quantize_rows(None, t, run.dx.data_ptr(), poisoned.y, 512, 2)
    msg = L.cllm_last_error() or b""
    gpu.lib.check(L.cllm_stream_sync(None), "sync")
    assert rc != 0 and (b"no device quantizer" if L.cllm_blck_size(t) else b"not a multiple of the block (0)") in msg, (rc, msg)
    assert (L.cllm_blck_size(t) == 0) == (t in (O.Q8_1, O.Q8_K))
    assert (poisoned.buf.raw() == POISON).all()
