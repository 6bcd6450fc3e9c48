"""cllm_op_mul_mat / cllm_op_mul_mat_ex on the device over every operand layout of tests/matmul_layout_cases.py -- weight rows that are not back to back, a column slice
of a wider weight, padded and permuted src1, 4-D src1 with r2 / r3 > 1, padded dst, views at an offset -- against the CPU oracle, which tests/test_matmul_layout_model.py
holds word for word against the reference build on the same views, and which it shows to give another result as soon as one stride is taken for its dense value.

  exact routes       (default / exact prefill mode: the one-launch decode mat-vec, mmvq, mmx, gemv_kq, the lane-group float kernels, mmf_exact) dst == the oracle bit for
                     bit through the view, and every byte of the dst buffer outside the view still holds the sentinel
  tolerance tiers    mmq (prefill mode 0), dense_f16 (both tiles), mma_f16 (fast attention mode): every element inside tier_model's bound for that kernel, evaluated
                     on the dense copies; the padding keeps its sentinel.  mma_f16 is tier_model item 4 with the F16 weights as they are: the products of fp16 values are
                     exact in fp32, src1 is rounded to fp16 as the reference rounds it, so the only error is the fp32 accumulation of K terms on the matrix cores:
                     |got - R| <= 2 K 2^-24 sum_k |w_k x16_k|
  cllm_op_mul_mat_ex prologues 0 / 1 / 3 / 4 over padded src1 rows, the residual epilogue with a padded residual, the SiLU * up epilogue into a padded dst, at 12 and 40
                     columns in both prefill modes, against the same mode's node sequence
  declines           layouts no kernel can load: CLLM_E_UNSUPPORTED / CLLM_E_INVALID, cllm_last_error set, dst untouched

One case is one upload and one launch.  A test is one weight type in one layout: it walks that layout's shapes and column counts (K, N, M), goes on past a case that
differs, and fails at the end with the names of all that did (a case's name says type, K, N, M, batch and layout).  After a device error nothing further is started
(the remaining tests fail at once)."""
import ctypes as C
import functools

import numpy as np
import pytest

import matmul_layout_cases as L
import oracle as O
import tier_model as TM
from conftest import load_package, prefill_mode

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -2                     # cllm_status
_failed = []


def device_test(fn):
    """a test body that ends in anything but an assertion or a refused argument stops the module: nothing else is launched"""
    @functools.wraps(fn)
    def run(*a, **kw):
        if _failed:
            pytest.fail(f"not started: {_failed[0]} ended with a device error")
        try:
            return fn(*a, **kw)
        except AssertionError:
            raise
        except load_package().lib.CllmError as e:
            if e.rc in (INVALID, UNSUPPORTED):
                raise AssertionError(str(e)) from e
            _failed.append(fn.__name__)
            raise
        except BaseException:
            _failed.append(fn.__name__)
            raise
    return run


class Walk:
    """runs the cases of one test one after the other: an assertion, or a call refused for its arguments, fails that case and the walk goes on; anything else (a device
    error) ends the test at once"""

    def __init__(self):
        self.bad = []

    def case(self, name, fn):
        try:
            fn()
        except AssertionError as e:
            self.bad.append(f"{name}: {e}")
        except load_package().lib.CllmError as e:
            if e.rc not in (INVALID, UNSUPPORTED):
                raise
            self.bad.append(f"{name}: refused: {e}")

    def done(self, n):
        assert n > 0
        assert not self.bad, f"{len(self.bad)} of {n} cases fail:\n" + "\n".join(self.bad[:10])


def by_type_and_layout(cases):
    """{(type, layout): cases}, in case order"""
    out = {}
    for c in cases:
        out.setdefault((c.t, c.layout), []).append(c)
    return out


group_id = lambda k: f"{L.TYPE_NAME[k[0]]}-{k[1]}"  # noqa: E731
TH = L.thresholds()
EXACT_CASES = L.CASES
MMQ_CASES = [c for c in L.TUNED_CASES if L.route_of(c, TH, prefill=0) == "mmq"]
F16_MODE_CASES = [c for c in L.TUNED_CASES if L.route_of(c, TH, prefill=0, f16=True) == "dense_f16" and c.M == 40 and (c.N == 130 or c.layout in L.LAYOUTS_3D)]
MMA_CASES = [c for c in L.FLOAT_CASES if L.route_of(c, TH, attn=0) == "mma_f16"]
EXACT_GROUPS, MMQ_GROUPS, F16_MODE_GROUPS = by_type_and_layout(EXACT_CASES), by_type_and_layout(MMQ_CASES), by_type_and_layout(F16_MODE_CASES)


# ---- host <-> device ------------------------------------------------------------------------------------------------------------------------
def dev(gpu, raw, t, v):
    """the bytes of a whole buffer on the device, described as the view v"""
    lib = gpu.lib.get()
    raw = np.ascontiguousarray(raw)
    assert L.extent(t, v) <= raw.size
    buf = gpu.tensor.Buffer(raw.size)
    gpu.lib.check(lib.cllm_memcpy_h2d(buf.ptr, raw.ctypes.data_as(C.c_void_p), raw.size, None), "h2d")
    gpu.lib.check(lib.cllm_stream_sync(None), "sync")
    return gpu.Tensor(t, v.ne, v.nb, buf, v.offset)


def operands(gpu, c):
    b = L.build(c)
    return b, dev(gpu, b.w_raw, c.t, c.wv), dev(gpu, b.x_raw, gpu.F32, c.xv), dev(gpu, b.d_raw, gpu.F32, c.dv)


def padding_untouched(c, got):
    m = L.view_mask(got.size, L.F32, c.dv)
    assert np.all(got[~m] == L.SENTINEL), f"{c.name}: {int(np.sum(got[~m] != L.SENTINEL))} bytes of dst padding were written"


def same_through_the_view(c, got, exp):
    g = L.gather(got, L.F32, c.dv).reshape(-1).view(np.uint32)
    e = L.gather(exp, L.F32, c.dv).reshape(-1).view(np.uint32)
    bad = np.flatnonzero(g != e)
    assert bad.size == 0, f"{c.name}: {bad.size} differing words of {e.size}; (index, device, oracle): " + str([(int(i), hex(g[i]), hex(e[i])) for i in bad[:6]])
    padding_untouched(c, got)


def inside(tag, got, R, bound):
    """|got - R| <= bound at every element; prints the largest ratio"""
    err = np.abs(got.astype(np.float64) - R)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"TIER_RATIO {tag} {ratio:.4f}")
    assert np.all(np.isfinite(got)) and np.all(err <= bound), (tag, ratio)


def result(c, got):
    """the dst view of the buffer as float32 [ne13, ne12, M, N]"""
    return L.gather(got, L.F32, c.dv).view(np.float32).reshape(c.ne13, c.ne12, c.M, c.N)


def slices(c, b):
    """(i13, i12, weight rows [N, row bytes], src1 [M, K]) of every slice of the broadcast product"""
    r2, r3 = c.ne12 // c.ne02, c.ne13 // c.ne03
    for i13 in range(c.ne13):
        for i12 in range(c.ne12):
            yield i13, i12, b.w_dense[i13 // r3, i12 // r2], b.x_dense[i13, i12]


# ---- the exact routes -----------------------------------------------------------------------------------------------------------------------
def exact_case(gpu, c):
    b, dw, dx, dd = operands(gpu, c)
    _, exp = L.expected(O, c)
    gpu.ops.mul_mat(dw, dx, dst=dd)
    same_through_the_view(c, dd.raw()[:exp.size], exp)


@pytest.mark.parametrize("key", list(EXACT_GROUPS), ids=group_id)
@device_test
def test_exact_routes_equal_the_oracle_through_the_view(gpu, key):
    walk = Walk()
    for c in EXACT_GROUPS[key]:
        walk.case(c.name, lambda: exact_case(gpu, c))
    walk.done(len(EXACT_GROUPS[key]))


# ---- the tolerance tiers --------------------------------------------------------------------------------------------------------------------
def mmq_case(gpu, c):
    b, dw, dx, dd = operands(gpu, c)
    with prefill_mode(gpu, 0):
        gpu.ops.mul_mat(dw, dx, dst=dd)
    got = dd.raw()[:b.d_raw.size]
    y = result(c, got)
    for i13, i12, w, x in slices(c, b):
        R, bound = TM.fast_bound(TM.terms_matrix(c.t, w, TM.act_rows(O, c.t, x)))
        inside(f"fast {c.name} [{i12},{i13}]", y[i13, i12], R, bound)
    padding_untouched(c, got)


@pytest.mark.parametrize("key", list(MMQ_GROUPS), ids=group_id)
@device_test
def test_fast_prefill_is_inside_the_bound_through_the_view(gpu, key):
    """k_mmq: (n_t + 8) 2^-24 S over the float64 block terms of the dense copies (tier_model.fast_bound)"""
    walk = Walk()
    for c in MMQ_GROUPS[key]:
        walk.case(c.name, lambda: mmq_case(gpu, c))
    walk.done(len(MMQ_GROUPS[key]))


def f16_mode_case(gpu, c, tile):
    b, dw, dx, dd = operands(gpu, c)
    lib = C.CDLL(gpu.lib.SO_PATH)
    lib.cllm_debug_set_prefill_f16(1)
    lib.cllm_debug_set_mmd_tile(tile)
    try:
        with prefill_mode(gpu, 0):
            gpu.ops.mul_mat(dw, dx, dst=dd)
    finally:
        lib.cllm_debug_set_prefill_f16(0)
        lib.cllm_debug_set_mmd_tile(0)
    got = dd.raw()[:b.d_raw.size]
    y = result(c, got)
    for i13, i12, w, x in slices(c, b):
        R, bound = TM.f16_bound(c.t, w, x)
        inside(f"f16-{tile} {c.name} [{i12},{i13}]", y[i13, i12], R, bound)
    padding_untouched(c, got)


@pytest.mark.parametrize("key", list(F16_MODE_GROUPS), ids=group_id)
@device_test
def test_f16_prefill_is_inside_the_bound_through_the_view(gpu, key):
    """k_mmd at both tiles: tier_model.f16_bound of the dense copies"""
    walk = Walk()
    for c in F16_MODE_GROUPS[key]:
        for tile in (128, 256):
            walk.case(f"{c.name} tile {tile}", lambda: f16_mode_case(gpu, c, tile))
    walk.done(2 * len(F16_MODE_GROUPS[key]))


def mma_case(gpu, c):
    b, dw, dx, dd = operands(gpu, c)
    lib = gpu.lib.get()
    assert lib.cllm_set_prefill_attn_mode(0) == 0
    try:
        gpu.ops.mul_mat(dw, dx, dst=dd)
    finally:
        lib.cllm_set_prefill_attn_mode(-1)
    got = dd.raw()[:b.d_raw.size]
    y = result(c, got)
    for i13, i12, w, x in slices(c, b):
        w16 = np.ascontiguousarray(w).view(np.float16).astype(np.float64)              # [N, K]
        x16 = x.astype(np.float16).astype(np.float64)
        inside(f"mma {c.name} [{i12},{i13}]", y[i13, i12], x16 @ w16.T, 2 * c.K * TM.U32 * (np.abs(x16) @ np.abs(w16).T))
    padding_untouched(c, got)


@device_test
def test_fast_attention_product_is_inside_the_bound_through_the_view(gpu):
    """k_mma_f16 (fast attention mode, F16 weights, 16-byte aligned operands, every layout that keeps them so): the module docstring's bound"""
    assert {c.layout for c in MMA_CASES} >= {"dense", "w_row_pad", "x_row_pad", "d_row_pad", "w_3d_r2", "w_3d_r3", "x_permuted", "kq_like", "vp_like"}
    walk = Walk()
    for c in MMA_CASES:
        walk.case(c.name, lambda: mma_case(gpu, c))
    walk.done(len(MMA_CASES))


# ---- cllm_op_mul_mat_ex ---------------------------------------------------------------------------------------------------------------------
def padded_f32(gpu, a, pad_bytes, fill):
    """a [rows, n] float32 in rows 4 n + pad_bytes apart, the rest of the buffer `fill` -> (device view, the buffer as uploaded)"""
    rows, n = a.shape
    v = L.View([n, rows, 1, 1], [4, 4 * n + pad_bytes, (4 * n + pad_bytes) * rows, (4 * n + pad_bytes) * rows], 0)
    raw = np.full(L.extent(L.F32, v) + 16, fill, np.uint8)
    L.scatter(raw, L.F32, v, np.ascontiguousarray(a).view(np.uint8).reshape(1, 1, rows, 4 * n))
    return dev(gpu, raw, gpu.F32, v), raw, v


@pytest.mark.parametrize("mode", [1, 0], ids=["exact", "fast"])
@pytest.mark.parametrize("M", [12, 40])
@pytest.mark.parametrize("t", L.TUNED, ids=lambda t: L.TYPE_NAME[t])
@device_test
def test_mul_mat_ex_over_padded_operands_equals_the_node_sequences(gpu, t, M, mode):
    """src1 rows 4 K + 16 bytes apart (poison between them) under prologues 0, 1, 3 and 4 (4: gate and up both padded); a residual in rows 4 N + 12 apart; the SiLU * up
    epilogue into dst rows 4 (N / 2) + 12 apart -- bit for bit the same mode's node sequence over dense copies (test_mul_mat_ex_equals_the_node_sequences')"""
    ops, T = gpu.ops, gpu.Tensor
    K, N = 512, 130
    r_ = np.random.default_rng([41, t, M, mode])
    w = T.from_numpy(L.rand_blocks(t, N, K, r_), t, [K, N])
    xh, uh = r_.standard_normal((M, K)).astype(np.float32), r_.standard_normal((M, K)).astype(np.float32)
    gh = (1.0 + 0.1 * r_.standard_normal(K)).astype(np.float32)
    rh = r_.standard_normal((M, N)).astype(np.float32)
    x2h = r_.standard_normal((M, 2 * K)).astype(np.float32)
    xd, ud, g, rd, x2d = T.from_numpy(xh), T.from_numpy(uh), T.from_numpy(gh), T.from_numpy(rh), T.from_numpy(x2h)
    xs, _, _ = padded_f32(gpu, xh, 16, L.POISON)
    us, _, _ = padded_f32(gpu, uh, 16, L.POISON)
    x2s, _, _ = padded_f32(gpu, x2h, 16, L.POISON)
    bits = lambda a: a.numpy().view(np.uint32).reshape(-1)  # noqa: E731
    with prefill_mode(gpu, mode):
        y = ops.mul_mat(w, xd)
        yn = ops.mul_mat(w, ops.rms_norm_mul(xd, g, 1e-5))
        assert np.array_equal(bits(ops.mul_mat_ex(w, xs)), bits(y)), "pro 0"
        assert np.array_equal(bits(ops.mul_mat_ex(w, xs, pro=1, norm_w=g, eps=1e-5)), bits(yn)), "pro 1"
        ge = x2d.view([K, M], [8, x2d.nb[1]], offset=0); ue = x2d.view([K, M], [8, x2d.nb[1]], offset=4)
        want3 = ops.mul_mat(w, ops.mul(ops.silu(ops.cont(ge)), ops.cont(ue)))
        assert np.array_equal(bits(ops.mul_mat_ex(w, x2s, pro=3)), bits(want3)), "pro 3"
        want4 = ops.mul_mat(w, ops.mul(ops.silu(xd), ud))
        assert np.array_equal(bits(ops.mul_mat_ex(w, xs, pro=4, norm_w=us)), bits(want4)), "pro 4"
        # epilogue 0 with a padded residual (the padding is poison: read, it would show)
        rs, r_raw, _ = padded_f32(gpu, rh, 12, L.POISON)
        assert np.array_equal(bits(ops.mul_mat_ex(w, xs, resid=rs)), bits(ops.add(y, rd))), "epi 0, padded residual"
        assert np.array_equal(rs.raw(), r_raw), "the residual buffer was written"
        # epilogue 1 into a padded dst
        H = N // 2
        ds, d_raw, dv = padded_f32(gpu, np.zeros((M, H), np.float32), 12, L.SENTINEL)
        m = L.view_mask(d_raw.size, L.F32, dv)
        ops.mul_mat_ex(w, xs, epi=1, dst=ds)
        gate = y.view([H, M], [8, y.nb[1]], offset=0); up = y.view([H, M], [8, y.nb[1]], offset=4)
        want_s = ops.mul(ops.silu(ops.cont(gate)), ops.cont(up)).numpy()
        got = ds.raw()
        assert np.array_equal(L.gather(got, L.F32, dv).reshape(-1).view(np.uint32), want_s.view(np.uint32).reshape(-1)), "epi 1, padded dst"
        assert np.all(got[~m] == L.SENTINEL), "epi 1: dst padding was written"


# ---- declines -------------------------------------------------------------------------------------------------------------------------------
def _decline_views(t, M, what):
    """dense [K = 512, N = 20] x [K, M] (two slices where a slice stride is what is broken) with ONE thing no kernel can load"""
    K, N = 512, 20
    ne12, ne13 = (2 if what == "x.nb[2]" else 1), (2 if what == "x.nb[3]" else 1)
    wv, xv, dv = L.layout_views(t, K, N, M, 1, 1, ne12, ne13, ())
    wnb, xnb, dnb, woff, xoff = list(wv.nb), list(xv.nb), list(dv.nb), 0, 0
    if what == "x.nb[1]":                        # 8 bytes more: a multiple of 4, not of 16
        xnb[1] += 8; xnb[2] = xnb[1] * M; xnb[3] = xnb[2]
    elif what == "x.nb[2]":
        xnb[2] += 8; xnb[3] = xnb[2] * ne12
    elif what == "x.nb[3]":
        xnb[3] += 8
    elif what == "x.data":
        xoff = 4
    elif what == "w.offset":                     # half the type's row_align
        woff = L.ROW_ALIGN[t] // 2
    elif what == "w.nb[1]":
        wnb[1] += L.ROW_ALIGN[t] // 2; wnb[2] = wnb[1] * N; wnb[3] = wnb[2]
    elif what == "d.nb[1]":
        dnb[1] += 2; dnb[2] = dnb[1] * M; dnb[3] = dnb[2]
    elif what == "w.odd":
        woff = 1
    else:
        raise KeyError(what)
    return L.View(wv.ne, wnb, woff), L.View(xv.ne, xnb, xoff), L.View(dv.ne, dnb, 0)


Q4_0, Q4_1, Q8_0, Q4_K, Q5_K, Q6_K, IQ4_XS = 2, 3, 8, 12, 13, 14, 23
DECLINES = [(t, M, what) for t in (Q4_0, Q4_K, Q6_K) for M in (3, 12) for what in ("x.nb[1]", "x.nb[2]", "x.nb[3]", "x.data")] + \
           [(t, M, what) for t in (Q4_K, Q4_1, Q5_K, IQ4_XS) for M in (1, 3, 12, 40) for what in ("w.offset", "w.nb[1]")] + \
           [(t, M, "d.nb[1]") for t in (Q4_0, Q4_K, Q6_K, L.F16, L.F32) for M in (3, 12, 40)] + \
           [(t, M, "w.odd") for t in (Q4_0, Q8_0, Q6_K, L.F16) for M in (1, 3, 12)] + \
           [(t, M, "x.data") for t in (Q4_0, Q4_K) for M in (1,)]


DECLINE_GROUPS = {}
for _t, _M, _what in DECLINES:
    DECLINE_GROUPS.setdefault((_t, _what), []).append(_M)


@pytest.mark.parametrize("key", list(DECLINE_GROUPS), ids=group_id)
@device_test
def test_layouts_no_kernel_can_load_are_declined(gpu, key):
    """at every column count of the group: an error code, cllm_last_error set by THIS call, and not a byte of dst written (the case is dense but for the one broken
    thing, so a call that went on would compute something)"""
    t, what = key
    walk = Walk()
    for M in DECLINE_GROUPS[key]:
        walk.case(f"{L.TYPE_NAME[t]}-M{M}-{what}", lambda: declined_case(gpu, t, M, what))
    walk.done(len(DECLINE_GROUPS[key]))


def declined_case(gpu, t, M, what):
    lib = gpu.lib.get()
    wv, xv, dv = _decline_views(t, M, what)
    rng = np.random.default_rng([7, t, M])
    w_raw = np.full(L.extent(t, wv) + 16, L.POISON, np.uint8)
    rows = rng.standard_normal((20, 512)).astype(np.float16 if t == L.F16 else np.float32).view(np.uint8) if t in L.FLOAT_TYPES else L.rand_blocks(t, 20, 512, rng)
    L.scatter(w_raw, t, wv, rows.reshape(1, 1, 20, -1))
    x_raw = np.zeros(L.extent(L.F32, xv) + 16, np.uint8)
    d_raw = np.full(L.extent(L.F32, dv) + 16, L.SENTINEL, np.uint8)
    dw, dx, dd = dev(gpu, w_raw, t, wv), dev(gpu, x_raw, gpu.F32, xv), dev(gpu, d_raw, gpu.F32, dv)
    ca, cb, cd = dw.c(), dx.c(), dd.c()
    ws = int(lib.cllm_mul_mat_wsize(C.byref(ca), C.byref(cb)))
    scratch = gpu.tensor.Buffer(max(ws, 16))
    assert lib.cllm_set_prefill_mode(7) != 0 and b"set_prefill_mode" in lib.cllm_last_error()          # a known last error, for this call to replace
    rc = lib.cllm_op_mul_mat(None, C.byref(ca), C.byref(cb), C.byref(cd), scratch.ptr, scratch.nbytes)
    gpu.ops.sync()
    err = lib.cllm_last_error()
    assert rc in (INVALID, UNSUPPORTED), (rc, err)
    assert err and b"set_prefill_mode" not in err, err
    assert np.all(dd.raw() == L.SENTINEL), "a declined call wrote dst"
