"""GPU: the sparse-MoE kernels against the CPU oracle at every launch geometry (the cases, the plans and the oracle chains: tests/moe_model.py; that each case has the
geometry it is named for: tests/test_moe_model.py).

  one token    cllm_op_mul_mat_id (k_gemv_dec<.., MOE> EPI 0, or the general path past 64 slots / K 32768), cllm_op_mul_mat_id_silu_mul (EPI 1),
               cllm_op_mul_mat_id_combine (EPI 3), cllm_op_moe_router (EPI 2), cllm_op_moe_router_gate_up (EPI 5), cllm_op_moe_combine, and a whole block in place;
  many tokens  cllm_op_mul_mat_id of all 22 quantized types through launch_mmvq_id / launch_gemv_kq_id, up to the 65535 (slot, token) pairs of one launch.

Everything here is the exact tier: values are compared as uint32 words with the oracle chain, ids exactly, and every byte of padding (dst rows further apart than N,
the gaps between the tokens' planes) must still hold the sentinel it was filled with.  Where a case is meant for a fused launcher the test also shows that it ran:
the fused entry points return CLLM_E_UNSUPPORTED instead of falling back (gpu.ops raises on it), and cllm_op_mul_mat_id, which does fall back inside, quantizes the
activation into the caller's scratch on its general path only -- a sentinel-filled scratch that comes back untouched is the one-token kernel's signature.

After a device error nothing further is started (the remaining tests fail at once); a call refused for its arguments (CLLM_E_INVALID / CLLM_E_UNSUPPORTED) is an
ordinary failure."""
import ctypes as C
import functools

import numpy as np
import pytest

import moe_model as M
import oracle as O
from conftest import load_package

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -2                     # cllm_status
_failed = []
name_of = lambda c: c.name  # noqa: E731


def device_test(fn):
    """a test body that ends in anything but an assertion (a HIP error, a fault reported by the library) stops the module: nothing else is launched"""
    @functools.wraps(fn)
    def run(*a, **kw):
        if _failed:
            pytest.fail(f"not started: {_failed[0]} ended with a device error")
        try:
            return fn(*a, **kw)
        except AssertionError:
            raise
        except load_package().lib.CllmError as e:
            if e.rc in (INVALID, UNSUPPORTED):              # an argument or a shape refused: a failed test, nothing was launched
                raise AssertionError(str(e)) from e
            _failed.append(fn.__name__)
            raise
        except BaseException:
            _failed.append(fn.__name__)
            raise
    return run


@pytest.fixture(scope="module")
def n_cu(gpu):
    n = C.c_int(0)
    gpu.lib.check(gpu.lib.get().cllm_device_info(0, None, 0, None, None, C.byref(n)), "device_info")
    assert n.value > 0
    return n.value


# ---- host <-> device helpers -------------------------------------------------------------------------------------------------------------
def dev_w(gpu, w, t, K, N, E, pad=0):
    if not pad:
        return gpu.Tensor.from_numpy(w, t, [K, N, E])
    buf, nb2 = M.padded_experts(w, E, pad)
    return gpu.Tensor.from_strided(buf, t, [K, N, E], [O.TYPE_SIZE[t], O.row_size(t, K), nb2, nb2 * E])


def dev_a(gpu, a, pad1=0, pad2=0):
    """a: [n2, n1, n0] float32 | int32 -> the device tensor over a sentinel-padded buffer"""
    buf, nb, _ = M.padded(a, pad1, pad2)
    return gpu.Tensor.from_strided(buf, gpu.I32 if a.dtype == np.int32 else gpu.F32, list(reversed(a.shape)), nb)


def dev_out(gpu, want, pad1=0, pad2=0):
    """-> (a device tensor of want's shape and padding, EVERY byte the sentinel; the buffer expected afterwards; the mask of the tensor's own bytes)"""
    exp, nb, mask = M.padded(want, pad1, pad2)
    t = gpu.Tensor.from_strided(np.full(exp.size, M.SENTINEL, np.uint8), gpu.I32 if want.dtype == np.int32 else gpu.F32, list(reversed(want.shape)), nb)
    return t, exp, mask


def check_out(t, exp, mask):
    got = t.raw()[:exp.size]
    g, e = got[mask].view(np.uint32), exp[mask].view(np.uint32)
    assert np.array_equal(g, e), (int(np.sum(g != e)), np.flatnonzero(g != e)[:6].tolist(), g.view(np.float32)[g != e][:3].tolist(), e.view(np.float32)[g != e][:3].tolist())
    assert np.array_equal(got[~mask], exp[~mask]), f"{int(np.sum(got[~mask] != exp[~mask]))} bytes of padding were written"


def untouched(t):
    return bool(np.all(t.raw() == M.SENTINEL))


def bits(t):
    return t.numpy().view(np.uint32).reshape(-1)


def same_bits(t, want):
    g, e = bits(t), np.ascontiguousarray(want).view(np.uint32).reshape(-1)
    assert np.array_equal(g, e), (int(np.sum(g != e)), np.flatnonzero(g != e)[:6].tolist(), g.view(np.float32)[g != e][:3].tolist(), e.view(np.float32)[g != e][:3].tolist())


def call_mul_mat_id(gpu, as_, b, ids, dst):
    """the raw call with a sentinel-filled scratch -> (rc, did the call write the scratch: the general path's quantized activation)"""
    L = gpu.lib.get()
    ca, cb, ci, cd = as_.c(), b.c(), ids.c(), dst.c()
    need = int(L.cllm_mul_mat_wsize(C.byref(ca), C.byref(cb)))
    ws = gpu.Tensor.from_strided(np.full(need + 64, M.SENTINEL, np.uint8), gpu.I32, [(need + 64) // 4], [4])
    rc = L.cllm_op_mul_mat_id(None, C.byref(ca), C.byref(cb), C.byref(ci), C.byref(cd), ws.data_ptr(), ws.buf.nbytes)
    gpu.ops.sync()
    return rc, not untouched(ws)


def b_of(gpu, case, x):
    return dev_a(gpu, x, pad1=16 if case.b == "slot_pad" else 0)


# ---- one token: MUL_MAT_ID ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in M.ONE_TOK if c.epi == 0], ids=name_of)
@device_test
def test_one_token_mul_mat_id_equals_the_oracle(gpu, n_cu, case):
    c, d = case, M.one_tok_data(case)
    path, plan = M.one_tok_plan(c, n_cu)
    assert path == c.want["path"] and (path != "decode_id" or M.holds(plan, c.want)), (path, plan, n_cu)
    as_ = dev_w(gpu, d["w"], c.t, c.K, c.N, c.E, c.w_pad)
    b, ids = b_of(gpu, c, d["x"]), gpu.Tensor.from_numpy(d["ids"])
    dst, exp, mask = dev_out(gpu, d["want"], c.dst_pad)
    rc, general = call_mul_mat_id(gpu, as_, b, ids, dst)
    assert rc == 0, gpu.lib.get().cllm_last_error()
    assert general == (path != "decode_id"), "the one-token kernel was to run" if path == "decode_id" else "the general path was to run"
    check_out(dst, exp, mask)
    same_bits(gpu.ops.mul_mat_id(as_, b, ids), d["want"])


@pytest.mark.parametrize("case", [c for c in M.ONE_TOK if c.epi == 1], ids=name_of)
@device_test
def test_one_token_gate_up_silu_mul_equals_the_oracle(gpu, n_cu, case):
    """the fused launch on a host-made interleaved pack (padded expert stride, padded dst) and through gpu.ops (the device's cllm_pack_rows); where the launcher
    refuses -- features % 8, more than 64 slots, K past 32768 -- nothing is written and the four nodes give the oracle's bits"""
    c, d, ops, L = case, M.one_tok_data(case), gpu.ops, gpu.lib.get()
    path, plan = M.one_tok_plan(c, n_cu)
    assert path == c.want["path"] and (path == "nodes" or M.holds(plan, c.want)), (path, plan, n_cu)
    packed = dev_w(gpu, d["w"], c.t, c.K, 2 * c.N, c.E, c.w_pad)
    b, ids = b_of(gpu, c, d["x"]), gpu.Tensor.from_numpy(d["ids"])
    dst, exp, mask = dev_out(gpu, d["want"], c.dst_pad)
    rc = L.cllm_op_mul_mat_id_silu_mul(None, C.byref(packed.c()), C.byref(b.c()), C.byref(ids.c()), C.byref(dst.c()))
    ops.sync()
    wg, wu = dev_w(gpu, d["wg"], c.t, c.K, c.N, c.E), dev_w(gpu, d["wu"], c.t, c.K, c.N, c.E)
    if path == "decode_id":
        assert rc == 0, L.cllm_last_error()
        check_out(dst, exp, mask)
        same_bits(ops.mul_mat_id_silu_mul(wg, wu, b, ids), d["want"])
    else:
        assert rc == UNSUPPORTED and untouched(dst)
        same_bits(ops.mul(ops.silu(ops.mul_mat_id(wg, b, ids)), ops.mul_mat_id(wu, b, ids)), d["want"])


# ---- one token: down projection + combine -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.COMBINE, ids=name_of)
@device_test
def test_mul_mat_id_combine_equals_the_oracle(gpu, n_cu, case):
    """fused (two slots): one launch, residual absent / present / in place.  Refused (1, 4, 8 slots; K past 32768): CLLM_E_UNSUPPORTED, not a byte written, and the
    two calls cllm_op_mul_mat_id -> cllm_op_moe_combine give the oracle's bits -- as does cllm_op_moe_combine alone on the oracle's expert outputs, in every case"""
    c, d, ops, T, L = case, M.combine_data(case), gpu.ops, gpu.Tensor, gpu.lib.get()
    plan = M.plan_combine(c.t, c.K, c.H, n_cu, c.U)
    assert (plan is not None) == c.want["fused"] and (plan is None or M.holds(plan, c.want)), (plan, n_cu)
    w = dev_w(gpu, d["w"], c.t, c.K, c.H, c.E)
    x, ids, p = T.from_numpy(d["x"]), T.from_numpy(d["ids"]), T.from_numpy(d["probs"])
    resid = lambda: None if d["resid"] is None else T.from_numpy(d["resid"])  # noqa: E731
    if plan is not None:
        r = resid()
        got = ops.mul_mat_id_combine(w, x, ids, p, r, dst=r if c.resid == "inplace" else None)          # raises on CLLM_E_UNSUPPORTED: no fallback behind it
        same_bits(got, d["want"])
        if r is not None and c.resid != "inplace":
            same_bits(r, d["resid"])
    else:
        dst, _, _ = dev_out(gpu, d["want"][None])
        r = resid()
        rc = L.cllm_op_mul_mat_id_combine(None, C.byref(w.c()), C.byref(x.c()), C.byref(ids.c()), C.byref(p.c()), C.byref(r.c()) if r is not None else None, C.byref(dst.c()))
        ops.sync()
        assert rc == UNSUPPORTED and untouched(dst)
        down = ops.mul_mat_id(w, x, ids)
        same_bits(down, d["down"])
        same_bits(ops.moe_combine(down, p, ids, r, dst=r if c.resid == "inplace" else None), d["want"])
    r = resid()
    same_bits(ops.moe_combine(T.from_numpy(d["down"]), p, ids, r), d["want"])


@pytest.mark.parametrize("H,k,T_,E", [(100, 1, 3, 8), (257, 2, 5, 8), (64, 4, 2, 16), (1031, 8, 3, 64), (40, 64, 2, 64)])
@device_test
def test_moe_combine_many_tokens_equals_the_oracle(gpu, H, k, T_, E):
    rng = np.random.default_rng([H, k, T_, E])
    e = rng.standard_normal((T_, k, H)).astype(np.float32)
    pr = np.stack([M.soft_row(rng, E) for _ in range(T_)])
    ids = np.zeros((T_, k), np.int32)
    O.top_k(O.tensor(pr, O.F32, [E, T_]), O.tensor(ids, O.I32, [k, T_]))
    r = rng.standard_normal((T_, H)).astype(np.float32)
    T = gpu.Tensor
    for resid in (None, r):
        got = gpu.ops.moe_combine(T.from_numpy(e), T.from_numpy(pr), T.from_numpy(ids), None if resid is None else T.from_numpy(resid))
        same_bits(got, M.ref_combine(e, pr, ids, resid))


# ---- one token: the router, alone and in front of the gate / up launch --------------------------------------------------------------------------
def node_router(gpu, c, d):
    ops, T = gpu.ops, gpu.Tensor
    xn = ops.rms_norm_mul(T.from_numpy(d["x"]), T.from_numpy(d["gw"]), M.EPS)
    pr = ops.soft_max(ops.mul_mat(T.from_numpy(d["wr"], c.t, [c.K, c.E]), xn))
    return xn, pr, ops.top_k(pr, min(c.k, c.E))


@pytest.mark.parametrize("case", M.ROUTER, ids=name_of)
@device_test
def test_moe_router_equals_the_oracle(gpu, case):
    c, d, ops, T, L = case, M.router_data(case), gpu.ops, gpu.Tensor, gpu.lib.get()
    plan = M.plan_router(c.t, c.K, c.E, c.k)
    x, gw, wr = T.from_numpy(d["x"]), T.from_numpy(d["gw"]), T.from_numpy(d["wr"], c.t, [c.K, c.E])
    if plan is not None:
        xn, pr, ids = ops.moe_router(x, gw, M.EPS, wr, c.k)                            # raises on CLLM_E_UNSUPPORTED
        x2 = T.from_numpy(d["x"])                                                      # in place on x
        gpu.lib.check(L.cllm_op_moe_router(None, C.byref(x2.c()), C.byref(gw.c()), C.c_float(M.EPS), C.byref(wr.c()), C.byref(x2.c()), C.byref(pr.c()), C.byref(ids.c())), "moe_router")
        same_bits(x2, d["xnorm"])
    else:
        assert c.E > 64 or c.K > 16384
        oxn, _, _ = dev_out(gpu, d["xnorm"][None, None])
        opr, _, _ = dev_out(gpu, d["probs"][None, None])
        oid, _, _ = dev_out(gpu, d["ids"][None, None])
        rc = L.cllm_op_moe_router(None, C.byref(x.c()), C.byref(gw.c()), C.c_float(M.EPS), C.byref(wr.c()), C.byref(oxn.c()), C.byref(opr.c()), C.byref(oid.c()))
        ops.sync()
        assert rc == UNSUPPORTED and untouched(oxn) and untouched(opr) and untouched(oid)
        xn, pr, ids = node_router(gpu, c, d)
    same_bits(xn, d["xnorm"])
    same_bits(pr, d["probs"])
    assert np.array_equal(ids.numpy().reshape(-1), d["ids"])


@pytest.mark.parametrize("case", M.ROUTER, ids=name_of)
@device_test
def test_moe_router_gate_up_equals_the_oracle(gpu, n_cu, case):
    c, d, ops, T, L = case, M.router_data(case), gpu.ops, gpu.Tensor, gpu.lib.get()
    plan = M.plan_router_silu(c.t, c.K, 2 * c.F, c.E, c.k, n_cu)
    assert (plan is not None) == c.want["fused"] and (plan is None or M.holds(plan, c.want)), (plan, n_cu)
    x, gw, wr = T.from_numpy(d["x"]), T.from_numpy(d["gw"]), T.from_numpy(d["wr"], c.t, [c.K, c.E])
    wg, wu = dev_w(gpu, d["wg"], c.t, c.K, c.F, c.E), dev_w(gpu, d["wu"], c.t, c.K, c.F, c.E)
    if plan is not None:
        pr, ids, g = ops.moe_router_gate_up(x, gw, M.EPS, wr, wg, wu, c.k)             # raises on CLLM_E_UNSUPPORTED
    else:
        k = min(c.k, c.E)
        packed = dev_w(gpu, M.interleave_rows(d["wg"], d["wu"], c.E), c.t, c.K, 2 * c.F, c.E)
        opr, _, _ = dev_out(gpu, d["probs"][None, None])
        oid, _, _ = dev_out(gpu, d["ids"][None, None])
        og, _, _ = dev_out(gpu, d["g"][None])
        rc = L.cllm_op_moe_router_gate_up(None, C.byref(x.c()), C.byref(gw.c()), C.c_float(M.EPS), C.byref(wr.c()), C.byref(packed.c()), C.byref(opr.c()), C.byref(oid.c()), C.byref(og.c()))
        ops.sync()
        assert rc == UNSUPPORTED and untouched(opr) and untouched(oid) and untouched(og)
        xn, pr, ids = node_router(gpu, c, d)
        xn3, ids2 = xn.view([c.K, 1, 1], [4, 4 * c.K, 4 * c.K]), ids.view([k, 1], [4, 4 * k])
        g = ops.mul(ops.silu(ops.mul_mat_id(wg, xn3, ids2)), ops.mul_mat_id(wu, xn3, ids2))
    same_bits(pr, d["probs"])
    assert np.array_equal(ids.numpy().reshape(-1), d["ids"])
    same_bits(g, d["g"])


# ---- many tokens ----------------------------------------------------------------------------------------------------------------------------
def run_multi(gpu, c, d, want):
    as_ = dev_w(gpu, d["w"], c.t, c.K, c.N, c.E)
    b, ids = gpu.Tensor.from_numpy(d["x"]), dev_a(gpu, d["ids"][None], pad1=c.ids_pad)
    ids = ids.view([c.U, c.T], [4, ids.nb[1]])
    dst, exp, mask = dev_out(gpu, want, *c.dst_pad)
    rc, general = call_mul_mat_id(gpu, as_, b, ids, dst)
    return rc, general, dst, exp, mask


@pytest.mark.parametrize("case", M.MULTI + [M.PAIRS_AT_LIMIT], ids=name_of)
@device_test
def test_many_token_mul_mat_id_equals_the_oracle(gpu, n_cu, case):
    c, d = case, M.multi_data(case)
    path, plan = M.mul_mat_id_path(c.t, c.K, c.N, c.U, c.T, n_cu)
    assert path == c.want["path"] and M.holds(plan, c.want), (path, plan, n_cu)
    rc, general, dst, exp, mask = run_multi(gpu, c, d, d["want"])
    assert rc == 0, gpu.lib.get().cllm_last_error()
    assert general
    check_out(dst, exp, mask)


@device_test
def test_many_token_mul_mat_id_refuses_more_than_65535_pairs(gpu, n_cu):
    c = M.PAIRS_OVER
    assert c.U * c.T == M.MAX_PAIRS + 1 and M.mul_mat_id_path(c.t, c.K, c.N, c.U, c.T, n_cu) == (None, None)
    rng = np.random.default_rng(65536)
    d = {"w": M.rand_blocks(c.t, c.N * c.E, c.K, rng), "x": rng.standard_normal((c.T, 1, c.K)).astype(np.float32), "ids": rng.integers(0, c.E, (c.T, c.U)).astype(np.int32)}
    rc, _, dst, _, _ = run_multi(gpu, c, d, np.zeros((c.T, c.U, c.N), np.float32))
    assert rc == UNSUPPORTED and b"too many (slot, token) pairs" in gpu.lib.get().cllm_last_error()
    assert untouched(dst)


# ---- one token's whole block, in place on the residual stream -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.BLOCKS, ids=name_of)
@device_test
def test_whole_block_in_place_equals_the_oracle(gpu, n_cu, case):
    """cllm_op_moe_router_gate_up -> cllm_op_mul_mat_id_combine back to back, the second reading what the first published, the result written over the residual"""
    c, d, ops, T = case, M.block_data(case), gpu.ops, gpu.Tensor
    assert M.plan_router_silu(c.t, c.K, 2 * c.F, c.E, c.k, n_cu) and M.plan_combine(c.t, c.F, c.K, n_cu, c.k)
    x, gw, wr = T.from_numpy(d["x"].reshape(1, c.K)), T.from_numpy(d["gw"]), T.from_numpy(d["wr"], c.t, [c.K, c.E])
    wg, wu, wd = dev_w(gpu, d["wg"], c.t, c.K, c.F, c.E), dev_w(gpu, d["wu"], c.t, c.K, c.F, c.E), dev_w(gpu, d["wd"], c.t, c.F, c.K, c.E)
    pr, ids, g = ops.moe_router_gate_up(x, gw, M.EPS, wr, wg, wu, c.k)
    ops.mul_mat_id_combine(wd, g, ids.view([c.k, 1], [4, 4 * c.k]), pr.view([c.E, 1], [4, 4 * c.E]), x, dst=x)
    ref = d["ref"]
    same_bits(pr, ref["probs"])
    assert np.array_equal(ids.numpy().reshape(-1), ref["ids"])
    same_bits(g, ref["g"])
    same_bits(x, ref["out"])
