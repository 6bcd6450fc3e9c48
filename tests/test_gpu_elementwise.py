"""SCALE (with a bias), ADD / MUL / DIV (every broadcast form, strided, in place, past one trip of the grid-stride loop) and DIAG_MASK_INF on the
device, through the C ABI via the Python mirror, against the reference's own CPU backend (tests/ref_ggml.py): every case is compared through
a uint32 view and 0 differing words are allowed.  The one exception: elements that are NaN in the reference although no input element is
(inf * 0, inf - inf, 0 / 0, inf / inf) are compared as `both NaN` -- the mask comes from the inputs and the reference alone and covers under
1 % of a case (elementwise_cases.assert_same_words asserts that).  tests/test_elementwise_model.py settles the arithmetic on the CPU."""
import numpy as np
import pytest

import elementwise_cases as E
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


def binary_reference(op, a_ne, b_ne):
    a, b = E.binary_inputs(op, a_ne, b_ne)
    want = reference((op, tuple(a_ne), tuple(b_ne)), lambda: R.binary(op, a, b))
    return a, b, want, E.invalid(want, a, E.repeated(b, a.shape))


def column_block(gpu, x, fill):
    """x as a column block of a parent whose rows are 7 floats longer (nb[1] > ne0 * 4, nb[0] == 4), the other floats holding `fill`:
    (the parent tensor, the view, the parent's host copy)"""
    left, extra = 3, 7
    wide = np.full(x.shape[:-1] + (x.shape[-1] + extra,), fill, np.float32)
    wide[..., left:left + x.shape[-1]] = x
    parent = gpu.Tensor.from_numpy(wide)
    ne = list(reversed(x.shape))
    w = 4 * (ne[0] + extra)
    return parent, parent.view(ne, [4, w, w * ne[1], w * ne[1] * ne[2]], 4 * left), wide


# ---- SCALE ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("s,b", E.SCALE_SB)
@pytest.mark.parametrize("ne0", E.SCALE_NE0)
def test_scale_with_a_bias(gpu, ne0, s, b, inplace):
    """x * s + b rounds once wherever the reference's ggml_vec_mad1_f32 does: in every element of a row, its 32-wide body and its leftovers"""
    x = E.scale_input(ne0)
    want = reference(("scale", ne0, s, b), lambda: R.scale_bias(x, s, b))
    t = gpu.Tensor.from_numpy(x)
    out = gpu.ops.scale(t, s, b, dst=t if inplace else None)
    assert (out is t) == inplace
    E.assert_same_words(out.numpy(), want, E.invalid(want, x), f"scale ne0 {ne0} s {s} b {b}")
    if not inplace:
        assert np.array_equal(t.numpy().reshape(-1).view(np.uint32), x.reshape(-1).view(np.uint32))


# ---- ADD / MUL / DIV -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_ne,b_ne", E.BROADCAST_CASES, ids=str)
@pytest.mark.parametrize("op", E.BINARY_OPS)
def test_binary_broadcast(gpu, op, a_ne, b_ne):
    a, b, want, mask = binary_reference(op, a_ne, b_ne)
    got = getattr(gpu.ops, op)(gpu.Tensor.from_numpy(a), gpu.Tensor.from_numpy(b)).numpy()
    E.assert_same_words(got, want, mask, f"{op} {a_ne} {b_ne}")


@pytest.mark.parametrize("op", E.BINARY_OPS)
def test_binary_past_one_trip_of_the_grid_stride_loop(gpu, op):
    """[4099, 513]: 2 102 787 elements for a grid capped at 8192 x 256 threads; the last 5635 are a thread's second element"""
    a_ne, b_ne = E.BIG_CASE
    assert int(np.prod(a_ne)) > 8192 * 256
    a, b, want, mask = binary_reference(op, a_ne, b_ne)
    got = getattr(gpu.ops, op)(gpu.Tensor.from_numpy(a), gpu.Tensor.from_numpy(b)).numpy()
    E.assert_same_words(got, want, mask, f"{op} {a_ne} {b_ne}")


@pytest.mark.parametrize("b_ne", [E.A_NE, [33, 1, 1, 1], [11, 5, 3, 2], [1, 1, 1, 1]], ids=str)
@pytest.mark.parametrize("op", E.BINARY_OPS)
def test_binary_in_place(gpu, op, b_ne):
    """dst is a: the `_inplace` forms the host builds (residual adds, the norm weights)"""
    a, b, want, mask = binary_reference(op, E.A_NE, b_ne)
    ta, tb = gpu.Tensor.from_numpy(a), gpu.Tensor.from_numpy(b)
    out = getattr(gpu.ops, op)(ta, tb, dst=ta)
    assert out is ta
    E.assert_same_words(ta.numpy(), want, mask, f"{op} in place, b {b_ne}")
    assert np.array_equal(tb.numpy().reshape(-1).view(np.uint32), b.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("strided", ["a", "b", "dst", "a_b_dst"])
@pytest.mark.parametrize("op", E.BINARY_OPS)
def test_binary_row_strided_operands(gpu, op, strided):
    """a, b, dst as column blocks of wider parents.  The reference builds its operands dense; the views hold the same values, so the same result
    is expected, and the parent of dst keeps its bytes outside the view"""
    b_ne = [33, 5, 1, 2]
    a, b, want, mask = binary_reference(op, E.A_NE, b_ne)
    ta = column_block(gpu, a, -1.0)[1] if "a" in strided else gpu.Tensor.from_numpy(a)
    tb = column_block(gpu, b, -2.0)[1] if "b" in strided else gpu.Tensor.from_numpy(b)
    if "dst" in strided:
        old = np.arange(a.size, dtype=np.float32).reshape(a.shape) + 0.5
        parent, td, wide = column_block(gpu, old, 77.0)
        getattr(gpu.ops, op)(ta, tb, dst=td)
        after = parent.numpy().reshape(wide.shape)
        E.assert_same_words(after[..., 3:3 + a.shape[-1]], want, mask, f"{op} strided {strided}")
        outside = np.ones(wide.shape, bool)
        outside[..., 3:3 + a.shape[-1]] = False
        assert np.array_equal(after[outside], wide[outside])
    else:
        E.assert_same_words(getattr(gpu.ops, op)(ta, tb).numpy(), want, mask, f"{op} strided {strided}")


# ---- DIAG_MASK_INF -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("ne,n_past", E.DIAG_CASES, ids=str)
def test_diag_mask_inf(gpu, ne, n_past, inplace):
    x = E.diag_input(ne)
    want = reference(("diag", tuple(ne), n_past), lambda: R.diag_mask_inf(x, n_past))
    if n_past >= ne[0]:
        assert np.array_equal(want.view(np.uint32), x.view(np.uint32))          # nothing is masked
    t = gpu.Tensor.from_numpy(x)
    out = gpu.ops.diag_mask_inf(t, n_past, dst=t if inplace else None)
    assert (out is t) == inplace
    E.assert_same_words(out.numpy(), want, None, f"diag_mask_inf {ne} n_past {n_past}")


# ---- what is declined ----------------------------------------------------------------------------------------------------------------------
def declined(gpu, call, dst, rc, word):
    before = dst.raw().copy()
    with pytest.raises(gpu.lib.CllmError) as e:
        call()
    assert e.value.rc == rc and word in str(e.value), str(e.value)
    assert np.array_equal(dst.raw(), before)


@pytest.mark.parametrize("b_ne", [[32, 1, 1, 1], [33, 2, 1, 1], [33, 5, 3, 4], [66, 5, 3, 2]], ids=str)
@pytest.mark.parametrize("op", E.BINARY_OPS)
def test_a_b_that_does_not_repeat_into_a_is_declined(gpu, op, b_ne):
    a, _ = E.binary_inputs(op, E.A_NE, E.A_NE)
    ta, tb = gpu.Tensor.from_numpy(a), gpu.Tensor.from_numpy(np.ones(E.shape_of(b_ne), np.float32))
    dst = gpu.Tensor.from_numpy(np.full(a.shape, 7.0, np.float32))
    declined(gpu, lambda: getattr(gpu.ops, op)(ta, tb, dst=dst), dst, CLLM_E_INVALID, "broadcast")


@pytest.mark.parametrize("op", E.BINARY_OPS + ["scale", "diag_mask_inf"])
def test_a_type_other_than_f32_or_another_shape_of_dst_is_declined(gpu, op):
    shape = E.shape_of(E.A_NE)
    f32 = gpu.Tensor.from_numpy(np.ones(shape, np.float32))
    f16 = gpu.Tensor.from_numpy(np.ones(shape, np.float16))
    i32 = gpu.Tensor.from_numpy(np.ones(shape, np.int32))
    dst = gpu.Tensor.from_numpy(np.full(shape, 7.0, np.float32))
    smaller = gpu.Tensor.from_numpy(np.full(E.shape_of([33, 5, 3, 1]), 7.0, np.float32))
    if op in E.BINARY_OPS:
        run = lambda a, b, d: getattr(gpu.ops, op)(a, b, dst=d)                   # noqa: E731
    elif op == "scale":
        run = lambda a, b, d: gpu.ops.scale(a, 0.5, 0.25, dst=d)                  # noqa: E731
    else:
        run = lambda a, b, d: gpu.ops.diag_mask_inf(a, 2, dst=d)                  # noqa: E731
    declined(gpu, lambda: run(f16, f32, dst), dst, CLLM_E_UNSUPPORTED, "type")
    declined(gpu, lambda: run(f32, f32, f16), f16, CLLM_E_UNSUPPORTED, "type")
    if op in E.BINARY_OPS:
        declined(gpu, lambda: run(f32, i32, dst), dst, CLLM_E_UNSUPPORTED, "type")
    declined(gpu, lambda: run(f32, f32, smaller), smaller, CLLM_E_INVALID, "shape")
