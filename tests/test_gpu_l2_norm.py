"""GGML_OP_L2_NORM on the device, through the C ABI (cllm_op_l2_norm) via the Python mirror (ops.l2_norm), against the reference's own CPU backend
(tests/ref_l2_group_norm.py): every case is compared through a uint32 view and 0 differing words are allowed.  tests/test_l2_group_norm_model.py settles the arithmetic
on the CPU; this file shows that the two launch shapes compute it: either side of a float4 group, of a wave, of the switch between the wave-per-row and the workgroup
shape (512), of the workgroup's single pass, several groups per thread; row counts that leave waves of the wave-per-row shape idle; in place, strided and unaligned rows;
the rows on which the ORDER of the double sum decides (they take the serial fallback, per wave or by wave 0); rows that hold a NaN, an inf or zeros alone, overflow;
what is declined."""
import numpy as np
import pytest

import ref_l2_group_norm as G
import ref_norm as N
from permuted_views import permuted

pytestmark = pytest.mark.gpu

NE0 = [1, 3, 4, 5, 63, 64, 65, 128, 255, 256, 257, 511, 512, 513, 1024, 1025, 4096, 4100, 8200]
EPS = 1e-6
CLLM_E_INVALID, CLLM_E_UNSUPPORTED = -1, -2
BOUNDARY_ROWS = 24

_cache = {}


def shared(key, make):
    """an input and the reference's result, computed once, shared and left unchanged"""
    if key not in _cache:
        x, want = make()
        x.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (x, want)
    return _cache[key]


def random_case(ne0, rows=6):
    def make():
        x = N.random_rows(rows, ne0, 700 + ne0 + rows)
        return x, G.l2_norm(x, EPS)
    return shared(("random", ne0, rows), make)


def boundary_case(ne0):
    def make():
        x, moved = G.l2_boundary_rows(ne0, BOUNDARY_ROWS // 2, np.random.default_rng(2000 * ne0 + 1))
        x = np.concatenate([x, moved])                                       # either side of the boundary
        return x, G.l2_norm(x, EPS)
    return shared(("boundary", ne0), make)


def run(gpu, x, eps=EPS):
    return gpu.ops.l2_norm(gpu.Tensor.from_numpy(x), eps).numpy().reshape(x.shape)


@pytest.mark.parametrize("ne0", NE0)
def test_l2_norm_has_the_bits_of_the_reference(gpu, ne0):
    x, want = random_case(ne0)
    N.assert_same_words(run(gpu, x), want, f"[{ne0}, 6]")


@pytest.mark.parametrize("rows", [1, 5, 6, 7])
@pytest.mark.parametrize("ne0", [128, 513])
def test_row_counts_that_leave_waves_idle(gpu, ne0, rows):
    """four rows per workgroup of the wave-per-row shape: 1, 5, 6 and 7 rows leave three, three, two and one wave without a row (513: the workgroup shape, one row each)"""
    x, want = random_case(ne0, rows)
    N.assert_same_words(run(gpu, x), want, f"[{ne0}, {rows}]")


def test_the_per_head_shape(gpu):
    """[head_k_dim = 128, heads = 4, tokens = 3]: the query and the key of a gated delta net's linear attention"""
    def make():
        x = N.random_rows(12, 128, 31).reshape(3, 4, 128)
        return x, G.l2_norm(x, EPS)
    x, want = shared(("heads",), make)
    N.assert_same_words(run(gpu, x), want, "[128, 4, 3]")


@pytest.mark.parametrize("eps", [0.0, 1e-12, 1e-5, 3.0])
@pytest.mark.parametrize("ne0", [257, 1025])
def test_other_eps(gpu, ne0, eps):
    """(eps = 3.0 is above some of the rows' lengths: fmaxf takes eps)"""
    x, _ = random_case(ne0)
    N.assert_same_words(run(gpu, x, eps), G.l2_norm(x, eps), f"eps {eps}")


@pytest.mark.parametrize("ne0", [5, 128, 512, 1025, 8200])
def test_in_place(gpu, ne0):
    """dst is src: ggml_l2_norm_inplace"""
    x, want = random_case(ne0)
    t = gpu.Tensor.from_numpy(x)
    out = gpu.ops.l2_norm(t, EPS, dst=t)
    assert out is t
    N.assert_same_words(t.numpy(), want, "in place")


@pytest.mark.parametrize("ne0,pad", [(33, 40), (1000, 1004)])
def test_strided_rows(gpu, ne0, pad):
    """a [ne0, 3] view of a wider buffer, as source and as destination: what lies between the rows is neither read into the sum nor written"""
    rng = np.random.default_rng(ne0)
    wide = (rng.standard_normal((3, pad)) * 2.0).astype(np.float32)
    wide[:, ne0:] = 1e30                                                      # (read into a sum, these would be seen)
    want = G.l2_norm(wide[:, :ne0], EPS)
    whole = gpu.Tensor.from_numpy(wide)
    src = whole.view([ne0, 3], [4, 4 * pad])
    N.assert_same_words(gpu.ops.l2_norm(src, EPS).numpy(), want, "strided source")
    back = np.full((3, pad), 7.0, np.float32)
    dst_buf = gpu.Tensor.from_numpy(back)
    gpu.ops.l2_norm(src, EPS, dst=dst_buf.view([ne0, 3], [4, 4 * pad]))
    got = dst_buf.numpy()
    N.assert_same_words(got[:, :ne0], want, "strided destination")
    assert np.array_equal(got[:, ne0:], back[:, ne0:])
    gpu.ops.l2_norm(src, EPS, dst=src)                                        # and in place
    got = whole.numpy()
    N.assert_same_words(got[:, :ne0], want, "strided, in place")
    assert np.array_equal(got[:, ne0:], wide[:, ne0:])


@pytest.mark.parametrize("ne0", [9, 521])
def test_a_permuted_padded_view(gpu, ne0):
    """[ne0, 3, 2, 2] with padded rows and nb[2] > nb[3] (tests/permuted_views.py), another padding on the destination: the reference's words over the gathered values.
    9: a wave per row; 521: a workgroup per row"""
    def make():
        x = N.random_rows(12, ne0, 709 + ne0).reshape(2, 2, 3, ne0)
        return x, G.l2_norm(x, EPS)
    x, want = shared(("permuted", ne0), make)
    src, _ = permuted(gpu, x, 3)
    dst, read = permuted(gpu, np.zeros_like(x), 7)
    gpu.ops.l2_norm(src, EPS, dst=dst)
    N.assert_same_words(read(), want, "permuted, padded")


@pytest.mark.parametrize("ne0", [33, 128, 1028])
def test_a_row_start_that_is_not_16_byte_aligned(gpu, ne0):
    """a view 4 bytes into its buffer (scalar loads and stores instead of float4), as source and as destination"""
    rng = np.random.default_rng(ne0)
    flat = (rng.standard_normal(2 * ne0 + 1) * 2.0).astype(np.float32)
    want = G.l2_norm(flat[1:].reshape(2, ne0), EPS)
    src = gpu.Tensor.from_numpy(flat).view([ne0, 2], [4, 4 * ne0], 4)
    N.assert_same_words(gpu.ops.l2_norm(src, EPS).numpy(), want, "unaligned source")
    dst_buf = gpu.Tensor.from_numpy(np.full(2 * ne0 + 1, 7.0, np.float32))
    gpu.ops.l2_norm(src, EPS, dst=dst_buf.view([ne0, 2], [4, 4 * ne0], 4))
    got = dst_buf.numpy()
    assert got[0] == 7.0
    N.assert_same_words(got[1:].reshape(2, ne0), want, "unaligned destination")


@pytest.mark.parametrize("ne0", [64, 128, 1000, 4096])
def test_rows_on_a_rounding_boundary(gpu, ne0):
    """rows whose sum of squares sits on a rounding boundary of (float) sum, either side of it (ref_l2_group_norm.l2_boundary_rows; tests/test_l2_group_norm_model.py
    shows that the order decides on them): a tree's total cannot stand.  64 and 128: the wave that owns the row redoes the sum itself, its neighbours in the workgroup
    do not wait for it; 1000 and 4096: wave 0 of the workgroup does.  Out of place and in place (the serial pass re-reads the row before anyone stores to it)."""
    x, want = boundary_case(ne0)
    t = gpu.Tensor.from_numpy(x)
    N.assert_same_words(gpu.ops.l2_norm(t, EPS).numpy(), want, "out of place")
    gpu.ops.l2_norm(t, EPS, dst=t)
    N.assert_same_words(t.numpy(), want, "in place")


@pytest.mark.parametrize("eps", [0.0, EPS])
@pytest.mark.parametrize("ne0", [9, 64, 1000])
def test_edge_rows(gpu, ne0, eps):
    """a NaN in the row (fmaxf drops it: scale = 1 / eps, only the NaN elements and any 0 * inf are NaN), an inf (scale 0), zeros alone (1 / eps), squares that overflow
    or vanish, a sum beyond the float range: the reference's words where it is not NaN, a NaN where it is"""
    def make():
        x = G.l2_edge_rows(ne0)
        with np.errstate(all="ignore"):
            return x, G.l2_norm(x, eps)
    x, want = shared(("edge", ne0, eps), make)
    N.assert_same_words_nan_for_nan(run(gpu, x, eps), want, "edge rows")


def test_an_empty_tensor_is_no_launch(gpu):
    t = gpu.Tensor(gpu.F32, [8, 0])
    assert gpu.ops.l2_norm(t, EPS).ne[:2] == [8, 0]
    t = gpu.Tensor(gpu.F32, [0, 4])
    assert gpu.ops.l2_norm(t, EPS).ne[:2] == [0, 4]


def test_a_non_dense_source_or_destination_is_declined(gpu):
    """nb[0] = 8: CLLM_E_UNSUPPORTED with a message, and the destination keeps what it held"""
    n = 33
    wide = gpu.Tensor.from_numpy(np.arange(2 * n, dtype=np.float32))
    every_other = wide.view([n], [8])
    dense = gpu.Tensor.from_numpy(np.full(n, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.l2_norm(every_other, EPS, dst=dense)
    assert e.value.rc == CLLM_E_UNSUPPORTED and "dense" in str(e.value)
    assert np.array_equal(dense.numpy(), np.full(n, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.l2_norm(dense, EPS, dst=every_other)
    assert e.value.rc == CLLM_E_UNSUPPORTED and "dense" in str(e.value)
    assert np.array_equal(wide.numpy(), np.arange(2 * n, dtype=np.float32))


def test_an_f16_tensor_is_declined(gpu):
    h = gpu.Tensor.from_numpy(np.ones(16, np.float16))
    f = gpu.Tensor.from_numpy(np.full(16, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.l2_norm(h, EPS, dst=f)
    assert e.value.rc == CLLM_E_UNSUPPORTED and "type" in str(e.value)
    assert np.array_equal(f.numpy(), np.full(16, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.l2_norm(f, EPS, dst=h)
    assert e.value.rc == CLLM_E_UNSUPPORTED and "type" in str(e.value)
    assert np.array_equal(h.numpy(), np.ones(16, np.float16))


def test_a_shape_mismatch_is_declined(gpu):
    a = gpu.Tensor.from_numpy(np.ones((2, 16), np.float32))
    d = gpu.Tensor.from_numpy(np.full((2, 8), 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.l2_norm(a, EPS, dst=d)
    assert e.value.rc == CLLM_E_INVALID and "shape" in str(e.value)
    assert np.array_equal(d.numpy(), np.full((2, 8), 7.0, np.float32))


def test_a_null_tensor_is_declined(gpu):
    a = gpu.Tensor.from_numpy(np.ones(16, np.float32))
    L = gpu.lib.get()
    ca = a.c()
    import ctypes as C
    assert L.cllm_op_l2_norm(None, None, C.byref(ca), EPS) == CLLM_E_INVALID
    assert L.cllm_op_l2_norm(None, C.byref(ca), None, EPS) == CLLM_E_INVALID
    assert b"null" in L.cllm_last_error()
    assert np.array_equal(a.numpy(), np.ones(16, np.float32))


@pytest.mark.parametrize("eps", [-1.0, float("nan")])
def test_a_negative_or_nan_eps_is_declined(gpu, eps):
    """the reference asserts eps >= 0 (ops.cpp:4069)"""
    a = gpu.Tensor.from_numpy(np.ones(16, np.float32))
    d = gpu.Tensor.from_numpy(np.full(16, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.l2_norm(a, eps, dst=d)
    assert e.value.rc == CLLM_E_INVALID and "eps" in str(e.value)
    assert np.array_equal(d.numpy(), np.full(16, 7.0, np.float32))
