"""GGML_OP_NORM on the device, through the C ABI (cllm_op_norm) via the Python mirror (ops.norm), against the reference's own CPU backend (tests/ref_norm.py): every case
is compared through a uint32 view and 0 differing words are allowed.  tests/test_norm_model.py settles the arithmetic on the CPU; this file shows that k_norm computes
it: either side of a group of 8, of a wave, of the workgroup's single pass, several groups per thread, in place, strided and unaligned rows, the rows on which the
ORDER of the two double sums decides (they take the serial fallbacks), overflow, constant and non-finite rows, what is declined, and the node sequence of a LayerNorm."""
import numpy as np
import pytest

import ref_norm as N
from permuted_views import permuted

pytestmark = pytest.mark.gpu

NE0 = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1024, 1025, 4096, 4100, 8200]
EPS = 1e-5
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


def random_case(ne0):
    def make():
        x = N.random_rows(6, ne0, 500 + ne0).reshape(2, 3, ne0)
        return x, N.norm(x, EPS)
    return shared(("random", ne0), make)


def boundary_case(ne0, which):
    def make():
        x = N.norm_boundary_rows(ne0, BOUNDARY_ROWS, np.random.default_rng(1000 * ne0 + len(which)), which)
        return x, N.norm(x, EPS)
    return shared(("boundary", ne0, which), make)


@pytest.mark.parametrize("ne0", NE0)
def test_norm_has_the_bits_of_the_reference(gpu, ne0):
    x, want = random_case(ne0)
    got = gpu.ops.norm(gpu.Tensor.from_numpy(x), EPS).numpy()
    N.assert_same_words_nan_for_nan(got, want, f"[2, 3, {ne0}]")            # (ne0 = 1: variance 0, finite here with eps > 0)


@pytest.mark.parametrize("eps", [0.0, 1e-6, 1e-12])
def test_other_eps(gpu, eps):
    x, _ = random_case(257)
    N.assert_same_words(gpu.ops.norm(gpu.Tensor.from_numpy(x), eps).numpy(), N.norm(x, eps), f"eps {eps}")


@pytest.mark.parametrize("ne0", [9, 1025, 8200])
def test_in_place(gpu, ne0):
    """dst is src: the `norm_inplace` the host's LayerNorm uses (src/layers.cpp:854-877)"""
    x, want = random_case(ne0)
    t = gpu.Tensor.from_numpy(x)
    out = gpu.ops.norm(t, EPS, dst=t)
    assert out is t
    N.assert_same_words(t.numpy(), want, "in place")


def test_strided_rows(gpu):
    """a [3, 33] view of a wider buffer, nb[1] = 40 * 4, as source and as destination: what lies between the rows is neither read into the sums nor written"""
    rng = np.random.default_rng(33)
    wide = (rng.standard_normal((3, 40)) * 2.0).astype(np.float32)
    want = N.norm(wide[:, :33], EPS)
    whole = gpu.Tensor.from_numpy(wide)
    src = whole.view([33, 3], [4, 160])
    N.assert_same_words(gpu.ops.norm(src, EPS).numpy(), want, "strided source")
    back = np.full((3, 40), 7.0, np.float32)
    dst_buf = gpu.Tensor.from_numpy(back)
    gpu.ops.norm(src, EPS, dst=dst_buf.view([33, 3], [4, 160]))
    got = dst_buf.numpy()
    N.assert_same_words(got[:, :33], want, "strided destination")
    assert np.array_equal(got[:, 33:], back[:, 33:])
    gpu.ops.norm(src, EPS, dst=src)                                           # and in place
    got = whole.numpy()
    N.assert_same_words(got[:, :33], want, "strided, in place")
    assert np.array_equal(got[:, 33:], wide[:, 33:])


def test_a_permuted_padded_view(gpu):
    """[9, 3, 2, 2] with padded rows and nb[2] > nb[3] (tests/permuted_views.py), another padding on the destination: the reference's words over the gathered values"""
    def make():
        x = N.random_rows(12, 9, 509).reshape(2, 2, 3, 9)
        return x, N.norm(x, EPS)
    x, want = shared(("permuted",), make)
    src, _ = permuted(gpu, x, 3)
    dst, read = permuted(gpu, np.zeros_like(x), 7)
    gpu.ops.norm(src, EPS, dst=dst)
    N.assert_same_words(read(), want, "permuted, padded")


@pytest.mark.parametrize("ne0", [33, 1028])
def test_a_row_start_that_is_not_16_byte_aligned(gpu, ne0):
    """a view 4 bytes into its buffer (scalar loads and stores instead of float4), as source and as destination"""
    rng = np.random.default_rng(ne0)
    flat = (rng.standard_normal(2 * ne0 + 1) * 2.0).astype(np.float32)
    want = N.norm(flat[1:].reshape(2, ne0), EPS)
    src = gpu.Tensor.from_numpy(flat).view([ne0, 2], [4, 4 * ne0], 4)
    N.assert_same_words(gpu.ops.norm(src, EPS).numpy(), want, "unaligned source")
    dst_buf = gpu.Tensor.from_numpy(np.full(2 * ne0 + 1, 7.0, np.float32))
    gpu.ops.norm(src, EPS, dst=dst_buf.view([ne0, 2], [4, 4 * ne0], 4))
    got = dst_buf.numpy()
    assert got[0] == 7.0
    N.assert_same_words(got[1:].reshape(2, ne0), want, "unaligned destination")


@pytest.mark.parametrize("which", ["mean", "var"])
@pytest.mark.parametrize("ne0", [64, 1000, 4096])
def test_rows_on_a_rounding_boundary(gpu, ne0, which):
    """rows whose S ("mean") or V / n ("var") sits on a float rounding boundary (ref_norm.norm_boundary_rows; tests/test_norm_model.py shows that the order decides
    on them): the workgroup's tree totals cannot stand, wave 0 redoes the sum in the reference's order.  Out of place and in place (the serial pass re-reads the row
    before any thread stores).  Without these rows a wrong tree order passes everything else."""
    x, want = boundary_case(ne0, which)
    t = gpu.Tensor.from_numpy(x)
    N.assert_same_words(gpu.ops.norm(t, EPS).numpy(), want, "out of place")
    gpu.ops.norm(t, EPS, dst=t)
    N.assert_same_words(t.numpy(), want, "in place")


@pytest.mark.parametrize("eps", [0.0, EPS])
@pytest.mark.parametrize("ne0", [9, 1000])
def test_overflow_and_constant_rows(gpu, ne0, eps):
    """squares that overflow (V = inf, scale 0, signed zeros out), a sum beyond the float range, rows of identical values (variance 0; eps = 0: 0 * inf): the
    reference's words where it is not NaN, a NaN where it is"""
    def make():
        x = N.overflow_and_constant_rows(ne0)
        return x, N.norm(x, eps)
    x, want = shared(("overflow", ne0, eps), make)
    N.assert_same_words_nan_for_nan(gpu.ops.norm(gpu.Tensor.from_numpy(x), eps).numpy(), want, "overflow / constant rows")


@pytest.mark.parametrize("ne0", [9, 1000])
def test_rows_with_a_nan_or_an_inf_are_nan_everywhere(gpu, ne0):
    """the same NaN positions as the reference, which is every element; payloads are not compared (two reductions whose operand order is not part of the contract)"""
    def make():
        x = N.non_finite_rows(ne0)
        return x, N.norm(x, EPS)
    x, want = shared(("nonfinite", ne0), make)
    assert np.isnan(want).all()
    assert np.isnan(gpu.ops.norm(gpu.Tensor.from_numpy(x), EPS).numpy()).all()


def test_an_empty_tensor_is_no_launch(gpu):
    t = gpu.Tensor(gpu.F32, [8, 0])
    assert gpu.ops.norm(t, EPS).ne[:2] == [8, 0]


def test_a_non_dense_source_or_destination_is_declined(gpu):
    """nb[0] = 8: CLLM_E_UNSUPPORTED with a message, and the destination keeps what it held"""
    n = 33
    wide = gpu.Tensor.from_numpy(np.arange(2 * n, dtype=np.float32))
    every_other = wide.view([n], [8])
    dense = gpu.Tensor.from_numpy(np.full(n, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.norm(every_other, EPS, dst=dense)
    assert e.value.rc == CLLM_E_UNSUPPORTED and "dense" in str(e.value)
    assert np.array_equal(dense.numpy(), np.full(n, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.norm(dense, EPS, dst=every_other)
    assert e.value.rc == CLLM_E_UNSUPPORTED and "dense" in str(e.value)
    assert np.array_equal(wide.numpy(), np.arange(2 * n, dtype=np.float32))


def test_an_f16_tensor_is_declined(gpu):
    h = gpu.Tensor.from_numpy(np.ones(16, np.float16))
    f = gpu.Tensor.from_numpy(np.full(16, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.norm(h, EPS, dst=f)
    assert e.value.rc == CLLM_E_UNSUPPORTED
    assert np.array_equal(f.numpy(), np.full(16, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.norm(f, EPS, dst=h)
    assert e.value.rc == CLLM_E_UNSUPPORTED


def test_a_shape_mismatch_is_declined(gpu):
    a = gpu.Tensor.from_numpy(np.ones((2, 16), np.float32))
    d = gpu.Tensor.from_numpy(np.full((2, 8), 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.norm(a, EPS, dst=d)
    assert e.value.rc == CLLM_E_INVALID
    assert np.array_equal(d.numpy(), np.full((2, 8), 7.0, np.float32))


@pytest.mark.parametrize("eps", [-1.0, float("nan")])
def test_a_negative_or_nan_eps_is_declined(gpu, eps):
    """the reference asserts eps >= 0 (ops.cpp:3661)"""
    a = gpu.Tensor.from_numpy(np.ones(16, np.float32))
    d = gpu.Tensor.from_numpy(np.full(16, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.norm(a, eps, dst=d)
    assert e.value.rc == CLLM_E_INVALID and "eps" in str(e.value)
    assert np.array_equal(d.numpy(), np.full(16, 7.0, np.float32))


def test_layer_norm_node_sequence(gpu):
    """NORM, MUL(weight [ne0]), ADD(bias [ne0]) as three launches -- what the module dispatches for the host's LayerNorm -- against the reference's three nodes, at
    Phi-2's width"""
    rng = np.random.default_rng(2560)
    x = (rng.standard_normal((5, 2560)) * 2.0 + 0.1).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(2560)).astype(np.float32)
    b = (0.1 * rng.standard_normal(2560)).astype(np.float32)
    T, ops = gpu.Tensor, gpu.ops
    got = ops.add(ops.mul(ops.norm(T.from_numpy(x), EPS), T.from_numpy(w)), T.from_numpy(b)).numpy()
    N.assert_same_words(got, N.layer_norm(x, w, b, EPS), "NORM -> MUL -> ADD")
