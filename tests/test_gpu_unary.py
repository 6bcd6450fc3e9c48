"""UNARY(TANH / RELU / SIGMOID / GELU / GELU_QUICK) and SQR on the device, through the C ABI (cllm_op_unary, cllm_op_sqr) via the Python
mirror, against the reference's own CPU backend (tests/ref_ggml.py): every case is compared through a uint32 view and 0 differing words
are allowed, NaN payloads and signs included.  tests/test_unary_model.py settles the arithmetic on the CPU; this file shows that the
kernels compute it: tails, bounds, several rows, special values, in place, and what is declined."""
import numpy as np
import pytest

import ref_ggml as R

pytestmark = pytest.mark.gpu

OPS = ["tanh", "relu", "sigmoid", "gelu", "gelu_quick", "sqr"]
# either side of an 8-wide body, either side of a 64-lane wave, a whole workgroup, one past a power of two (more than one workgroup)
NE0 = [1, 7, 8, 9, 31, 33, 256, 4097]
NE1, NE2 = 3, 2
CLLM_E_UNSUPPORTED = -2

_ref_cache = {}


def inputs(ne0):
    """[NE2, NE1, ne0] float32: activations of the usual size, a quarter of them replaced by random bit patterns (huge, tiny, NaN, inf)"""
    rng = np.random.default_rng(1000 + ne0)
    n = NE2 * NE1 * ne0
    x = (rng.standard_normal(n) * 4.0).astype(np.float32)
    bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = np.where(rng.random(n) < 0.25, bits, x)
    return x.reshape(NE2, NE1, ne0)


def special_row():
    return np.concatenate([R.special_values(), R.threshold_neighbours()])


def reference(name, key, x):
    """the reference's result, computed once per (op, input) and shared"""
    if (name, key) not in _ref_cache:
        y = R.unary(R.OPS[name], x)
        y.setflags(write=False)
        _ref_cache[(name, key)] = y
    return _ref_cache[(name, key)]


def run(gpu, name, src, dst=None):
    return gpu.ops.sqr(src, dst) if name == "sqr" else gpu.ops.unary(R.OPS[name], src, dst)


def assert_same_words(got, want, x):
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert bad.size == 0, f"{bad.size} differing words; (x, device, reference): " + str(
        [(hex(x.view(np.uint32).reshape(-1)[i]), hex(got.view(np.uint32).reshape(-1)[i]), hex(want.view(np.uint32).reshape(-1)[i])) for i in bad[:8]])


@pytest.mark.parametrize("ne0", NE0)
@pytest.mark.parametrize("name", OPS)
def test_op_has_the_bits_of_the_reference(gpu, name, ne0):
    x = inputs(ne0)
    got = run(gpu, name, gpu.Tensor.from_numpy(x)).numpy()
    assert got.shape == x.shape
    assert_same_words(got, reference(name, ne0, x), x)


@pytest.mark.parametrize("name", OPS)
def test_special_values_as_one_row(gpu, name):
    """+-0, +-inf, NaNs of either sign with payloads, subnormals, +-FLT_MAX, the GELU clamp, the fp16 range's edges and the neighbours of every
    branch threshold of glibc's tanhf / expm1f / expf"""
    x = special_row()
    got = run(gpu, name, gpu.Tensor.from_numpy(x)).numpy()
    assert_same_words(got, reference(name, "special", x), x)


@pytest.mark.parametrize("name", OPS)
def test_in_place(gpu, name):
    """source and destination are the same buffer: the `_inplace` forms the host uses (src/layers.cpp:405-409)"""
    x = inputs(33)
    t = gpu.Tensor.from_numpy(x)
    out = run(gpu, name, t, t)
    assert out is t
    assert_same_words(t.numpy(), reference(name, 33, x), x)


@pytest.mark.parametrize("name", OPS)
def test_a_non_dense_source_or_destination_is_declined(gpu, name):
    """rows whose elements are not adjacent (nb[0] != 4): CLLM_E_UNSUPPORTED with a message, and the destination keeps what it held"""
    n = 33
    wide = gpu.Tensor.from_numpy(np.arange(2 * n, dtype=np.float32))
    every_other = wide.view([n], [8])
    dense = gpu.Tensor.from_numpy(np.full(n, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        run(gpu, name, every_other, dense)
    assert e.value.rc == CLLM_E_UNSUPPORTED and "dense" in str(e.value)
    assert np.array_equal(dense.numpy(), np.full(n, 7.0, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        run(gpu, name, dense, every_other)
    assert e.value.rc == CLLM_E_UNSUPPORTED
    assert np.array_equal(wide.numpy(), np.arange(2 * n, dtype=np.float32))


@pytest.mark.parametrize("op", [0, 5, 16, 22])       # ABS, ELU, GELU_ERF, COUNT
def test_an_op_outside_the_enum_is_declined(gpu, op):
    x = gpu.Tensor.from_numpy(np.ones(8, np.float32))
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.unary(op, x)
    assert e.value.rc == CLLM_E_UNSUPPORTED and f"op {op}" in str(e.value)
