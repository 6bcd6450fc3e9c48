"""Settles the arithmetic of UNARY(TANH / RELU / SIGMOID / GELU / GELU_QUICK) and SQR on the CPU, before any kernel runs: the host side of
chatllm.cpp_amd/csrc/glibc_math.h -- the very functions the kernels of csrc/ops.hip evaluate per element, and the builder of the two GELU
tables the library uploads -- compiled alone with gcc (tests/unary_host.c, no HIP) and compared bit for bit, NaN payloads included, with the
reference's CPU backend driven through its public ggml API (tests/ref_ggml.py).  Skipped where oracle/_ref has not been built."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref_ggml as R

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")

HERE = os.path.dirname(os.path.abspath(__file__))
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tests/unary_host.c as a shared object that links nothing but libc; uncontracted, as csrc/Makefile compiles the kernels"""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to build the host side of glibc_math.h alone"
    so = str(tmp_path_factory.mktemp("unary_host") / "libunary_host.so")
    r = subprocess.run([gcc, "-O2", "-std=gnu11", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-fno-fast-math",
                        "-o", so, os.path.join(HERE, "unary_host.c")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return C.CDLL(so)


@pytest.fixture(scope="module")
def inputs():
    x = R.full_input_set()
    x.setflags(write=False)
    return x


def host_unary(host, op, x):
    y = np.empty_like(x)
    assert host.uh_unary(C.c_int(op), C.c_long(x.size), P(x), P(y)) == 0
    return y


def differing(a, b):
    return int(np.count_nonzero(a.view(np.uint32) != b.view(np.uint32)))


def test_the_input_set_has_what_it_promises(inputs):
    bits = inputs.view(np.uint32)
    assert inputs.size == 65536 + R.special_values().size + R.threshold_neighbours().size + (1 << 20)
    for b in (0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x007fffff, 0x7f7fffff, 0xff7fffff, 0x41b00000, 0x3f800000, 0x24000000):
        assert b in bits
    assert np.isnan(inputs).sum() > 2000            # the fp16 NaNs, the special ones and about 2^20 / 128 random ones
    halves = R.all_fp16_values()
    ok = ~np.isnan(halves)
    assert np.array_equal(R.fp32_to_fp16(halves[ok]), np.arange(65536, dtype=np.uint32).astype(np.uint16)[ok])      # every non-NaN table index is reached


@pytest.mark.parametrize("name", ["tanh", "relu", "sigmoid", "gelu", "gelu_quick", "sqr"])
def test_host_restatement_has_the_bits_of_the_reference(host, inputs, name):
    """what one thread of k_elementwise computes per element, as host code, against the reference's op node: 0 differing words"""
    ref = R.unary(R.OPS[name], inputs)
    got = host_unary(host, R.OPS[name], inputs)
    bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, [(hex(inputs.view(np.uint32)[i]), hex(got.view(np.uint32)[i]), hex(ref.view(np.uint32)[i])) for i in bad[:8]]


def test_host_built_gelu_tables_equal_the_reference_tables(host):
    """gm_build_gelu_tables against ggml_table_gelu_f16 / ggml_table_gelu_quick_f16 as ggml_cpu_init fills them: all 2 x 65 536 entries"""
    g, q = np.zeros(65536, np.uint16), np.zeros(65536, np.uint16)
    host.uh_build_tables(P(g), P(q))
    rg, rq = R.gelu_tables()
    assert np.count_nonzero(rg) > 30000 and np.count_nonzero(rq) > 30000       # (the reference's tables are filled)
    assert int(np.count_nonzero(g != rg)) == 0
    assert int(np.count_nonzero(q != rq)) == 0


def test_fp16_conversions_are_the_reference_ones(host, inputs):
    """the integer fp32 -> fp16 of the table index and fp16 -> fp32 of the table entry against the reference's portable conversions
    (what its x86-64-v3 build uses for single values), the latter over all 65 536 halves"""
    h = np.empty(inputs.size, np.uint16)
    host.uh_fp32_to_fp16(C.c_long(inputs.size), P(inputs), P(h))
    assert int(np.count_nonzero(h != R.fp32_to_fp16(inputs))) == 0
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    f = np.empty(65536, np.float32)
    host.uh_fp16_to_fp32(C.c_long(65536), P(halves), P(f))
    assert differing(f, R.fp16_to_fp32(halves)) == 0


def test_relu2_is_relu_then_sqr(host):
    x = R.special_values()
    assert differing(host_unary(host, R.SQR, host_unary(host, R.RELU, x)), R.unary(R.SQR, R.unary(R.RELU, x))) == 0
