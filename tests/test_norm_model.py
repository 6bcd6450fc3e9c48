"""Settles the arithmetic of GGML_OP_NORM on the CPU, before any kernel runs: chatllm.cpp_amd/csrc/norm_order.h -- the text k_norm (csrc/ops.hip) is built from: the float
steps, the group-of-8 tree, the two serial chains, the two interval tests -- compiled alone with gcc (tests/norm_host.c, no HIP) and compared word for word with the
reference's CPU backend driven through its public ggml API (tests/ref_norm.py).  Two evaluations: the reference's own order, and a deliberately different one
(pairwise sums) that stands only where the interval tests say the order cannot matter and falls back to the serial chains elsewhere, as the device's trees do.
Skipped where oracle/_ref has not been built."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref_ggml as R
import ref_norm as N

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")

HERE = os.path.dirname(os.path.abspath(__file__))
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
NE0 = [1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4096, 4100]
EPS = [0.0, 1e-6, 1e-5, 1e-12]
BOUNDARY_ROWS = 24


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tests/norm_host.c as a shared object that links nothing but libc and libm; uncontracted, as csrc/Makefile compiles the kernels"""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to build norm_order.h alone"
    so = str(tmp_path_factory.mktemp("norm_host") / "libnorm_host.so")
    r = subprocess.run([gcc, "-O2", "-std=gnu11", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-fno-fast-math",
                        "-o", so, os.path.join(HERE, "norm_host.c"), "-lm"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return C.CDLL(so)


def serial(host, x, eps):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    host.nh_rows_serial(C.c_long(x.shape[0]), C.c_long(x.shape[1]), P(x), P(y), C.c_float(eps))
    return y


def pairwise(host, x, eps, guarded=True):
    """(result, rows that redid S, rows that redid V)"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    fb = (C.c_long * 2)()
    assert host.nh_rows_pairwise(C.c_long(x.shape[0]), C.c_long(x.shape[1]), P(x), P(y), C.c_float(eps), C.c_int(1 if guarded else 0), fb) == 0
    return y, int(fb[0]), int(fb[1])


_boundary = {}


def boundary(n, which):
    """the rows and the reference's result, built once per (n, kind) and left unchanged"""
    if (n, which) not in _boundary:
        x = N.norm_boundary_rows(n, BOUNDARY_ROWS, np.random.default_rng(1000 * n + len(which)), which)
        want = N.norm(x, 1e-5)
        x.setflags(write=False)
        want.setflags(write=False)
        _boundary[(n, which)] = (x, want)
    return _boundary[(n, which)]


def serial_total(t):
    return float(np.add.accumulate(np.asarray(t, np.float64))[-1])          # (accumulate adds one by one, in index order)


def group_terms(x, mean):
    """what V adds for one row, with numpy float32 arithmetic: the group sums h_g in the reference's float tree, then the leftovers' squares"""
    v = x - np.float32(mean)
    q = v * v
    ng = x.size // 8
    t = q[: 8 * ng].reshape(ng, 8)
    t = t[:, :4] + t[:, 4:]
    return np.concatenate([(t[:, 0] + t[:, 2]) + (t[:, 1] + t[:, 3]), q[8 * ng:]])


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("ne0", NE0)
def test_random_rows_have_the_bits_of_the_reference(host, ne0, eps):
    x = N.random_rows(6, ne0, 100 + ne0)
    want = N.norm(x, eps)
    N.assert_same_words_nan_for_nan(serial(host, x, eps), want, "the reference's order")       # (ne0 = 1, eps = 0: 0 * inf, a NaN on both sides)
    N.assert_same_words_nan_for_nan(pairwise(host, x, eps)[0], want, "pairwise sums behind the interval tests")


def test_in_place_node_is_the_same_arithmetic():
    x = N.random_rows(3, 65, 7)
    N.assert_same_words(N.norm(x, 1e-5, inplace=True), N.norm(x, 1e-5), "ggml_norm_inplace")


@pytest.mark.parametrize("which", ["mean", "var"])
@pytest.mark.parametrize("ne0", [64, 1000, 4096, 4100])
def test_boundary_rows_are_worth_something(ne0, which):
    """plain numpy pairwise sums, no interval test: on at least a quarter of the rows the float differs from the one the serial sum gives"""
    x, _ = boundary(ne0, which)
    differ = 0
    for r in x:
        if which == "mean":
            t = r.astype(np.float64)
            differ += np.float32(serial_total(t)) != np.float32(float(np.sum(t)))
        else:
            mean = np.float32(serial_total(r.astype(np.float64))) / np.float32(ne0)
            t = group_terms(r, mean).astype(np.float64)
            differ += np.float32(serial_total(t) / ne0) != np.float32(float(np.sum(t)) / ne0)
    print(f"ne0 {ne0} {which}: the order decides on {differ} of {len(x)} rows")
    assert 4 * differ >= len(x), (differ, len(x))


@pytest.mark.parametrize("which", ["mean", "var"])
@pytest.mark.parametrize("ne0", [64, 1000, 4096, 4100])
def test_boundary_rows_have_the_bits_of_the_reference(host, ne0, which):
    """the rows on which the order decides: the serial chains give the reference's words; the pairwise order does too, because the interval tests send these rows to
    the serial chains -- and without the tests it does not"""
    x, want = boundary(ne0, which)
    N.assert_same_words(serial(host, x, 1e-5), want, "the reference's order")
    got, redo_s, redo_v = pairwise(host, x, 1e-5)
    print(f"ne0 {ne0} {which}: rows that redid S: {redo_s}, V: {redo_v}")
    N.assert_same_words(got, want, "pairwise sums behind the interval tests")
    assert (redo_s if which == "mean" else redo_v) == len(x)                 # every such row is caught
    unguarded, _, _ = pairwise(host, x, 1e-5, guarded=False)
    assert N.differing_words(unguarded, want) > 0                           # (the guard is what makes the difference)


def test_ordinary_rows_rarely_fall_back(host):
    """the interval tests are not trivially false: rows of ordinary activations keep their pairwise totals"""
    x = (np.random.default_rng(5).standard_normal((512, 1024)) * 2.0 + 0.25).astype(np.float32)
    got, redo_s, redo_v = pairwise(host, x, 1e-5)
    N.assert_same_words(got, N.norm(x, 1e-5), "pairwise sums behind the interval tests")
    assert redo_s + redo_v <= 2, (redo_s, redo_v)


@pytest.mark.parametrize("eps", [0.0, 1e-5])
@pytest.mark.parametrize("ne0", [1, 9, 64, 1000])
def test_overflow_and_constant_rows(host, ne0, eps):
    """squares that overflow, a sum beyond the float range, variance 0 (eps = 0: 0 * inf): the reference's words where it is not NaN, NaN where it is"""
    x = N.overflow_and_constant_rows(ne0)
    with np.errstate(all="ignore"):
        want = N.norm(x, eps)
        N.assert_same_words_nan_for_nan(serial(host, x, eps), want, "the reference's order")
        N.assert_same_words_nan_for_nan(pairwise(host, x, eps)[0], want, "pairwise sums behind the interval tests")


@pytest.mark.parametrize("ne0", [9, 64, 1000])
def test_rows_with_a_nan_or_an_inf_are_nan_everywhere(host, ne0):
    x = N.non_finite_rows(ne0)
    want = N.norm(x, 1e-5)
    assert np.isnan(want).all()                                             # the reference: every element
    assert np.isnan(serial(host, x, 1e-5)).all()
    assert np.isnan(pairwise(host, x, 1e-5)[0]).all()
