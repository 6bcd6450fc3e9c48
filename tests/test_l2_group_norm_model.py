"""Settles the arithmetic of GGML_OP_L2_NORM and GGML_OP_GROUP_NORM on the CPU, before any kernel runs: their part of chatllm.cpp_amd/csrc/norm_order.h -- the text
k_l2_norm, k_l2_norm_wave and k_group_norm (csrc/ops.hip) are built from: the float steps, the serial chains (GROUP_NORM's has two levels), the three interval tests --
compiled alone with gcc (tests/l2_group_norm_host.c, no HIP) and compared word for word with the reference's CPU backend driven through its public ggml API
(tests/ref_l2_group_norm.py).  Two evaluations of each node: the reference's own order, and a deliberately different one (pairwise sums) that stands only where the
interval tests say the order cannot matter and falls back to the serial chains elsewhere, as the device's trees do.  Skipped where oracle/_ref has not been built."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ref_ggml as R
import ref_l2_group_norm as G
import ref_norm as N

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")

HERE = os.path.dirname(os.path.abspath(__file__))
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
L2_NE0 = [1, 2, 7, 8, 9, 63, 64, 65, 128, 1023, 1024, 1025, 4100]
L2_EPS = [0.0, 1e-6, 1e-12]
GN_EPS = [0.0, 1e-6, 1e-5]
EPS = 1e-6
BOUNDARY_ROWS = 24
BOUNDARY_GROUPS = 12
SERIAL, GUARDED, UNGUARDED = 0, 1, 2


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tests/l2_group_norm_host.c as a shared object that links nothing but libc and libm; uncontracted, as csrc/Makefile compiles the kernels (the flags of
    tests/test_norm_model.py)"""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to build norm_order.h alone"
    so = str(tmp_path_factory.mktemp("l2_group_norm_host") / "libl2_group_norm_host.so")
    r = subprocess.run([gcc, "-O2", "-std=gnu11", "-fPIC", "-shared", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off", "-fno-fast-math",
                        "-o", so, os.path.join(HERE, "l2_group_norm_host.c"), "-lm"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return C.CDLL(so)


def l2_serial(host, x, eps):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    host.lg_l2_serial(C.c_long(x.shape[0]), C.c_long(x.shape[1]), P(x), P(y), C.c_float(eps))
    return y


def l2_pairwise(host, x, eps, guarded=True):
    """(result, rows that redid the sum)"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    fb = C.c_long(0)
    assert host.lg_l2_pairwise(C.c_long(x.shape[0]), C.c_long(x.shape[1]), P(x), P(y), C.c_float(eps), C.c_int(1 if guarded else 0), C.byref(fb)) == 0
    return y, int(fb.value)


def gn(host, x, n_groups, eps, mode):
    """(result, groups that redid S, groups that redid V); x: [ne3, C, ne1, ne0].  The destination starts as 7.0: a group without channels leaves it"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.full_like(x, 7.0)
    fb = (C.c_long * 2)()
    ne3, ch, ne1, ne0 = x.shape
    assert host.lg_group_norm(C.c_long(ne0), C.c_long(ne1), C.c_long(ch), C.c_long(ne3), C.c_int(n_groups), P(x), P(y), C.c_float(eps), C.c_int(mode), fb) == 0
    return y, int(fb[0]), int(fb[1])


_cache = {}


def l2_boundary(n):
    """the rows, the rows with the fine element one ulp up, and the reference's results, built once per n and left unchanged"""
    if ("l2", n) not in _cache:
        x, moved = G.l2_boundary_rows(n, BOUNDARY_ROWS, np.random.default_rng(2000 * n + 1))
        got = (x, moved, G.l2_norm(x, EPS), G.l2_norm(moved, EPS))
        for a in got:
            a.setflags(write=False)
        _cache[("l2", n)] = got
    return _cache[("l2", n)]


def gn_boundary(ne0, ne1, step, n_groups, which):
    """the same for GROUP_NORM: BOUNDARY_GROUPS groups as the dense tensor [BOUNDARY_GROUPS / n_groups, n_groups * step, ne1, ne0]"""
    key = ("gn", ne0, ne1, step, n_groups, which)
    if key not in _cache:
        flat, moved = G.group_boundary(ne0, ne1, step, BOUNDARY_GROUPS, np.random.default_rng(3000 * ne0 + 10 * ne1 + len(which)), which, EPS)
        x, xm = G.as_groups(flat, ne0, ne1, step, n_groups), G.as_groups(moved, ne0, ne1, step, n_groups)
        got = (x, xm, G.group_norm(x, n_groups, EPS), G.group_norm(xm, n_groups, EPS))
        for a in got:
            a.setflags(write=False)
        _cache[key] = got
    return _cache[key]


# ---- L2_NORM -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", L2_EPS)
@pytest.mark.parametrize("ne0", L2_NE0)
def test_l2_random_rows_have_the_bits_of_the_reference(host, ne0, eps):
    x = N.random_rows(6, ne0, 300 + ne0)
    want = G.l2_norm(x, eps)
    N.assert_same_words_nan_for_nan(l2_serial(host, x, eps), want, "the reference's order")
    N.assert_same_words_nan_for_nan(l2_pairwise(host, x, eps)[0], want, "pairwise sums behind the interval test")


def test_l2_in_place_node_is_the_same_arithmetic():
    x = N.random_rows(3, 65, 7)
    N.assert_same_words(G.l2_norm(x, EPS, inplace=True), G.l2_norm(x, EPS), "ggml_l2_norm_inplace")


@pytest.mark.parametrize("ne0", [64, 128, 1000, 4096])
def test_l2_boundary_rows_sit_on_the_boundary(ne0):
    """the reference's own result changes, in elements that were not touched, when the fine element moves by one ulp: every row"""
    x, moved, want, want_moved = l2_boundary(ne0)
    for r in range(len(x)):
        assert N.differing_words(want[r, : ne0 - 1], want_moved[r, : ne0 - 1]) > 0, f"row {r} misses the boundary"


@pytest.mark.parametrize("ne0", [64, 128, 1000, 4096])
def test_l2_boundary_rows_have_the_bits_of_the_reference(host, ne0):
    """the rows on which the order decides: the serial chain gives the reference's words; the pairwise order does too, because the interval test sends these rows to the
    serial chain"""
    for x, want in (l2_boundary(ne0)[0::2], l2_boundary(ne0)[1::2]):
        N.assert_same_words(l2_serial(host, x, EPS), want, "the reference's order")
        got, redo = l2_pairwise(host, x, EPS)
        N.assert_same_words(got, want, "pairwise sums behind the interval test")
        assert redo == len(x)                                                 # every such row is caught


def test_l2_unguarded_pairwise_sums_differ_on_boundary_rows(host):
    """-- and without the test it does not: the rows prove something"""
    differ = 0
    for ne0 in (64, 128, 1000, 4096):
        for x, want in (l2_boundary(ne0)[0::2], l2_boundary(ne0)[1::2]):
            got, _ = l2_pairwise(host, x, EPS, guarded=False)
            rows = int(np.count_nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1)))
            print(f"ne0 {ne0}: the pairwise order differs on {rows} of {len(x)} rows")
            differ += rows
    assert differ > 0


def test_l2_ordinary_rows_rarely_fall_back(host):
    """the interval test is not trivially false: rows of ordinary activations keep their pairwise totals"""
    x = (np.random.default_rng(5).standard_normal((2048, 128)) * 2.0).astype(np.float32)
    got, redo = l2_pairwise(host, x, EPS)
    N.assert_same_words(got, G.l2_norm(x, EPS), "pairwise sums behind the interval test")
    assert redo <= 2, redo


@pytest.mark.parametrize("eps", L2_EPS)
@pytest.mark.parametrize("ne0", [1, 9, 64, 1000])
def test_l2_edge_rows(host, ne0, eps):
    """a NaN in the row: fmaxf drops it, scale = 1 / eps, the other elements stay finite (eps > 0) or become inf / 0 * inf (eps = 0); an inf: scale 0; zeros: 1 / eps;
    overflowing and vanishing squares.  The reference's words where it is not NaN, a NaN where it is"""
    x = G.l2_edge_rows(ne0)
    with np.errstate(all="ignore"):
        want = G.l2_norm(x, eps)
        N.assert_same_words_nan_for_nan(l2_serial(host, x, eps), want, "the reference's order")
        N.assert_same_words_nan_for_nan(l2_pairwise(host, x, eps)[0], want, "pairwise sums behind the interval test")


def test_l2_what_the_reference_does_with_nan_inf_and_zero_rows():
    """the three cases of the contract, stated on the reference itself"""
    x = np.ones((3, 8), np.float32)
    x[0, 3] = np.nan
    x[1, 3] = np.inf
    x[2] = 0.0
    y = G.l2_norm(x, 1e-6)
    assert np.isnan(y[0, 3]) and np.array_equal(np.delete(y[0], 3), np.full(7, np.float32(1) / np.float32(1e-6), np.float32))      # scale = 1 / eps
    assert np.isnan(y[1, 3]) and np.array_equal(np.delete(y[1], 3), np.zeros(7, np.float32))                                      # scale = 0; inf * 0
    assert np.array_equal(y[2], np.zeros(8, np.float32))
    y = G.l2_norm(x, 0.0)
    assert np.isnan(y[0, 3]) and np.isinf(np.delete(y[0], 3)).all()                                                              # scale = inf
    assert np.isnan(y[2]).all()                                                                                                  # 0 * inf


# ---- GROUP_NORM ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", GN_EPS)
@pytest.mark.parametrize("ne,n_groups", G.GROUP_SHAPES)
def test_group_norm_random_tensors_have_the_bits_of_the_reference(host, ne, n_groups, eps):
    x = G.random_tensor(ne, 400 + ne[0])
    with np.errstate(all="ignore"):
        want = G.group_norm(x, n_groups, eps)
        got = gn(host, x, n_groups, eps, SERIAL)[0]
        N.assert_same_words_nan_for_nan(got, want, "the reference's order")                   # ([1, 1, 4, 1] / 2 ... groups of one value have variance 0)
        N.assert_same_words_nan_for_nan(gn(host, x, n_groups, eps, GUARDED)[0], want, "pairwise sums behind the interval tests")


def test_group_norm_in_place_node_is_the_same_arithmetic():
    x = G.random_tensor([33, 5, 5, 2], 9)
    N.assert_same_words(G.group_norm(x, 4, EPS, inplace=True), G.group_norm(x, 4, EPS), "ggml_group_norm_inplace")


BOUNDARY_SHAPES = [(64, 2, 2, 2), (1000, 3, 2, 1), (8, 4, 3, 4)]          # (ne0, ne1, channels per group, n_groups)


@pytest.mark.parametrize("which", ["mean", "var"])
@pytest.mark.parametrize("ne0,ne1,step,n_groups", BOUNDARY_SHAPES)
def test_group_norm_boundary_groups_sit_on_the_boundary(ne0, ne1, step, n_groups, which):
    """the reference's own result changes, in elements that were not touched, when the fine step moves by one ulp: every group"""
    x, xm, want, want_moved = gn_boundary(ne0, ne1, step, n_groups, which)
    n = ne0 * ne1 * step
    a, b = want.reshape(-1, n), want_moved.reshape(-1, n)
    for k in range(len(a)):
        assert N.differing_words(a[k, : n - 2], b[k, : n - 2]) > 0, f"group {k} misses the boundary"


@pytest.mark.parametrize("which", ["mean", "var"])
@pytest.mark.parametrize("ne0,ne1,step,n_groups", BOUNDARY_SHAPES)
def test_group_norm_boundary_groups_have_the_bits_of_the_reference(host, ne0, ne1, step, n_groups, which):
    x, xm, want, want_moved = gn_boundary(ne0, ne1, step, n_groups, which)
    for t, w in ((x, want), (xm, want_moved)):
        N.assert_same_words(gn(host, t, n_groups, EPS, SERIAL)[0], w, "the reference's order")
        got, redo_s, redo_v = gn(host, t, n_groups, EPS, GUARDED)
        print(f"{which}: groups that redid S: {redo_s}, V: {redo_v}")
        N.assert_same_words(got, w, "pairwise sums behind the interval tests")
        assert (redo_s if which == "mean" else redo_v) == BOUNDARY_GROUPS     # every such group is caught


@pytest.mark.parametrize("which", ["mean", "var"])
def test_group_norm_unguarded_pairwise_sums_differ_on_boundary_groups(host, which):
    """without the interval tests the other order does not give the reference's words: the groups prove something, of each kind"""
    differ = 0
    for ne0, ne1, step, n_groups in BOUNDARY_SHAPES:
        x, xm, want, want_moved = gn_boundary(ne0, ne1, step, n_groups, which)
        n = ne0 * ne1 * step
        for t, w in ((x, want), (xm, want_moved)):
            got = gn(host, t, n_groups, EPS, UNGUARDED)[0]
            groups = int(np.count_nonzero((got.view(np.uint32).reshape(-1, n) != w.view(np.uint32).reshape(-1, n)).any(axis=1)))
            print(f"[{ne0}, {ne1}] x {step} {which}: the pairwise order differs on {groups} of {BOUNDARY_GROUPS} groups")
            differ += groups
    assert differ > 0


def test_group_norm_ordinary_groups_rarely_fall_back(host):
    x = (np.random.default_rng(6).standard_normal((8, 64, 8, 8)) * 2.0 + 0.25).astype(np.float32)
    got, redo_s, redo_v = gn(host, x, 32, EPS, GUARDED)
    N.assert_same_words(got, G.group_norm(x, 32, EPS), "pairwise sums behind the interval tests")
    assert redo_s + redo_v <= 2, (redo_s, redo_v)


@pytest.mark.parametrize("eps", [0.0, 1e-5])
@pytest.mark.parametrize("ne0,ne1", [(9, 1), (8, 4), (250, 2)])
def test_group_norm_edge_groups(host, ne0, ne1, eps):
    """squares that overflow, a sum beyond the float range, constant groups (variance 0; eps = 0: 0 * inf), groups that hold a NaN or an inf: the reference's words where
    it is not NaN, a NaN where it is"""
    x, n_groups = G.group_edge_tensor(ne0, ne1)
    with np.errstate(all="ignore"):
        want = G.group_norm(x, n_groups, eps)
        N.assert_same_words_nan_for_nan(gn(host, x, n_groups, eps, SERIAL)[0], want, "the reference's order")
        N.assert_same_words_nan_for_nan(gn(host, x, n_groups, eps, GUARDED)[0], want, "pairwise sums behind the interval tests")


def test_an_empty_group_touches_nothing(host):
    """C = 5 in 4 groups: two channels each, the last group has none.  The reference's destination is not compared there, nothing writes it; this side leaves it"""
    x = G.random_tensor([8, 2, 5, 1], 11)
    got = gn(host, x, 4, EPS, SERIAL)[0]
    N.assert_same_words(got, G.group_norm(x, 4, EPS), "every channel is in a group that holds channels")
    got8 = gn(host, x, 8, EPS, SERIAL)[0]                                       # one channel each, three groups without any
    N.assert_same_words(got8, G.group_norm(x, 8, EPS), "more groups than channels")
