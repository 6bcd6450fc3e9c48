"""Settles the arithmetic of SCALE (with a bias), ADD / MUL / DIV (broadcast), DIAG_MASK_INF and ROPE on the CPU, before any kernel runs: the C
restatement the other tests lean on (oracle/ggml_oracle.c) against the reference's own CPU backend driven through its public ggml API
(tests/ref_ggml.py), word for word, at the cases the GPU tests use (tests/elementwise_cases.py, tests/rope_cases.py).  Skipped where
oracle/_ref has not been built.

What it found: ggml_vec_mad1_f32 rounds once in EVERY element of a row.  The 32-wide body is _mm256_fmadd_ps, and gcc contracts the leftovers'
`x[i]*s + b` into an fma too.  The oracle's (and the kernel's) multiply-then-add differed from it in all 30 cases whose product is inexact
(the three pairs with s not in {0, 1}, at every row length from 1 to 4097): 1 to 6391 words of a case, about a quarter of its elements."""
import numpy as np
import pytest

import elementwise_cases as E
import oracle as O
import ref_ggml as R
import rope_cases as RC

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")


def ne_of(x):
    return list(reversed(x.shape))


def nan_free_words_equal(got, want, what):
    """the oracle runs on the machine the reference runs on: NaNs included, every word is equal"""
    E.assert_same_words(got, want, None, what)


@pytest.mark.parametrize("s,b", E.SCALE_SB)
@pytest.mark.parametrize("ne0", E.SCALE_NE0)
def test_scale_with_a_bias(ne0, s, b):
    x = E.scale_input(ne0)
    want = R.scale_bias(x, s, b)
    got = np.zeros_like(x)
    O.scale(O.tensor(x, O.F32, ne_of(x)), O.tensor(got, O.F32, ne_of(x)), s, b)
    nan_free_words_equal(got, want, f"scale ne0 {ne0} s {s} b {b}")


@pytest.mark.parametrize("ne0", [7, 33, 100, 4097])
def test_the_reference_rounds_a_biased_scale_once_in_body_and_tail(ne0):
    """which elements of a row are single-rounded, from the reference's results alone: among the elements where fma(x, s, b) and the rounded
    product plus b differ (finite inputs; the fma is evaluated in double, exact for a float product, and rounded once more -- an element
    where that second rounding could matter is left out), the reference has the fma's bits in the body i0 < (ne0 & ~31) AND in the tail"""
    f = np.float32
    x = (np.random.default_rng(ne0).standard_normal((1, 8, 16, ne0)) * 4).astype(f)        # 128 rows: enough one-element tails that tell
    s, b = f(0.3), f(0.7)
    want = R.scale_bias(x, s, b)
    exact = x.astype(np.float64) * np.float64(s) + np.float64(b)             # product exact; the sum rounded to double
    fused = exact.astype(f)
    safe = np.abs(exact - fused.astype(np.float64)) < 0.49 * np.abs(np.spacing(fused)).astype(np.float64)      # not next to a float tie: double rounding cannot bite
    unfused = (x * s + b).astype(f)
    tells = safe & (fused.view(np.uint32) != unfused.view(np.uint32))
    body = np.arange(ne0) < (ne0 & ~31)
    assert tells[..., ~body].sum() > 0 and (ne0 < 32 or tells[..., body].sum() > 0)
    assert np.array_equal(want[tells], fused[tells])


@pytest.mark.parametrize("a_ne,b_ne", E.BROADCAST_CASES + [E.BIG_CASE], ids=str)
@pytest.mark.parametrize("op", E.BINARY_OPS)
def test_binary_broadcast(op, a_ne, b_ne):
    a, b = E.binary_inputs(op, a_ne, b_ne)
    want = R.binary(op, a, b)
    got = np.zeros_like(a)
    getattr(O, op)(O.tensor(a, O.F32, a_ne), O.tensor(b, O.F32, b_ne), O.tensor(got, O.F32, a_ne))
    nan_free_words_equal(got, want, f"{op} {a_ne} {b_ne}")
    masked = int(E.invalid(want, a, E.repeated(b, a.shape)).sum())
    print(f"{op} a {a_ne} b {b_ne}: {masked} invalid-operation NaNs of {a.size}")
    assert masked * 100 < a.size                         # what the GPU tests will mask stays under 1 %


@pytest.mark.parametrize("ne,n_past", E.DIAG_CASES, ids=str)
def test_diag_mask_inf(ne, n_past):
    x = E.diag_input(ne)
    want = R.diag_mask_inf(x, n_past)
    got = np.zeros_like(x)
    O.diag_mask_inf(O.tensor(x, O.F32, ne), O.tensor(got, O.F32, ne), n_past)
    nan_free_words_equal(got, want, f"diag_mask_inf {ne} {n_past}")
    i0, i1 = np.arange(ne[0])[None, :], np.arange(ne[1])[:, None]
    assert np.array_equal(np.isneginf(want) & ~np.isneginf(x), np.broadcast_to(i0 > n_past + i1, x.shape) & ~np.isneginf(x))


def oracle_rope(case, inplace):
    """(result, parent after) of oracle.rope over the same view"""
    parent = np.array(case.parent)
    src = O.tensor(parent, O.F32, case.ne, case.nb, case.offset)
    if inplace:
        O.rope(src, case.pos, case.ff, src, **case.params)
        shape = tuple(reversed(case.ne))
        out = np.lib.stride_tricks.as_strided(parent.reshape(-1)[case.offset // 4:], shape, tuple(reversed(case.nb))).copy()
    else:
        out = np.zeros(tuple(reversed(case.ne)), np.float32)
        O.rope(src, case.pos, case.ff, O.tensor(out, O.F32, case.ne), **case.params)
    return out, parent


ROPE_CASES = RC.layout_cases() + RC.n_dims_cases() + RC.parameter_cases() + RC.sweep_cases()


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("case", ROPE_CASES, ids=repr)
def test_rope(case, inplace):
    want, want_parent = R.rope(case.parent, case.ne, case.nb, case.offset, case.pos, case.ff, case.params, inplace)
    got, got_parent = oracle_rope(case, inplace)
    assert np.isfinite(want).all()
    nan_free_words_equal(got, want, f"rope {case}")
    nan_free_words_equal(got_parent, want_parent, f"rope {case}: the parent buffer")
    if not inplace:
        assert np.array_equal(want_parent.view(np.uint32), case.parent.view(np.uint32))


def test_the_sweeps_cross_every_threshold_of_sincosf():
    """each range has angles on both sides of the threshold it is named after; the sweep as a whole has every code path of gm_sincosf"""
    by = {c.name: RC.sweep_angles(c) for c in RC.sweep_cases()}
    for name, t in (("across_2^-12", 2.0 ** -12), ("across_pi/4", np.float32(np.pi / 4)), ("across_120", 120.0)):
        a = by[name]
        assert (a < t).sum() > 10000 and (a >= t).sum() > 10000, name
    assert np.array_equal(np.diff(by["across_pi/4"].view(np.uint32).astype(np.int64)), np.ones(RC.SWEEP_TOKENS - 1))       # consecutive floats
    assert np.array_equal(np.diff(by["across_120"].view(np.uint32).astype(np.int64)), np.ones(RC.SWEEP_TOKENS - 1))
    assert by["large_to_2^31"].max() == 2.0 ** 31 and (by["large_to_2^31"] >= 120).sum() > 65000
    for name in ("negative_0_to_-128", "negative_large", "random_int32"):
        assert (by[name] < -120).sum() > 1000, name
    assert (np.abs(by["negative_0_to_-128"]) < np.pi / 4).sum() > 100
