"""GGML_OP_NORM through the reference's own CPU backend (the libraries of tests/ref_ggml.py: oracle/_ref/libggml-cpu.so over libggml-base.so), the inputs the CPU and
the GPU tests of NORM share, and how the two compare a result with the reference's."""
import ctypes as C
from fractions import Fraction

import numpy as np

import ref_ggml as R

_ready = False


def _libs():
    global _ready
    base, cpu = R.libs()
    if not _ready:
        P = C.c_void_p
        for name in ("ggml_norm", "ggml_norm_inplace"):
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P, C.c_float]
        for name in ("ggml_mul", "ggml_add"):
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P, P]
        _ready = True
    return base, cpu


def _run(x, eps, inplace=False, weight=None, bias=None):
    base, cpu = _libs()
    x = np.ascontiguousarray(x, np.float32)
    ne = list(reversed(x.shape)) + [1] * (4 - x.ndim)
    mem = 6 * x.nbytes + 16 * base.ggml_tensor_overhead() + base.ggml_graph_overhead() + (1 << 16)
    ctx = base.ggml_init(R._InitParams(mem, None, False))
    assert ctx
    try:
        def tensor(v, dims):
            t = base.ggml_new_tensor_4d(ctx, R.GGML_TYPE_F32, *dims)
            C.memmove(base.ggml_get_data(t), v.ctypes.data, v.nbytes)
            return t
        a = tensor(x, ne)
        d = (base.ggml_norm_inplace if inplace else base.ggml_norm)(ctx, a, C.c_float(eps))
        if weight is not None:
            d = base.ggml_mul(ctx, d, tensor(np.ascontiguousarray(weight, np.float32), [x.shape[-1], 1, 1, 1]))
            d = base.ggml_add(ctx, d, tensor(np.ascontiguousarray(bias, np.float32), [x.shape[-1], 1, 1, 1]))
        g = base.ggml_new_graph(ctx)
        base.ggml_build_forward_expand(g, d)
        assert cpu.ggml_graph_compute_with_ctx(ctx, g, 1) == 0
        out = np.empty_like(x)
        C.memmove(out.ctypes.data, base.ggml_get_data(d), x.nbytes)
        return out
    finally:
        base.ggml_free(ctx)


def norm(x, eps, inplace=False):
    """the reference's NORM node over x (float32 [..., ne0], up to 4 dimensions), same shape"""
    return _run(x, eps, inplace)


def layer_norm(x, weight, bias, eps):
    """the three nodes of the host's LayerNorm::forward (src/layers.cpp:2153-2204): NORM, MUL(weight [ne0]), ADD(bias [ne0])"""
    return _run(x, eps, False, weight, bias)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def random_rows(rows, n, seed):
    """N(0, 4), 10 % replaced by values spread over +-2^-30 .. 2^30 and +-0"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, n)) * 2.0).astype(np.float32)
    wide = (np.ldexp(rng.uniform(1.0, 2.0, (rows, n)), rng.integers(-30, 30, (rows, n))) * rng.choice([-1.0, 1.0], (rows, n))).astype(np.float32)
    wide[rng.random((rows, n)) < 0.2] = 0.0
    wide[rng.random((rows, n)) < 0.1] *= np.float32(-1.0)          # (-0 among them)
    return np.where(rng.random((rows, n)) < 0.1, wide, x)


def _exact(v):
    return Fraction(float(v))


def _below(miss, f, guess):
    """the largest non-negative float v with f(v) <= miss (f exact and increasing in v), searched from guess"""
    v = np.float32(guess)
    while f(v) > miss:
        v = np.nextafter(v, np.float32(0))
    while f(np.nextafter(v, np.float32(np.inf))) <= miss:
        v = np.nextafter(v, np.float32(np.inf))
    return v


def norm_boundary_rows(n, rows, rng, which):
    """rows on which the ORDER of a double accumulation of NORM decides a float, built the way synth_helpers.rms_boundary_rows is (exact rational arithmetic picks the
    last elements; n >= 32).
    which = "mean": S = sum x_i sits on a float rounding boundary (the midpoint of two neighbouring floats) to ~2^-60.  A quarter of the elements are 32 .. 128 in size,
        either sign (their partial sums are exact doubles, ulp 2^-44 and up); the others, 2^-20 .. 2^-40, have their low bits far below that ulp and are rounded at
        every addition, in any order: the float that (float) S becomes depends on the order.
    which = "var": the same for V / n.  The elements come in adjacent pairs (r, -r), so that the reference's serial S is exactly 0, the mean 0 and every centred
        value the element itself; every second group of 8 starts with a pair of 32 .. 128 (h_g ~ 2^13), the other group sums (2^-21, float ulp 2^-44) are rounded at
        every addition to an accumulator of 2^13 and more, in any order.  The last two groups of 8 hold one pair each, (c, -c) and (f, -f): h = 2 c^2 and 2 f^2
        exactly, the coarse and the fine step onto the boundary."""
    assert n >= 32 and which in ("mean", "var")
    out = np.zeros((rows, n), np.float32)
    for r in range(rows):
        if which == "mean":
            x = (rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-40, -19, n))).astype(np.float32)
            big = rng.random(n) < 0.25
            big[0] = True
            x[big] = (rng.uniform(32.0, 128.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)[big]
            x[n - 2] = x[n - 1] = 0.0
            rest = sum(_exact(v) for v in x[: n - 2])
            m = np.float32(float(rest))
            target = _exact(m) + Fraction(float(abs(np.spacing(m)))) / 2          # the midpoint above m: at most one float spacing above what is there
            if target < rest:
                target += Fraction(float(abs(np.spacing(m))))
            target -= Fraction(float(np.spacing(abs(float(target))))) / 2               # half a double ulp off: no order lands on the tie itself
            for j in (n - 2, n - 1):
                x[j] = _below(target - rest, _exact, float(target - rest))
                rest += _exact(x[j])
        else:
            ng = n // 8
            half = (rng.standard_normal(n // 2) * 2.0 ** -12).astype(np.float32)
            x = np.zeros(n, np.float32)
            x[0: 2 * (n // 2): 2], x[1: 2 * (n // 2): 2] = half, -half      # (an odd n: the last leftover stays 0)
            lead = (rng.uniform(32.0, 128.0, (ng + 1) // 2)).astype(np.float32)
            x[0: 8 * ng: 16], x[1: 8 * ng: 16] = lead, -lead
            x[8 * (ng - 2): 8 * ng] = 0.0
            sq = x * x                                                       # float products; the mean is 0
            t = sq[: 8 * ng].reshape(ng, 8)
            t = t[:, :4] + t[:, 4:]
            h = (t[:, 0] + t[:, 2]) + (t[:, 1] + t[:, 3])
            rest = sum(_exact(v) for v in h) + sum(_exact(v) for v in sq[8 * ng:])
            m = np.float32(float(rest / n) * (1 + 2.0 ** -10))              # a float a little above the variance so far ...
            target = (_exact(m) + Fraction(float(np.spacing(m))) / 2) * n    # ... and the midpoint to its successor, as a sum
            target -= Fraction(float(np.spacing(float(target)))) / 2                     # half a double ulp off: no order lands on the tie itself
            for g in (ng - 2, ng - 1):
                two_sq = lambda v: 2 * _exact(np.float32(v) * np.float32(v))      # noqa: E731
                v = _below(target - rest, two_sq, np.sqrt(float(target - rest) / 2.0))
                x[8 * g], x[8 * g + 1] = v, -v
                rest += two_sq(v)
        out[r] = x
    return out


def overflow_and_constant_rows(n):
    """finite rows whose squares overflow (|x| ~ 1e30: V = inf, scale 0, signed zeros out), whose SUM overflows the float range (mean inf), and rows of identical
    values (variance 0: with eps = 0 that is 0 * inf)"""
    rng = np.random.default_rng(77 + n)
    big = (rng.standard_normal(n) * 1e30).astype(np.float32)
    huge = np.full(n, 3.0e38, np.float32)
    huge[::3] = np.float32(2.5e38)
    rows = [big, -np.abs(big), huge, np.full(n, 1.5, np.float32), np.full(n, -0.0, np.float32), np.zeros(n, np.float32), np.full(n, 1e-30, np.float32),
            np.full(n, np.float32(0.1), np.float32)]
    return np.stack(rows)


def non_finite_rows(n):
    """rows that hold a NaN or an inf somewhere: first, last and an inner element, +inf, -inf, both"""
    rng = np.random.default_rng(99 + n)
    rows = []
    for where, what in ((0, np.nan), (n - 1, np.nan), (n // 2, np.nan), (0, np.inf), (n - 1, -np.inf), (n // 3, np.inf)):
        x = rng.standard_normal(n).astype(np.float32)
        x[where] = what
        rows.append(x)
    x = rng.standard_normal(n).astype(np.float32)
    x[0], x[n - 1] = np.inf, -np.inf
    rows.append(x)
    return np.stack(rows)


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
def differing_words(got, want):
    return int(np.count_nonzero(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)))


def assert_same_words(got, want, what=""):
    """0 differing words"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).reshape(-1) != want.view(np.uint32).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} words differ; (index, got, reference): " + str(
        [(int(i), hex(got.view(np.uint32).reshape(-1)[i]), hex(want.view(np.uint32).reshape(-1)[i])) for i in bad[:8]])


def assert_same_words_nan_for_nan(got, want, what=""):
    """the reference's words where it is finite or inf; a NaN (any payload, any sign) exactly where it gives a NaN.  The payload passes through two reductions whose
    operand order is not part of the contract."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ ({int(np.isnan(got).sum())} vs {int(np.isnan(want).sum())})"
    ok = ~np.isnan(want)
    assert_same_words(got[ok], want[ok], what)
