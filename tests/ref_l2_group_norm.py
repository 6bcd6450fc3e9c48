"""GGML_OP_L2_NORM and GGML_OP_GROUP_NORM through the reference's own CPU backend (the libraries of tests/ref_ggml.py, one thread, as ref_norm._run), and the inputs the
CPU and the GPU tests of the two nodes share: the rows and groups on which the ORDER of a double accumulation decides a float, and the edge rows."""
import ctypes as C
from fractions import Fraction

import numpy as np

import ref_ggml as R
import ref_norm as N

_ready = False


def _libs():
    global _ready
    base, cpu = R.libs()
    if not _ready:
        P = C.c_void_p
        for name in ("ggml_l2_norm", "ggml_l2_norm_inplace"):
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P, C.c_float]
        for name in ("ggml_group_norm", "ggml_group_norm_inplace"):
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P, C.c_int, C.c_float]
        for name in ("ggml_mul", "ggml_add"):
            getattr(base, name).restype, getattr(base, name).argtypes = P, [P, P, P]
        _ready = True
    return base, cpu


def _run(x, make, weight=None, bias=None):
    """one graph, one thread: make(base, ctx, a) is the node; weight and bias ([C]) follow it as MUL and ADD by a [1, 1, C] tensor"""
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
        d = make(base, ctx, tensor(x, ne))
        if weight is not None:
            d = base.ggml_mul(ctx, d, tensor(np.ascontiguousarray(weight, np.float32), [1, 1, ne[2], 1]))
            d = base.ggml_add(ctx, d, tensor(np.ascontiguousarray(bias, np.float32), [1, 1, ne[2], 1]))
        g = base.ggml_new_graph(ctx)
        base.ggml_build_forward_expand(g, d)
        assert cpu.ggml_graph_compute_with_ctx(ctx, g, 1) == 0
        out = np.empty_like(x)
        C.memmove(out.ctypes.data, base.ggml_get_data(d), x.nbytes)
        return out
    finally:
        base.ggml_free(ctx)


def l2_norm(x, eps, inplace=False):
    """the reference's L2_NORM node over x (float32 [..., ne0], up to 4 dimensions), same shape"""
    return _run(x, lambda base, ctx, a: (base.ggml_l2_norm_inplace if inplace else base.ggml_l2_norm)(ctx, a, C.c_float(eps)))


def group_norm(x, n_groups, eps, inplace=False):
    """the reference's GROUP_NORM node over x (float32 [ne3, C, ne1, ne0] in numpy order), same shape"""
    assert x.ndim == 4
    return _run(x, lambda base, ctx, a: (base.ggml_group_norm_inplace if inplace else base.ggml_group_norm)(ctx, a, int(n_groups), C.c_float(eps)))


def group_norm_affine(x, n_groups, eps, weight, bias):
    """the three nodes of the host's GroupNorm::forward (src/layers.cpp:2153-2207): GROUP_NORM, MUL and ADD by a [1, 1, C] view of weight and bias"""
    assert x.ndim == 4
    return _run(x, lambda base, ctx, a: base.ggml_group_norm(ctx, a, int(n_groups), C.c_float(eps)), weight, bias)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
GROUP_SHAPES = [([7, 3, 6, 2], 3), ([64, 1, 8, 1], 2), ([33, 5, 5, 2], 4), ([16, 16, 32, 1], 32), ([1, 1, 4, 1], 2), ([4100, 3, 2, 1], 1)]      # (ne, n_groups)


def random_tensor(ne, seed):
    """ref_norm.random_rows in the numpy shape of ne = [ne0, ne1, C, ne3]"""
    return N.random_rows(ne[1] * ne[2] * ne[3], ne[0], seed).reshape(ne[3], ne[2], ne[1], ne[0])


def _sq(v):
    """the float product the loops add, exactly"""
    v = np.float32(v)
    return Fraction(float(v * v))


def _serial(t):
    """t[0] + t[1] + ... in float64, one by one in index order (accumulate adds that way), from +0.0"""
    t = np.asarray(t, np.float64)
    return float(np.add.accumulate(t)[-1]) if t.size else 0.0


def _up(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


def _last_below(upper, hi):
    """the largest float32 v in [0, hi) for which upper(v) is False; upper is monotonic (False ... False True ... True), upper(0) is False and upper(hi) is True.
    Non-negative floats are ordered as their bit patterns are."""
    assert not upper(np.float32(0)) and upper(np.float32(hi)), "the boundary is not between 0 and the coarse element"
    lo, hi = 0, int(np.float32(hi).view(np.uint32))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if upper(np.uint32(mid).view(np.float32)):
            hi = mid
        else:
            lo = mid
    return np.uint32(lo).view(np.float32)


def _l2_scale(s):
    with np.errstate(all="ignore"):
        return np.float32(1) / np.sqrt(np.float32(s))


def _norm_scale(var, eps):
    with np.errstate(all="ignore"):
        return np.float32(1) / np.sqrt(np.float32(var) + np.float32(eps))


def _midpoint_whose_sides_differ(m, scale):
    """(m, the midpoint of m and its successor) for the first float at or above m on whose two sides `scale` differs: a boundary the OUTPUT can see (the square root
    maps about every second pair of neighbouring floats to one float)"""
    m = np.float32(m)
    while scale(m) == scale(_up(m)):
        m = _up(m)
    return m, (Fraction(float(m)) + Fraction(float(_up(m)))) / 2


def l2_boundary_rows(n, rows, rng):
    """(x, x_moved): rows whose sum of squares sits on a rounding boundary of (float) sum, built as synth_helpers.rms_boundary_rows is (n >= 8): x[0] = 64, so that the
    accumulator is 4096 and up and every later square (2^-24) loses its low bits at every addition, in any order; exact rational arithmetic puts the sum a coarse step
    (x[n-2]) below the midpoint of two floats on whose sides the scale differs; the last element is then the LARGEST float for which the reference's own serial chain
    (which adds it last) still rounds down.  x_moved: the same rows with that element one ulp up -- the serial chain rounds up, which test code asserts against the
    reference itself, so that a builder which misses the boundary cannot pass silently."""
    assert n >= 8
    out = np.zeros((rows, n), np.float32)
    moved = np.zeros((rows, n), np.float32)
    for r in range(rows):
        x = (rng.standard_normal(n) * 2.0 ** -12).astype(np.float32)
        x[0] = np.float32(64.0)
        x[n - 2] = x[n - 1] = 0.0
        rest = sum(_sq(v) for v in x[: n - 2])
        m, mid = _midpoint_whose_sides_differ(np.float32(float(rest) * (1 + 2.0 ** -10)), _l2_scale)
        c = N._below(mid - rest, _sq, np.sqrt(float(mid - rest)))
        x[n - 2] = np.nextafter(c, np.float32(0))                     # one ulp short: what is missing (~2^-21) stays far above what the additions round (~2^-38)
        before = _serial((x[: n - 1] * x[: n - 1]).astype(np.float64))
        x[n - 1] = _last_below(lambda v: np.float32(before + float(np.float32(v) * np.float32(v))) > m, x[n - 2])
        out[r] = moved[r] = x
        moved[r, n - 1] = _up(x[n - 1])
    return out, moved


def _group_totals(rows_of_terms):
    """the two-level chain of GROUP_NORM up to, not including, the last row: (the rows' totals added serially, the last row's terms)"""
    return _serial([_serial(t) for t in rows_of_terms[:-1]]), rows_of_terms[-1]


def group_boundary(ne0, ne1, step, count, rng, which, eps):
    """(x, x_moved), float32 [count, step * ne1 * ne0]: `count` groups of `step` channels of ne1 rows of ne0 (ne0 a multiple of 4, 8 and up), each laid out as the group lies
    in a dense tensor, on which the ORDER of a double accumulation of GROUP_NORM decides a float.
    which = "mean": S puts (float)(S / N) on a rounding boundary.  Elements as in ref_norm.norm_boundary_rows: a quarter 32 .. 128 in size, either sign, the others 2^-20
        .. 2^-40, rounded at every addition in any order; the last two elements of the group are the coarse and the fine step.
    which = "var": adjacent pairs (r, -r), so that every row's chain and S are exactly 0, the mean is 0 and every centred value the element itself; V puts
        (float)(V / N) on a boundary on whose two sides the scale differs.  Every row starts with a pair of 32 .. 128, the others are 2^-12; the last two pairs (c, -c)
        and (f, -f) are the coarse and the fine step.
    The fine step is the LARGEST float for which the reference's own two-level chain still rounds down; x_moved has it one ulp up (both elements of the pair)."""
    assert ne0 % 4 == 0 and ne0 >= 8 and which in ("mean", "var")
    n = ne0 * ne1 * step
    out = np.zeros((count, n), np.float32)
    moved = np.zeros((count, n), np.float32)
    for k in range(count):
        if which == "mean":
            x = (rng.standard_normal(n) * np.ldexp(1.0, rng.integers(-40, -19, n))).astype(np.float32)
            big = rng.random(n) < 0.25
            big[0] = True
            x[big] = (rng.uniform(32.0, 128.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)[big]
            x[n - 2] = x[n - 1] = 0.0
            rest = sum(N._exact(v) for v in x)
            m = np.float32(float(rest / n))
            if (Fraction(float(m)) + Fraction(float(_up(m)))) / 2 * n <= rest:
                m = _up(m)
            mid = (Fraction(float(m)) + Fraction(float(_up(m)))) / 2 * n
            x[n - 2] = N._below((mid - rest) * (1 - Fraction(1, 4096)), N._exact, float(mid - rest))      # what is missing stays far above what the additions round
            so_far, last = _group_totals(x.astype(np.float64).reshape(-1, ne0))
            before = _serial(last[:-1])

            def upper(v, so_far=so_far, before=before, m=m):
                return np.float32((so_far + (before + float(np.float32(v)))) / float(n)) > m
            x[n - 1] = _last_below(upper, x[n - 2])
            out[k] = moved[k] = x
            moved[k, n - 1] = _up(x[n - 1])
        else:
            half = (rng.standard_normal(n // 2) * 2.0 ** -12).astype(np.float32)
            half[:: ne0 // 2] = rng.uniform(32.0, 128.0, ne1 * step).astype(np.float32)
            x = np.zeros(n, np.float32)
            x[0::2], x[1::2] = half, -half
            x[n - 4:] = 0.0
            rest = sum(_sq(v) for v in x)
            m, mid = _midpoint_whose_sides_differ(np.float32(float(rest / n) * (1 + 2.0 ** -10)), lambda var: _norm_scale(var, eps))
            mid *= n
            two_sq = lambda v: 2 * _sq(v)      # noqa: E731
            c = np.nextafter(N._below(mid - rest, two_sq, np.sqrt(float(mid - rest) / 2.0)), np.float32(0))
            x[n - 4], x[n - 3] = c, -c
            so_far, last = _group_totals((x * x).astype(np.float64).reshape(-1, ne0))
            before = _serial(last[:-2])

            def upper(v, so_far=so_far, before=before, m=m):
                q = float(np.float32(v) * np.float32(v))
                return np.float32((so_far + ((before + q) + q)) / float(n)) > m
            f = _last_below(upper, c)
            x[n - 2], x[n - 1] = f, -f
            out[k] = moved[k] = x
            moved[k, n - 2], moved[k, n - 1] = _up(f), -_up(f)
    return out, moved


def as_groups(flat, ne0, ne1, step, n_groups):
    """[ne3 * n_groups, step * ne1 * ne0] groups as the dense tensor [ne3, n_groups * step, ne1, ne0] whose groups they are"""
    return np.ascontiguousarray(flat.reshape(-1, n_groups * step, ne1, ne0))


def l2_edge_rows(n):
    """what ops.cpp:4086 does with rows that hold a NaN (fmaxf drops it: scale = 1 / eps), an inf (scale = 0), zeros alone (scale = 1 / eps), squares that overflow
    (sum = inf) or vanish, and a sum beyond the float range"""
    return np.concatenate([N.non_finite_rows(n), N.overflow_and_constant_rows(n), np.full((1, n), 1e-25, np.float32)])


def group_edge_tensor(ne0, ne1):
    """[1, 2 * rows, ne1, ne0], two channels per group: every kind of ref_norm.overflow_and_constant_rows and non_finite_rows as one group each"""
    rows = np.concatenate([N.overflow_and_constant_rows(2 * ne1 * ne0), N.non_finite_rows(2 * ne1 * ne0)])
    return np.ascontiguousarray(rows.reshape(1, 2 * rows.shape[0], ne1, ne0)), rows.shape[0]
