"""The cases that tests/test_elementwise_model.py (CPU: oracle against the reference) and tests/test_gpu_elementwise.py, tests/test_gpu_rope.py
(the kernels against the reference) share: shapes, inputs, the mask of invalid-operation NaNs and the word-for-word comparison.
Arrays are in numpy order (reversed ne), always 4-D for the element-wise ops."""
import numpy as np

F32_SPECIALS = np.array([0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7f7fffff, 0xff7fffff], np.uint32).view(np.float32)


def activations(shape, seed):
    """the form of test_gpu_unary.inputs: activations of the usual size, a quarter of them replaced by random bit patterns (huge, tiny, NaN)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = (rng.standard_normal(n) * 4.0).astype(np.float32)
    bits = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.where(rng.random(n) < 0.25, bits, x).reshape(shape)


def shape_of(ne):
    return tuple(reversed(list(ne) + [1] * (4 - len(ne))))


def repeated(b, shape):
    """b as the reference repeats it into `shape`: element i of the result is b[i % b.shape] in every dimension"""
    return np.tile(b, [s // t for s, t in zip(shape, b.shape)])


def invalid(ref, *operands):
    """the elements that are NaN in the reference although no input element is: inf*0, inf-inf, 0/0, inf/inf.  From the inputs and the
    reference alone.  Their sign and payload are the machine's default NaN, which x86 and gfx950 need not share: compared as `both NaN`"""
    m = np.isnan(ref)
    for o in operands:
        m &= ~np.isnan(o)
    return m


def assert_same_words(got, want, mask=None, what=""):
    """0 differing uint32 words outside the mask; NaN in both inside it.  The masked share must be under 1 %"""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.size == want.size, (got.size, want.size)
    mask = np.zeros(want.size, bool) if mask is None else mask.reshape(-1)
    assert mask.sum() * 100 < want.size or not mask.any(), f"{what}: {int(mask.sum())} of {want.size} elements are invalid-operation NaNs: 1 % or more"
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero((g != w) & ~mask)
    assert bad.size == 0, f"{what}: {bad.size} differing words of {want.size}; (index, got, reference): " + str([(int(i), hex(g[i]), hex(w[i])) for i in bad[:8]])
    assert np.isnan(got[mask]).all(), f"{what}: an invalid operation of the reference is not NaN here"


# ---- SCALE ---------------------------------------------------------------------------------------------------------------------------------
# either side of one and of two 32-wide steps of ggml_vec_mad1_f32's vector body, a row without a body, a long row with a one-element tail
SCALE_NE0 = [1, 7, 31, 32, 33, 63, 64, 65, 100, 4097]
SCALE_NE1, SCALE_NE2 = 3, 2
SCALE_SB = [(0.3, 0.0), (0.3, 0.7), (-1.7, 1e-3), (1.0 / 3.0, -5.0), (1.0, 1.0), (0.0, 2.0)]


def scale_input(ne0):
    """[1, 2, 3, ne0]; rows of 63 and more also hold +-inf, +-0, subnormals and +-FLT_MAX (2 infinities in >= 378 elements: inf * 0 stays
    under 1 %)"""
    x = activations((1, SCALE_NE2, SCALE_NE1, ne0), 2000 + ne0)
    n = x.size
    if ne0 >= 63:
        x.reshape(-1)[[(k * n) // 8 + 5 for k in range(8)]] = F32_SPECIALS
    return x


# ---- ADD / MUL / DIV -----------------------------------------------------------------------------------------------------------------------
BINARY_OPS = ["add", "mul", "div"]
A_NE = [33, 5, 3, 2]
# full, a row, a scalar, broadcast in some of dims 1-3 and full in others, three repeats along ne0
B_NES = [[33, 5, 3, 2], [33, 1, 1, 1], [1, 1, 1, 1], [1, 5, 1, 1], [33, 1, 3, 1], [33, 5, 1, 2], [11, 5, 3, 2], [1, 1, 3, 2]]
# a of row length 1, 8 and 4097 against a row vector; [4099, 513]: 2 102 787 elements, past one trip of the kernel's 8192 x 256 grid-stride loop
ROW_CASES = [([1, 5, 3, 2], [1, 1, 1, 1]), ([8, 5, 3, 2], [8, 1, 1, 1]), ([4097, 3, 2, 1], [4097, 1, 1, 1])]
BIG_CASE = ([4099, 513, 1, 1], [4099, 1, 1, 1])
BROADCAST_CASES = [(A_NE, b) for b in B_NES] + ROW_CASES
_cache = {}


def binary_inputs(op, a_ne, b_ne):
    """(a, b) for one case, read-only and built once.  DIV's b also holds exact zeros and subnormals.  No element has a NaN in both operands
    (which payload survives is not defined across machines).  Cases of 900 and more elements with a b of 8 and more also get, at chosen
    places, inf + -inf, inf * 0, inf / inf, 0 / 0 and the valid operations next to them (inf + inf, 0 * 0, x / 0)"""
    key = (op, tuple(a_ne), tuple(b_ne))
    if key in _cache:
        return _cache[key]
    seed = 3000 + 7 * sum((i + 1) * v for i, v in enumerate(list(a_ne) + list(b_ne))) + BINARY_OPS.index(op)
    a, b = activations(shape_of(a_ne), seed), activations(shape_of(b_ne), seed + 1)
    rng = np.random.default_rng(seed + 2)
    if op == "div" and b.size >= 8:
        r = rng.random(b.shape)
        b[r < 0.03] = 0.0
        b[(r >= 0.03) & (r < 0.04)] = -0.0
        sub = rng.integers(1, 1 << 23, size=b.shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
        b[(r >= 0.04) & (r < 0.07)] = sub[(r >= 0.04) & (r < 0.07)]
    if a.size >= 900 and b.size >= 8:
        which = repeated(np.arange(b.size).reshape(b.shape), a.shape).reshape(-1)
        j_inf, j_zero = 5, 7
        b.reshape(-1)[j_inf], b.reshape(-1)[j_zero] = np.inf, 0.0
        at_inf, at_zero = np.flatnonzero(which == j_inf), np.flatnonzero(which == j_zero)
        for i, v in zip(at_inf, [-np.inf, 0.0, np.inf, 1.5][:at_inf.size]):
            a.reshape(-1)[i] = v
        for i, v in zip(at_zero, [0.0, -np.inf, -2.5][:at_zero.size]):
            a.reshape(-1)[i] = v
    a[np.isnan(a) & np.isnan(repeated(b, a.shape))] = 1.5
    a.setflags(write=False)
    b.setflags(write=False)
    _cache[key] = (a, b)
    return a, b


# ---- DIAG_MASK_INF -------------------------------------------------------------------------------------------------------------------------
# a square with n_past 0; rows that are masked from column 35 on; n_past == ne0 and far beyond: nothing is masked; ne[3] == 2
DIAG_CASES = [([7, 7, 2, 1], 0), ([40, 6, 3, 2], 34), ([40, 6, 3, 2], 40), ([40, 6, 3, 2], 1000)]


def diag_input(ne):
    return activations(shape_of(ne), 4000 + ne[0])
