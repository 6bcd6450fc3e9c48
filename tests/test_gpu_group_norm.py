"""GGML_OP_GROUP_NORM on the device, through the C ABI (cllm_op_group_norm) via the Python mirror (ops.group_norm), against the reference's own CPU backend
(tests/ref_l2_group_norm.py): every case is compared through a uint32 view and 0 differing words are allowed.  tests/test_l2_group_norm_model.py settles the arithmetic
on the CPU; this file shows that k_group_norm computes it: rows that are no multiple of 4, groups of one pass and of several per thread, an uneven last group and groups
without channels, in place, strided and unaligned rows, the groups on which the ORDER of the two double sums decides (wave 0 redoes them as two-level chains), overflow,
constant and non-finite groups, what is declined, and the node sequence of a GroupNorm."""
import ctypes as C

import numpy as np
import pytest

import ref_l2_group_norm as G
import ref_norm as N
from permuted_views import permuted

pytestmark = pytest.mark.gpu

SHAPES = G.GROUP_SHAPES + [([8, 8, 64, 1], 32)]          # the image decoder's [W, H, 512] / 32, scaled down
EPS = 1e-6
CLLM_E_INVALID, CLLM_E_UNSUPPORTED = -1, -2
BOUNDARY_TENSORS = 6

_cache = {}


def shared(key, make):
    """an input and the reference's result, computed once, shared and left unchanged"""
    if key not in _cache:
        x, want = make()
        x.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (x, want)
    return _cache[key]


def ids(shapes):
    return ["x".join(str(v) for v in ne) + f"/{g}" for ne, g in shapes]


def random_case(ne, n_groups):
    def make():
        x = G.random_tensor(ne, 900 + ne[0])
        with np.errstate(all="ignore"):
            return x, G.group_norm(x, n_groups, EPS)
    return shared(("random", tuple(ne), n_groups), make)


def boundary_case(ne, n_groups, which):
    """BOUNDARY_TENSORS tensors of shape ne, every group of every one on the boundary; half of them on its other side (the fine step one ulp up)"""
    def make():
        ne0, ne1, ch, ne3 = ne
        step = ch // n_groups
        flat, moved = G.group_boundary(ne0, ne1, step, BOUNDARY_TENSORS * n_groups * ne3 // 2, np.random.default_rng(3000 * ne0 + 10 * ne1 + len(which)), which, EPS)
        x = G.as_groups(np.concatenate([flat, moved]), ne0, ne1, step, n_groups).reshape(BOUNDARY_TENSORS, ne3, ch, ne1, ne0)
        return x, np.stack([G.group_norm(t, n_groups, EPS) for t in x])
    return shared(("boundary", tuple(ne), n_groups, which), make)


def run(gpu, x, n_groups, eps=EPS):
    return gpu.ops.group_norm(gpu.Tensor.from_numpy(x), n_groups, eps).numpy().reshape(x.shape)


@pytest.mark.parametrize("ne,n_groups", SHAPES, ids=ids(SHAPES))
def test_group_norm_has_the_bits_of_the_reference(gpu, ne, n_groups):
    x, want = random_case(ne, n_groups)
    N.assert_same_words_nan_for_nan(run(gpu, x, n_groups), want, f"{ne} / {n_groups}")


@pytest.mark.parametrize("ne,n_groups", SHAPES, ids=ids(SHAPES))
def test_in_place(gpu, ne, n_groups):
    """dst is src: the `group_norm_inplace` the host's GroupNorm uses by default"""
    x, want = random_case(ne, n_groups)
    t = gpu.Tensor.from_numpy(x)
    out = gpu.ops.group_norm(t, n_groups, EPS, dst=t)
    assert out is t
    N.assert_same_words_nan_for_nan(t.numpy().reshape(x.shape), want, "in place")


@pytest.mark.parametrize("eps", [0.0, 1e-5, 1e-12])
def test_other_eps(gpu, eps):
    x, _ = random_case([33, 5, 5, 2], 4)
    N.assert_same_words(run(gpu, x, 4, eps), G.group_norm(x, 4, eps), f"eps {eps}")


def test_more_groups_than_channels(gpu):
    """C = 5 in 8 groups: one channel each, three groups without any.  Out of place the untouched destination would show a write by a group that has no channels; every
    channel here is in a group, so the whole result is the reference's"""
    x, _ = random_case([33, 5, 5, 2], 4)
    N.assert_same_words(run(gpu, x, 8), G.group_norm(x, 8, EPS), "8 groups of 5 channels")
    N.assert_same_words(run(gpu, x, 5000), G.group_norm(x, 5000, EPS), "5000 groups of 5 channels")


def test_strided_rows_channels_and_batches(gpu):
    """a [30, 3, 4, 2] view of a [40, 4, 5, 3] buffer, as source and as destination, and in place: rows, channels and batches are all strided; what lies outside the
    view is neither read into the sums nor written"""
    rng = np.random.default_rng(40)
    wide = (rng.standard_normal((3, 5, 4, 40)) * 2.0 + 0.5).astype(np.float32)
    inside = np.zeros(wide.shape, bool)
    inside[:2, :4, :3, :30] = True
    wide[~inside] = 1e30                                                      # (read into a sum, these would be seen)
    want = G.group_norm(wide[:2, :4, :3, :30], 2, EPS)
    nb = [4, 160, 640, 3200]
    whole = gpu.Tensor.from_numpy(wide)
    src = whole.view([30, 3, 4, 2], nb)
    N.assert_same_words(gpu.ops.group_norm(src, 2, EPS).numpy().reshape(want.shape), want, "strided source")
    back = np.full(wide.shape, 7.0, np.float32)
    dst_buf = gpu.Tensor.from_numpy(back)
    gpu.ops.group_norm(src, 2, EPS, dst=dst_buf.view([30, 3, 4, 2], nb))
    got = dst_buf.numpy().reshape(wide.shape)
    N.assert_same_words(got[:2, :4, :3, :30], want, "strided destination")
    assert np.array_equal(got[~inside], back[~inside])
    gpu.ops.group_norm(src, 2, EPS, dst=src)
    got = whole.numpy().reshape(wide.shape)
    N.assert_same_words(got[:2, :4, :3, :30], want, "strided, in place")
    assert np.array_equal(got[~inside], wide[~inside])


def test_a_permuted_padded_view(gpu):
    """[5, 3, 4, 2] in 2 groups with padded rows and nb[2] > nb[3] (tests/permuted_views.py), another padding on the destination: the reference's words over the
    gathered values"""
    def make():
        x = G.random_tensor([5, 3, 4, 2], 905)
        return x, G.group_norm(x, 2, EPS)
    x, want = shared(("permuted",), make)
    src, _ = permuted(gpu, x, 3)
    dst, read = permuted(gpu, np.zeros_like(x), 6)
    gpu.ops.group_norm(src, 2, EPS, dst=dst)
    N.assert_same_words(read(), want, "permuted, padded")


@pytest.mark.parametrize("ne0", [33, 1028])
def test_row_starts_that_are_not_16_byte_aligned(gpu, ne0):
    """a view 4 bytes into its buffer, as source and as destination; ne0 = 33: every row starts at another offset from a 16-byte boundary (alignment is decided per row)"""
    rng = np.random.default_rng(ne0)
    n = 2 * 4 * ne0
    flat = (rng.standard_normal(n + 1) * 2.0).astype(np.float32)
    want = G.group_norm(flat[1:].reshape(1, 4, 2, ne0), 2, EPS)
    nb = [4, 4 * ne0, 8 * ne0]
    src = gpu.Tensor.from_numpy(flat).view([ne0, 2, 4], nb, 4)
    N.assert_same_words(gpu.ops.group_norm(src, 2, EPS).numpy().reshape(want.shape), want, "unaligned source")
    dst_buf = gpu.Tensor.from_numpy(np.full(n + 1, 7.0, np.float32))
    gpu.ops.group_norm(src, 2, EPS, dst=dst_buf.view([ne0, 2, 4], nb, 4))
    got = dst_buf.numpy()
    assert got[0] == 7.0
    N.assert_same_words(got[1:].reshape(want.shape), want, "unaligned destination")


BOUNDARY = [([64, 2, 4, 1], 2), ([1000, 3, 2, 2], 1)]


@pytest.mark.parametrize("which", ["mean", "var"])
@pytest.mark.parametrize("ne,n_groups", BOUNDARY, ids=ids(BOUNDARY))
def test_groups_on_a_rounding_boundary(gpu, ne, n_groups, which):
    """groups whose S puts (float)(S / N) on a rounding boundary ("mean"), or whose V does with (float)(V / N) at a mean of exactly 0 ("var"), either side of it
    (ref_l2_group_norm.group_boundary; tests/test_l2_group_norm_model.py shows that the order decides on them): the workgroup's tree totals cannot stand, wave 0 redoes
    the sum as the reference's two-level chain.  Out of place and in place (the serial passes re-read the group before any thread stores)."""
    x, want = boundary_case(ne, n_groups, which)
    for k in range(len(x)):
        t = gpu.Tensor.from_numpy(x[k])
        N.assert_same_words(gpu.ops.group_norm(t, n_groups, EPS).numpy().reshape(want[k].shape), want[k], f"tensor {k}, out of place")
        gpu.ops.group_norm(t, n_groups, EPS, dst=t)
        N.assert_same_words(t.numpy().reshape(want[k].shape), want[k], f"tensor {k}, in place")


@pytest.mark.parametrize("eps", [0.0, 1e-5])
@pytest.mark.parametrize("ne0,ne1", [(9, 1), (250, 2)])
def test_edge_groups(gpu, ne0, ne1, eps):
    """squares that overflow (V = inf, scale 0, signed zeros out), a sum beyond the float range, constant groups (variance 0; eps = 0: 0 * inf), groups that hold a NaN or
    an inf: the reference's words where it is not NaN, a NaN where it is"""
    def make():
        x, n_groups = G.group_edge_tensor(ne0, ne1)
        with np.errstate(all="ignore"):
            return x, G.group_norm(x, n_groups, eps)
    x, want = shared(("edge", ne0, ne1, eps), make)
    N.assert_same_words_nan_for_nan(run(gpu, x, x.shape[1] // 2, eps), want, "edge groups")


def test_an_empty_tensor_is_no_launch(gpu):
    t = gpu.Tensor(gpu.F32, [8, 2, 0, 1])
    assert gpu.ops.group_norm(t, 2, EPS).ne == [8, 2, 0, 1]
    t = gpu.Tensor(gpu.F32, [0, 2, 4, 1])
    assert gpu.ops.group_norm(t, 2, EPS).ne == [0, 2, 4, 1]


def _declined(gpu, src, dst, n_groups, rc, word, keeps):
    with pytest.raises(gpu.lib.CllmError) as e:
        gpu.ops.group_norm(src, n_groups, EPS, dst=dst)
    assert e.value.rc == rc and word in str(e.value), str(e.value)
    assert np.array_equal(keeps[0].numpy(), keeps[1])


def test_a_non_dense_source_or_destination_is_declined(gpu):
    """nb[0] = 8: CLLM_E_UNSUPPORTED with a message, and the destination keeps what it held"""
    n = 32
    before = np.arange(2 * n, dtype=np.float32)
    wide = gpu.Tensor.from_numpy(before)
    every_other = wide.view([8, 2, 2], [8, 64, 128])
    dense = gpu.Tensor.from_numpy(np.full((2, 2, 8), 7.0, np.float32))
    _declined(gpu, every_other, dense, 2, CLLM_E_UNSUPPORTED, "dense", (dense, np.full((2, 2, 8), 7.0, np.float32)))
    _declined(gpu, dense, every_other, 2, CLLM_E_UNSUPPORTED, "dense", (wide, before))


def test_an_f16_tensor_is_declined(gpu):
    h = gpu.Tensor.from_numpy(np.ones((2, 2, 8), np.float16))
    f = gpu.Tensor.from_numpy(np.full((2, 2, 8), 7.0, np.float32))
    _declined(gpu, h, f, 2, CLLM_E_UNSUPPORTED, "type", (f, np.full((2, 2, 8), 7.0, np.float32)))
    _declined(gpu, f, h, 2, CLLM_E_UNSUPPORTED, "type", (h, np.ones((2, 2, 8), np.float16)))


def test_a_shape_mismatch_is_declined(gpu):
    a = gpu.Tensor.from_numpy(np.ones((4, 2, 16), np.float32))
    d = gpu.Tensor.from_numpy(np.full((4, 2, 8), 7.0, np.float32))
    _declined(gpu, a, d, 2, CLLM_E_INVALID, "shape", (d, np.full((4, 2, 8), 7.0, np.float32)))


@pytest.mark.parametrize("n_groups", [0, -3])
def test_no_groups_is_declined(gpu, n_groups):
    a = gpu.Tensor.from_numpy(np.ones((4, 2, 8), np.float32))
    d = gpu.Tensor.from_numpy(np.full((4, 2, 8), 7.0, np.float32))
    _declined(gpu, a, d, n_groups, CLLM_E_INVALID, "n_groups", (d, np.full((4, 2, 8), 7.0, np.float32)))


def test_a_null_tensor_is_declined(gpu):
    a = gpu.Tensor.from_numpy(np.ones((4, 2, 8), np.float32))
    L = gpu.lib.get()
    ca = a.c()
    assert L.cllm_op_group_norm(None, None, C.byref(ca), 2, EPS) == CLLM_E_INVALID
    assert L.cllm_op_group_norm(None, C.byref(ca), None, 2, EPS) == CLLM_E_INVALID
    assert b"null" in L.cllm_last_error()
    assert np.array_equal(a.numpy(), np.ones((4, 2, 8), np.float32))


def test_more_than_2_31_channel_batch_pairs_is_declined(gpu):
    """ne[2] * ne[3] = 2^31, described over a small buffer with strides of 0 (nothing is launched, nothing is read)"""
    buf = gpu.Tensor.from_numpy(np.full(8, 7.0, np.float32))
    big = buf.view([8, 1, 1 << 16, 1 << 15], [4, 32, 0, 0])
    _declined(gpu, big, big, 2, CLLM_E_UNSUPPORTED, "2^31", (buf, np.full(8, 7.0, np.float32)))


def test_group_norm_node_sequence(gpu):
    """GROUP_NORM, MUL and ADD by a [1, 1, C] view of weight and bias as three launches -- what the module dispatches for the host's GroupNorm -- against the
    reference's three nodes, at the image decoder's channel count with a small image"""
    rng = np.random.default_rng(512)
    x = (rng.standard_normal((1, 512, 6, 6)) * 2.0 + 0.1).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(512)).astype(np.float32)
    b = (0.1 * rng.standard_normal(512)).astype(np.float32)
    T, ops = gpu.Tensor, gpu.ops
    wv, bv = T.from_numpy(w).view([1, 1, 512], [4, 4, 4]), T.from_numpy(b).view([1, 1, 512], [4, 4, 4])
    got = ops.add(ops.mul(ops.group_norm(T.from_numpy(x), 32, EPS), wv), bv).numpy().reshape(x.shape)
    N.assert_same_words(got, G.group_norm_affine(x, 32, EPS, w, b), "GROUP_NORM -> MUL -> ADD")
