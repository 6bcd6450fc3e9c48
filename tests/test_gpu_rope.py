"""cllm_op_rope against the reference's own CPU backend (ggml_rope_ext / ggml_rope_ext_inplace over ggml_view_4d, tests/ref_ggml.py): strided views
of the fused [q | k | v] buffer, padded heads, ne[3] == 2, n_dims below ne0, more pairs than threads, positions at and beyond every range of the
cos / sin argument reduction, negative positions, every parameter, the three zones of the YaRN ramp -- and the device's cos / sin swept
through the op itself at half a million angles.  All inputs are finite: every word must be equal, in the result and, in place, in the whole
parent buffer.  tests/test_elementwise_model.py holds the same cases for the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import elementwise_cases as E
import ref_ggml as R
import rope_cases as RC

pytestmark = pytest.mark.gpu

CLLM_E_INVALID, CLLM_E_UNSUPPORTED = -1, -2
CASES = RC.layout_cases() + RC.n_dims_cases() + RC.parameter_cases()
_ref_cache = {}


def reference(case, inplace):
    """(result, parent after) of the reference, computed once per case"""
    if (case.name, inplace) not in _ref_cache:
        _ref_cache[(case.name, inplace)] = R.rope(case.parent, case.ne, case.nb, case.offset, case.pos, case.ff, case.params, inplace)
    return _ref_cache[(case.name, inplace)]


def device_rope(gpu, case, inplace):
    """(result, parent after) of cllm_op_rope over the same view of the same parent"""
    parent = gpu.Tensor.from_numpy(case.parent)
    view = parent.view(case.ne, case.nb, case.offset)
    kw = {k: v for k, v in case.params.items() if k not in ("n_dims", "mode")}
    out = gpu.ops.rope_ext(view, gpu.Tensor.from_numpy(case.pos), gpu.Tensor.from_numpy(case.ff) if case.ff is not None else None,
                           case.params["n_dims"], case.params["mode"], inplace=inplace, **kw)
    after = parent.numpy().reshape(case.parent.shape)
    if inplace:
        assert out is view
        result = np.lib.stride_tricks.as_strided(after.reshape(-1)[case.offset // 4:], tuple(reversed(case.ne)), tuple(reversed(case.nb))).copy()
    else:
        result = out.numpy()
    return result, after


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_rope_has_the_bits_of_the_reference(gpu, case, inplace):
    want, want_parent = reference(case, inplace)
    got, got_parent = device_rope(gpu, case, inplace)
    E.assert_same_words(got, want, None, f"rope {case}")
    # in place: the v slice, the padding, the pass-through channels and everything else keep their bytes; out of place: the source is only read
    E.assert_same_words(got_parent, want_parent, None, f"rope {case}: the parent buffer")
    if inplace and case.params["n_dims"] < case.ne[0]:
        changed = got_parent.reshape(-1).view(np.uint32) != case.parent.reshape(-1).view(np.uint32)
        assert 0 < changed.sum() <= case.ne[1] * case.ne[2] * case.ne[3] * case.params["n_dims"]


def test_the_yarn_cases_have_pairs_below_on_and_above_the_ramp():
    for case in CASES:
        if case.params.get("ext_factor", 0.0) == 0.0:
            continue
        p = case.params
        corr0, corr1 = RC.yarn_corr_dims(p["n_dims"], p["n_ctx_orig"], p["freq_base"], p["beta_fast"], p["beta_slow"])
        y = (np.arange(p["n_dims"] // 2, dtype=np.float32) - corr0) / max(np.float32(0.001), corr1 - corr0)
        assert (y <= 0).sum() > 4 and ((y > 0) & (y < 1)).sum() > 4 and (y >= 1).sum() > 4, (case, corr0, corr1)


@pytest.mark.parametrize("case", RC.sweep_cases(), ids=repr)
def test_cos_sin_of_the_device_swept_through_the_op(gpu, case):
    """hd == n_dims == 2, x == (1, 0), freq_scale == 2^-k: token t of the result is (cos, sin) of pos[t] * 2^-k, the device's gm_cosf / gm_sinf on
    one side and the host's libm inside the reference's rope on the other; 65 536 angles per launch"""
    want, _ = reference(case, False)
    got, _ = device_rope(gpu, case, False)
    angles = RC.sweep_angles(case)
    bad = np.flatnonzero((got.reshape(-1, 2).view(np.uint32) != want.reshape(-1, 2).view(np.uint32)).any(axis=1))
    print(f"{case}: {bad.size} of {angles.size} angles differ")
    assert bad.size == 0, f"{bad.size} angles differ; (angle, device cos sin, reference cos sin): " + str(
        [(float(angles[i]).hex(), got.reshape(-1, 2)[i].tolist(), want.reshape(-1, 2)[i].tolist()) for i in bad[:6]])


TABLE_POSITIONS = [0, 1, 4095, 131071]


@pytest.mark.parametrize("mode", [0, 2], ids=["normal", "neox"])
@pytest.mark.parametrize("head_dim", [2, 64, 128, 192])
def test_rope_table_has_the_words_of_rope(gpu, head_dim, mode):
    """cllm_op_rope_table against cllm_op_rope, word for word: both take the plain table entry (rope_theta, rope_entry, common.h) and must not drift apart.
    Rows whose pairs are (1, 0), n_dims == head_dim, no frequency factors, freq_scale 1, ext_factor 0, attn_factor 1: rope_rot_a / rope_rot_b return exactly
    (cos, sin), so token t of the rotated tensor is the table of position TABLE_POSITIONS[t] -- interleaved as the table is in mode 0, cos | sin halves in mode 2.
    What each case reaches: head_dim 2 -- pair 0 alone, the recurrence of zero multiplications; 64 -- 32 pairs, half of the table kernel's 64 threads idle;
    128 -- one full trip of the 64-thread fill; 192 -- 96 pairs, the fill's second trip (threads 0..31 only) and recurrences of up to 95 multiplications;
    mode 0 / 2 -- both arms of rope_pair in k_rope; position 0 -- theta == 0 for every pair (cos 1, sin +0); 1 -- angles of at most 1; 4095 and 131071 -- large angles
    (pair 0: theta == pos) shrinking through every quadrant down the table, so the recurrence's rounding shows in cos and sin."""
    half = head_dim // 2
    x = np.zeros((len(TABLE_POSITIONS), 1, head_dim), np.float32)
    x[..., (slice(0, None, 2) if mode == 0 else slice(0, half))] = 1.0
    pos = np.array(TABLE_POSITIONS, np.int32)
    rot = gpu.ops.rope_ext(gpu.Tensor.from_numpy(x), gpu.Tensor.from_numpy(pos), None, head_dim, mode, freq_base=10000.0).numpy().reshape(len(TABLE_POSITIONS), head_dim)
    for t, p in enumerate(TABLE_POSITIONS):
        cs = gpu.Tensor.from_numpy(np.full(head_dim, 7.0, np.float32))
        gpu.lib.check(gpu.lib.get().cllm_op_rope_table(None, gpu.Tensor.from_numpy(pos[t:t + 1]).data_ptr(), head_dim, 10000.0, cs.data_ptr()), "rope_table")
        table = cs.numpy().reshape(half, 2)
        want = rot[t].reshape(half, 2) if mode == 0 else np.stack([rot[t, :half], rot[t, half:]], axis=1)
        E.assert_same_words(table, np.ascontiguousarray(want), None, f"rope_table head_dim {head_dim} mode {mode} position {p}")
        if p == 0:
            assert np.array_equal(table.view(np.uint32), np.tile(np.array([1.0, 0.0], np.float32).view(np.uint32), (half, 1)))


# ---- what is declined ----------------------------------------------------------------------------------------------------------------------
def declined(gpu, rc, word, ne=(64, 2, 5), nb=None, pos_len=5, **kw):
    x = np.arange(2 * 5 * 2 * 64, dtype=np.float32)
    src = gpu.Tensor.from_numpy(x).view(list(ne), nb or [4, 4 * ne[0], 4 * ne[0] * ne[1]])
    dst = gpu.Tensor.from_numpy(np.full(x.shape, 7.0, np.float32))
    p = gpu.lib.RopeParams(kw.get("n_dims", 64), kw.get("mode", 2), 0, 10000.0, 1.0, 0.0, 1.0, 0.0, 0.0)
    pos = gpu.Tensor.from_numpy(np.arange(pos_len, dtype=np.int32))
    cs, cp, cd = src.c(), pos.c(), dst.view(list(ne), kw.get("dst_nb") or [4, 4 * ne[0], 4 * ne[0] * ne[1]]).c()
    r = gpu.lib.get().cllm_op_rope(None, C.byref(cs), C.byref(cp), None, C.byref(cd), C.byref(p))
    msg = gpu.lib.get().cllm_last_error().decode()
    assert r == rc and word in msg, (r, msg)
    assert np.array_equal(dst.numpy(), np.full(x.shape, 7.0, np.float32))
    assert np.array_equal(src.raw().view(np.float32)[:x.size], x)


def test_what_rope_declines(gpu):
    declined(gpu, CLLM_E_UNSUPPORTED, "mode 4", mode=4)
    declined(gpu, CLLM_E_INVALID, "n_dims", n_dims=63)                       # odd
    declined(gpu, CLLM_E_INVALID, "n_dims", n_dims=66)                       # n_dims > ne0
    declined(gpu, CLLM_E_INVALID, "pos", pos_len=4)                          # a position tensor shorter than ne[2]
    declined(gpu, CLLM_E_INVALID, "shape", nb=[8, 512, 1024])                # nb[0] != 4 in the source ...
    declined(gpu, CLLM_E_INVALID, "shape", dst_nb=[8, 512, 1024])            # ... and in the destination
