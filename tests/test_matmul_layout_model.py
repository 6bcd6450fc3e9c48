"""CPU: the cases of tests/matmul_layout_cases.py mean what they say, before tests/test_gpu_matmul_layouts.py holds the kernels against them.

  a) the oracle over the strided views == the oracle over the dense copies, word for word, and it leaves every byte of dst padding alone;
  b) the oracle == the reference's own CPU backend on the same views, word for word (where oracle/_ref is built);
  c) every case BITES: computing with one altered stride or offset replaced by its dense value gives another result, for every alteration of the layout
     (matmul_layout_cases.alterations) whose replaced view stays inside the buffer, and for at least one per case -- so a kernel that took row_size(K) for nb01,
     N for the dst stride or a dense slice index for nb12 would fail the GPU test of that case;
  d) the case list reaches every route of cllm_op_mul_mat (matmul_layout_cases.route_of, from the thresholds the library reports), and on every strided route
     there is a case that bites on the weight's row stride and one that bites on the dst stride."""
import numpy as np
import pytest

import matmul_layout_cases as L
import oracle as O
import ref_ggml as R

FAMILY_CASES = {"tuned": L.TUNED_CASES, "kq": L.KQ_CASES, "float": L.FLOAT_CASES}


def words(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def bites(c, b, exp, alt):
    """does the oracle with the alteration `alt` undone give another dst buffer?  None: the replaced view would leave its buffer"""
    _, op, field, value = alt
    v = L.altered_view({"w": c.wv, "x": c.xv, "d": c.dv}[op], field, value)
    t, size = (c.t, b.w_raw.size) if op == "w" else (L.F32, b.x_raw.size if op == "x" else b.d_raw.size)
    if L.extent(t, v) > size:
        return None
    got = L.oracle_over_views(O, c, b, **{op + "v": v})
    return not np.array_equal(got, exp)


@pytest.mark.parametrize("family", list(FAMILY_CASES))
def test_views_equal_dense_copies_and_every_layout_bites(family):
    """a) and c)"""
    for c in FAMILY_CASES[family]:
        b = L.build(c)
        want, exp = L.expected(O, c)
        assert not np.isnan(want).any() and np.all(np.abs(want) < 1e30), (c.name, "the expected product holds poison")
        got = L.oracle_over_views(O, c, b)
        assert np.array_equal(words(got), words(exp)), c.name
        alts = L.alterations(c)
        assert bool(alts) == (c.layout != "dense"), c.name
        res = [(a[0], bites(c, b, exp, a)) for a in alts]
        assert all(r is not False for _, r in res), (c.name, res)
        assert not alts or any(r for _, r in res), (c.name, res)


def reference_weight(c, b):
    """-> (raw weight buffer, view) for the reference.  Its mat-mul hands tinyBLAS the row stride as nb01 / type_size, in whole blocks (ggml-cpu.c, the
    llamafile_sgemm calls of ggml_compute_forward_mul_mat), so it cannot address rows a fraction of a block apart: with 16 bytes between Q4_0 rows it reads every
    row but the first from the wrong place.  Such a view (the C ABI takes it, byte strides and all; a ggml graph never builds one) goes to the reference with each
    stride rounded up to whole blocks: the same rows, the same poison between them, the same product"""
    ts = L.TYPE_SIZE[c.t]
    if all(n % ts == 0 for n in c.wv.nb[1:]):
        return b.w_raw, c.wv
    nb1 = L._up(c.wv.nb[1], ts)
    nb2 = L._up(max(c.wv.nb[2], nb1 * c.N), ts)
    nb3 = L._up(max(c.wv.nb[3], nb2 * c.ne02), ts)
    v = L.View(c.wv.ne, [ts, nb1, nb2, nb3], c.wv.offset)
    raw = np.full(L.extent(c.t, v) + 16, L.POISON, np.uint8)
    L.scatter(raw, c.t, v, b.w_dense)
    return raw, v


@pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built (needs the reference sources)")
@pytest.mark.parametrize("family", list(FAMILY_CASES))
def test_oracle_equals_the_reference_backend_on_the_same_views(family):
    """b)  (rows a fraction of a block apart: reference_weight)"""
    whole = 0
    for c in FAMILY_CASES[family]:
        b = L.build(c)
        want, _ = L.expected(O, c)
        w_raw, wv = reference_weight(c, b)
        whole += wv is c.wv
        got = R.mul_mat(w_raw, R.View(c.t, wv.ne, wv.nb, wv.offset), b.x_raw, R.View(R.GGML_TYPE_F32, c.xv.ne, c.xv.nb, c.xv.offset))
        assert np.array_equal(words(got), words(want)), (c.name, int(np.sum(words(got) != words(want))))
    assert 2 * whole > len(FAMILY_CASES[family])


def test_poison_and_sentinel():
    """0x7f bytes are what the module says they are, and a weight buffer is poison wherever its view is not"""
    assert np.full(4, L.POISON, np.uint8).view(np.float32)[0] > 3.3e38
    assert np.isnan(np.full(2, L.POISON, np.uint8).view(np.float16)[0])
    c = next(c for c in L.TUNED_CASES if c.layout == "combined" and c.M == 12)
    b = L.build(c)
    for raw, t, v in ((b.w_raw, c.t, c.wv), (b.x_raw, L.F32, c.xv)):
        m = L.view_mask(raw.size, t, v)
        assert np.all(raw[~m] == L.POISON) and (~m).sum() > 0
    assert np.all(b.d_raw == L.SENTINEL)


def test_the_cases_reach_every_route_and_bite_there():
    """d)  The mutation this predicts: mm_tile_args_of (csrc/mm_tile.h) or launch_gemv_kq (csrc/gemv_kq.hip) taking the dense row size for nb01 fails the GPU test
    of every case listed under w.nb[1] for mmx / mmq / gemv_kq"""
    th = L.thresholds()
    reached = {}
    for c in L.CASES:
        modes = [dict()] + ([dict(prefill=0), dict(prefill=0, f16=True)] if c.family == "tuned" else [dict(attn=0)] if c.t == L.F16 else [])
        for m in modes:
            reached.setdefault(L.route_of(c, th, **m), []).append(c)
    assert set(reached) >= set(L.ROUTES), sorted(set(L.ROUTES) - set(reached))
    strided = ("decode_two_launches", "mmvq", "mmx", "mmq", "dense_f16", "gemv_kq_nc1", "gemv_kq_nc8", "gemv_kq_nc8+ragged", "f_vd", "f_t8", "mmf_exact_t8",
               "mmf_exact_vd", "mma_f16")
    for route in strided:
        for label in ("w.nb[1]", "d.nb[1]") if route not in ("decode_two_launches", "gemv_kq_nc1") else ("w.nb[1]",):
            hit = None
            for c in reached[route]:
                alt = [a for a in L.alterations(c) if a[0] == label]
                if alt and len(L.alterations(c)) == 1:                      # the stride alone: nothing else would fail the case
                    b = L.build(c)
                    if bites(c, b, L.expected(O, c)[1], alt[0]):
                        hit = c
                        break
            assert hit is not None, (route, label)
            print(f"BITES {route} {label}: {hit.name}")
    # one-column products have no dst stride to get wrong; their dst is still checked through an offset
    assert any(a[0] == "d.offset" for c in reached["decode_one_launch"] for a in L.alterations(c))


def test_the_shapes_the_issue_names_are_there():
    names = {c.name for c in L.CASES}
    for n in ("q4_k-K512-N130-M70-w_row_pad", "q4_0-K96-N7-M1-w_col_slice", "q8_0-K512-N20-M12-b2x2.2x4-w_3d_r3", "q4_1-K512-N20-M40-b1x1.3x1-x_permuted",
              "iq2_xxs-K512-N20-M9-combined", "mxfp4-K96-N20-M5-offset", "f16-K203-N17-M40-x_row_pad", "f32-K128-N20-M3-w_row_pad", "f16-K128-N264-M40-b2x1.4x1-kq_like",
              "f16-K264-N128-M40-b2x1.4x1-vp_like"):
        assert n in names, n
    assert not any(c.M == 1 and c.layout in ("x_row_pad", "d_row_pad") for c in L.CASES)          # nothing observable: not generated
