"""CPU-only: what the GPU tests of PAD, PAD_REFLECT_1D, UPSCALE and CONV_TRANSPOSE_1D stand on.  The header declares the four entries and the library exports them; the
numpy restatements of tests/ref_resample.py equal the reference's own CPU backend, word for word, on every case list the GPU files use (so every reference graph of
those lists has run here without a ggml assert); of the twelve ways gcc may contract the bilinear expression exactly one matches the reference on the bilinear list, and
the un-contracted form does not; CONV_TRANSPOSE_1D with the taps added in descending order, or with a plain sequential dot product, differs from the reference on its
list -- without which those lists would prove nothing about the orders."""
import os
import subprocess

import numpy as np
import pytest

import ref_ggml as R
import ref_norm as N
import ref_resample as RR
from test_abi import header_symbols

NEW = ("cllm_op_pad", "cllm_op_pad_reflect_1d", "cllm_op_upscale", "cllm_op_conv_transpose_1d")
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built")


def test_the_header_declares_and_the_library_exports_the_four_entries(pkg):
    syms = header_symbols()
    for s in NEW:
        assert s in syms, s
        assert s in pkg.lib.SIGNATURES, s
    out = subprocess.check_output(["nm", "-D", "--defined-only", pkg.lib.SO_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [s for s in NEW if s not in exported]
    txt = open(os.path.join(os.path.dirname(pkg.lib.SO_PATH), "..", "include", "chatllm_hip.h")).read()
    for cite in ("ggml_compute_forward_pad_f32", "ggml_compute_forward_pad_reflect_1d", "ggml_compute_forward_upscale_f32", "ggml_compute_forward_conv_transpose_1d_f16_f32"):
        assert cite in txt, cite
    for name in ("pad", "pad_reflect_1d", "upscale", "conv_transpose_1d"):
        assert callable(getattr(pkg.ops, name)), name


# ---- PAD / PAD_REFLECT_1D -------------------------------------------------------------------------------------------------------------------
PAD_SOURCES = RR.pad_sources()


@needs_ref
@pytest.mark.parametrize("i", range(len(PAD_SOURCES)), ids=[s[0] for s in PAD_SOURCES])
def test_pad_restated(i):
    name, raw, view, p = PAD_SOURCES[i]
    N.assert_same_words(RR.pad_np(RR.gather(raw, view), p), RR.pad(raw, view, p), name)


def test_the_pad_inputs_carry_the_edge_values():
    x = np.concatenate([RR.gather(raw, view).reshape(-1) for _, raw, view, _ in PAD_SOURCES])
    w = x.view(np.uint32)
    assert np.any(w == 0x80000000) and np.any(np.isinf(x)) and np.any((w & 0x7f800000 == 0) & (w & 0x007fffff != 0))
    assert len({int(v) for v in w[np.isnan(x)]}) >= 6        # NaNs of several payloads


@needs_ref
@pytest.mark.parametrize("case", RR.REFLECT)
def test_pad_reflect_1d_restated(case):
    x = RR.reflect_input(case)
    N.assert_same_words(RR.pad_reflect_1d_np(x, case[1], case[2]), RR.pad_reflect_1d(x, case[1], case[2]), str(case))


# ---- UPSCALE ----------------------------------------------------------------------------------------------------------------------------------
UP_SOURCES = RR.upscale_sources()


@needs_ref
@pytest.mark.parametrize("mode", [RR.NEAREST, RR.BILINEAR])
@pytest.mark.parametrize("i", range(len(UP_SOURCES)), ids=[s[0] for s in UP_SOURCES])
def test_upscale_restated(i, mode):
    name, raw, view, ne = UP_SOURCES[i]
    N.assert_same_words(RR.upscale_np(RR.gather(raw, view), ne, mode), RR.upscale(raw, view, ne, mode), name)


@needs_ref
def test_exactly_one_contraction_pattern_of_the_bilinear_expression_matches_the_reference():
    """differing words per candidate, summed over the bilinear case list: 0 for one pattern alone, and not for the un-contracted form"""
    miss = dict.fromkeys(RR.bilinear_patterns(), 0)
    for name, raw, view, ne in UP_SOURCES:
        want = RR.upscale(raw, view, ne, RR.BILINEAR)
        x = RR.gather(raw, view)
        for pat in miss:
            miss[pat] += N.differing_words(RR.upscale_np(x, ne, RR.BILINEAR, pat), want)
    assert [p for p, n in miss.items() if n == 0] == [RR.BILINEAR_PATTERN], miss
    assert miss["plain/plain/plain"] > 0, miss


# ---- CONV_TRANSPOSE_1D ------------------------------------------------------------------------------------------------------------------------
def _ct_ref(k, x, s0, layout="dense"):
    (kr, kv), (xr, xv) = RR.conv_t_views(k, x, layout)
    return RR.conv_transpose_1d(kr, kv, xr, xv, s0)


@needs_ref
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("case", RR.CONV_T)
def test_conv_transpose_1d_restated(case, f16):
    k, x = RR.conv_t_operands(case, f16)
    N.assert_same_words(RR.conv_transpose_1d_np(k, x, case[4]), _ct_ref(k, x, case[4]), str(case))


@needs_ref
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("layout", ["padded data", "padded kernel"])
def test_conv_transpose_1d_reads_the_strides_as_given(layout, f16):
    case = (5, 2, 70, 4, 2)
    k, x = RR.conv_t_operands(case, f16, 1)
    N.assert_same_words(RR.conv_transpose_1d_np(k, x, case[4]), _ct_ref(k, x, case[4], layout), layout)


@needs_ref
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_the_wrong_orders_differ_from_the_reference_on_the_case_list(f16):
    desc = seq = 0
    for case in RR.CONV_T:
        k, x = RR.conv_t_operands(case, f16)
        want = _ct_ref(k, x, case[4])
        desc += N.differing_words(RR.conv_transpose_1d_np(k, x, case[4], descending=True), want)
        seq += N.differing_words(RR.conv_transpose_1d_np(k, x, case[4], sequential=True), want)
    assert desc > 0 and seq > 0, (desc, seq)


@needs_ref
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_products_of_minus_zero_and_untouched_outputs_give_plus_zero(f16):
    """every product is -0.0: every output is +0.0f, where taps reach it and where none does (s0 > K)"""
    k = np.full((8, 3, 2), 1.5, np.float32)
    k = k.astype(np.float16).view(np.uint16) if f16 else k
    x = np.full((8, 5), -0.0, np.float32)
    want = _ct_ref(k, x, 4)
    assert np.all(want.view(np.uint32) == 0)
    N.assert_same_words(RR.conv_transpose_1d_np(k, x, 4), want)


@needs_ref
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_data_beyond_the_fp16_range(f16):
    """1e5 rounds to the fp16 infinity under an F16 kernel (inf - inf: NaN for NaN) and stays finite under an F32 kernel"""
    case = (4, 3, 40, 6, 2)
    k, x = RR.conv_t_operands(case, f16, 2)
    x = x.copy()
    x[::3, ::2] = np.float32(1e5)
    x[1, 1] = np.float32(-7e4)
    want = _ct_ref(k, x, case[4])
    assert np.any(np.isnan(want)) == f16
    N.assert_same_words_nan_for_nan(RR.conv_transpose_1d_np(k, x, case[4]), want)
