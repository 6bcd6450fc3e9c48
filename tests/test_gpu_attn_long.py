"""GPU: single-token attention past the long-context threshold (CLLM_ATTN_LONG), every form, through cllm_op_rope_kv_attn_decode.

  flash  (CLLM_ATTN_LONG_FLASH=1): k_rope_kv_prep + the split-KV flash kernel with the position count read on the device + the merge, with whole splits past the
         live positions -- every element against float64 with fattn_model's bound under attn_long_model.long_flash_plan (tests/test_attn_long_model.py shows
         that the right algorithm passes it and that a kernel which ignores n_kv_dev, or merges an empty partial with weight 1, does not);
  three launches (ML % 32 != 0, or CLLM_ATTN_LONG_3=1), the fused two launches, a threshold of 64 (CLLM_ATTN_LONG=64), every k_attn_long_scores<HD, MODE, R2>:
         bit-identical to the node sequence;
  rows whose soft-max total sits next to a float rounding boundary (attn_long_model.attn_boundary_case): the serial fallback of k_attn_dec, of the general
         kernel k_attn_decode (called without a RoPE table) and of both attn_long.hip kernels, bit-identical to the node sequence AND to the CPU oracle's node
         sequence (the node sequence's own SOFT_MAX takes its fallback on the same rows: two wrong fallbacks must not be able to agree with each other).

The three switches are read once per process: each setting runs tests/attn_long_worker.py in a fresh child under its own time limit, started once per module; a
child that ends badly fails its fixture, every test that needs it errors, and nothing further is started on the GPU.  The default environment runs in-process.

Every case holds fp16 NaN in the V cache and values of exponent 2^14 in the K cache past n_kv (and checks both caches word for word against the node
sequence).  The node sequence views n_kv positions only, so the reference never sees the poison; a kernel that reads past n_kv does."""
import os
import subprocess
import sys

import numpy as np
import pytest

import attn_long_model as AL
import attn_long_worker as W
from conftest import ROOT

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 120                      # seconds per child: a few dozen launches on tensors of a few MB (the flash list: 152 cases), plus the start of the process
_failed = []                             # a child, or the in-process run, ended badly: nothing else is started


def _child(name, env, tmp_path_factory):
    if _failed:
        pytest.fail(f"not started: the run for {_failed[0]} ended badly")
    out = str(tmp_path_factory.mktemp("attn_long") / f"{name}.npz")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_long_worker.py"), name, out], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _failed.append(name)
        raise
    if r.returncode != 0:
        _failed.append(name)
        pytest.fail(f"worker {name} {env}: exit status {r.returncode}\n{(r.stdout + r.stderr)[-1500:]}")
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def res_flash(gpu, tmp_path_factory):
    return _child("flash", {"CLLM_ATTN_LONG_FLASH": "1"}, tmp_path_factory)


@pytest.fixture(scope="module")
def res_three(gpu, tmp_path_factory):
    return _child("three", {"CLLM_ATTN_LONG_3": "1"}, tmp_path_factory)


@pytest.fixture(scope="module")
def res_thr64(gpu, tmp_path_factory):
    return _child("thr64", {"CLLM_ATTN_LONG": "64"}, tmp_path_factory)


@pytest.fixture(scope="module")
def res_default(gpu):
    if _failed:
        pytest.fail(f"not started: the run for {_failed[0]} ended badly")
    try:
        return W.run_cases(gpu, AL.CASE_LISTS["default"])
    except BaseException:
        _failed.append("default (in-process)")
        raise


def caches_equal_the_node_sequence(res, case):
    """both caches, word for word (as differences from the case's initial caches), and exactly the new token's row / column was written"""
    kind, hd, nh, nkv, mode, ML, n_kv, extra = case
    key, KD, pos = AL.case_key(case), hd * nkv, n_kv - 1
    for c in ("k", "v"):
        assert np.array_equal(res[f"{key}.g{c}_i"], res[f"{key}.w{c}_i"]) and np.array_equal(res[f"{key}.g{c}_v"], res[f"{key}.w{c}_v"]), c
    assert set(res[key + ".gk_i"]) <= set(range(pos * KD, pos * KD + KD)) and set(res[key + ".gv_i"]) <= set(range(pos, KD * ML, ML))


def bit_identical(res, case):
    key = AL.case_key(case)
    got, want = res[key + ".got"], res[key + ".want"]
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (int(np.sum(got.view(np.uint32) != want.view(np.uint32))), float(np.max(np.abs(got - want))))
    caches_equal_the_node_sequence(res, case)


# ---- the split-KV flash form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AL.FLASH_CASES, ids=AL.flash_id)
def test_flash_decode_is_inside_the_bound_at_every_element(res_flash, case):
    """|got - R| <= bound at every element (R, bound: fattn_model.reference over the rotated fp16 operands under the long plan); finite although V is NaN and K
    huge past n_kv; caches as the node sequence leaves them.  The largest |got - R| / bound is printed.
    That the flash form RAN: cllm_op_rope_kv_attn_decode falls through to the bit-exact forms when launch_attn_long_flash declines (switch not latched, scratch
    misaligned, max_splits < 4), and those pass this bound too.  They equal the node sequence word for word; the flash form adds in another order (MFMA tiles, fp16
    P, a merge), so over nh * hd words it cannot: the result must differ from the node sequence somewhere.
    Where the global maximum sits: `ascending` puts it in the last live split for every head; `split_maxima` at key n_kv - 1 for odd kv heads and at key 0 for
    even ones, so the nkv = 1 shape has it in the last live split under `ascending` only."""
    hd, nh, nkv, mode, ML, n_kv, prof = case
    ref = AL.flash_case_data(case)["ref"]
    got = res_flash[AL.case_key(("flash",) + case) + ".got"].reshape(ref["R"].shape)
    err = np.abs(got.astype(np.float64) - ref["R"])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(ref["bound"] > 0, err / ref["bound"], np.where(err == 0, 0.0, np.inf))
    print(f"\n|got - R| / bound: {np.nanmax(ratio):.3f} {AL.flash_id(case)}")
    assert np.all(np.isfinite(got))
    assert np.all(err <= ref["bound"]), (float(np.nanmax(ratio)), int(np.sum(~(err <= ref["bound"]))), np.argwhere(~(err <= ref["bound"]))[:4].tolist())
    caches_equal_the_node_sequence(res_flash, ("flash",) + case)
    want = res_flash[AL.case_key(("flash",) + case) + ".want"]
    differ = int(np.sum(got.reshape(-1).view(np.uint32) != want.view(np.uint32)))
    print(f"words that differ from the node sequence: {differ} of {want.size}")
    assert differ >= 1


@pytest.mark.parametrize("case", AL.CASE_LISTS["flash"][len(AL.FLASH_CASES):], ids=AL.case_key)
def test_flash_declined_falls_through_to_the_one_launch_kernel(res_flash, case):
    """one byte of scratch less than cllm_attn_decode_wsize asks for: the dispatcher skips both long forms; 64 query heads per kv head: both long forms decline
    (r2 > 32, r2 not in 1 / 2 / 4 / 8).  Either way k_attn_dec runs at n_kv 600: bit-identical to the node sequence"""
    bit_identical(res_flash, case)


# ---- the exact forms: bit-identical to the node sequence ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in AL.CASE_LISTS["default"] if c[0] == "random"], ids=AL.case_key)
def test_long_exact_forms_equal_the_node_sequence(res_default, case):
    bit_identical(res_default, case)


@pytest.mark.parametrize("case", AL.CASE_LISTS["three"], ids=AL.case_key)
def test_three_launches_forced_equal_the_node_sequence_and_the_fused_form(res_three, res_default, case):
    bit_identical(res_three, case)
    key = AL.case_key(case)
    assert np.array_equal(res_three[key + ".got"].view(np.uint32), res_default[key + ".got"].view(np.uint32))


@pytest.mark.parametrize("case", AL.CASE_LISTS["thr64"], ids=AL.case_key)
def test_threshold_64_equals_the_node_sequence(res_thr64, case):
    bit_identical(res_thr64, case)


# ---- the soft-max's serial fallback inside the attention kernels --------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in AL.CASE_LISTS["default"] if c[0] in ("boundary", "boundary_nt")], ids=AL.case_key)
def test_soft_max_fallback_inside_attention(res_default, case):
    """with a RoPE table -- n_kv 300 and 500: k_attn_dec (one soft-max site, decode_fused.hip); 777 at ML 1024: k_attn_long_softmax_pv; 777 at ML 1032:
    k_attn_long_softmax.  boundary_nt, the same inputs at n_kv 300 and 500 without a table (rope_cs = NULL): the general kernel k_attn_decode and its own site"""
    kind, hd, nh, nkv, mode, ML, n_kv, extra = case
    d = AL.boundary_attn_case((hd, nh, nkv, ML, n_kv - 1, mode))
    assert len(d["hits"]) >= 1
    bit_identical(res_default, case)
    key, orc = AL.case_key(case), d["oracle"]
    p, got = res_default[key + ".p"], res_default[key + ".got"]
    bad = [h for h in range(nh) if not np.array_equal(p[h].view(np.uint32), orc["p"][h].view(np.uint32))]
    assert not bad, (bad, d["hits"])
    assert np.array_equal(got.view(np.uint32), orc["out"].view(np.uint32)), int(np.sum(got.view(np.uint32) != orc["out"].view(np.uint32)))
