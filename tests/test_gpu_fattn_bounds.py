"""GPU: flash attention (fattn.hip: k_fattn, k_fattn_merge) element by element against float64, on score profiles that drive the lazy rescale, p > 1,
fp16-subnormal p, merge weights far from 1 and the masking edges.

tests/test_gpu_fattn.py judges the kernel by max |got - want| / max |want| on Gaussian q and k, where m_run moves once per row and every split has about the
same maximum.  Here every element of every case satisfies |got - R| <= bound, with R and the bound from tests/fattn_model.py (derived from the kernel's
roundings; tests/test_fattn_model.py shows that the right algorithm passes it, that mutants do not, and that the inputs reach the paths they name).  Through
the C ABI, as tests/test_gpu_fattn.py does.  The largest |got - R| / bound of each case is printed before the assertion."""
import numpy as np
import pytest

import fattn_model as FM
from conftest import prefill_mode

pytestmark = pytest.mark.gpu


def run_flash_attn_ext(gpu, case, d):
    api, kv_t, D, N, H, Hkv, n_kv, n_past, profs, mm, ML = case
    B, T = len(profs), gpu.Tensor
    dq = T.from_numpy(d["q"], gpu.F32, [D, N, H, B])
    dk = T.from_numpy(d["k"] if kv_t == FM.F16 else d["k"].reshape(-1), kv_t, [D, n_kv, Hkv, B])
    dv = T.from_numpy(d["v"] if kv_t == FM.F16 else d["v"].reshape(-1), kv_t, [D, n_kv, Hkv, B])
    dm = None
    if d["mask"] is not None:
        dm = T.from_numpy(d["mask"], gpu.F16, [n_kv, N] if d["mask"].ndim == 2 else [n_kv, N, H])
    return gpu.ops.flash_attention(dq, dk, dv, dm, float(d["scale"])).numpy().reshape(B, N, H, D)


def run_attn_prefill(gpu, case, d):
    """the K cache [k_hidden, max_len] and the V^T cache [max_len, k_hidden] as the runner keeps them, longer than n_kv: K goes on with the profile (its first
    row past n_kv would carry the largest weight), V holds NaN there"""
    api, kv_t, D, N, H, Hkv, n_kv, n_past, profs, mm, ML = case
    T, KD = gpu.Tensor, D * Hkv
    q = np.ascontiguousarray(d["q"][0].transpose(1, 0, 2))                     # [N, H, D] as the projection leaves it
    kc = np.ascontiguousarray(d["k"][0].transpose(1, 0, 2)).reshape(ML, KD)
    vc = np.ascontiguousarray(d["v"][0].transpose(0, 2, 1)).reshape(KD, ML)
    vc[:, n_kv:] = np.float16(np.nan)
    dq = T.from_numpy(q, gpu.F32, [D, H, N]).permute(0, 2, 1, 3)
    dk = T.from_numpy(kc, gpu.F16, [KD, ML]).view([D, n_kv, Hkv], [2, KD * 2, D * 2])
    dv = T.from_numpy(vc, gpu.F16, [ML, KD]).view([n_kv, D, Hkv], [2, ML * 2, ML * D * 2])
    with prefill_mode(gpu, 0):
        got = gpu.ops.attn_prefill(dq, dk, dv, float(d["scale"]), n_past).numpy().reshape(H, N, D)
    return np.ascontiguousarray(got.transpose(1, 0, 2))[None]


@pytest.mark.parametrize("case", FM.CASES, ids=FM.case_id)
def test_flash_attention_is_inside_the_bound_at_every_element(gpu, case):
    d = FM.case_data(case)
    ref = d["ref"]
    got = (run_attn_prefill if case[0] == "prefill" else run_flash_attn_ext)(gpu, case, d)
    assert got.shape == ref["R"].shape
    err = np.abs(got.astype(np.float64) - ref["R"])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(ref["bound"] > 0, err / ref["bound"], np.where(err == 0, 0.0, np.inf))
    print(f"\n|got - R| / bound: {np.nanmax(ratio):.3f} {FM.case_id(case)}")
    assert np.all(np.isfinite(got))
    assert np.all(err <= ref["bound"]), (float(np.nanmax(ratio)), int(np.sum(~(err <= ref["bound"]))), np.argwhere(~(err <= ref["bound"]))[:4].tolist())
    assert np.all(got[ref["n_vis"] == 0] == 0.0)                              # nothing visible -> exact zeros
