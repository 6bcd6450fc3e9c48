"""GPU parity of GGML_OP_FLASH_ATTN_EXT with a logit soft-cap (k_fattn's CAP form, fattn_cap.hip: head sizes 128 / 256, F16 / Q8_0 K / V):
    s = cap * tanh(scale / cap * K[kv] . Q[n]) + mask[kv, n], then the soft-max and P.V
against the same formula in float64 over the same converted operands as test_gpu_fattn.exact(): rel_err < FA_EXACT, the kernel's own figure against
float64 (the hardware tanh adds about 1e-5 relative to a probability: fattn.h, fa_tanh).  The oracle's flash attention has no cap argument: no oracle
leg.  Every case first shows on the CPU that its cap bites: the float64 result without the cap is further than 10 FA_EXACT from the one with it."""
import numpy as np
import pytest

import oracle as O
from test_gpu_fattn import FA_EXACT, deq, exact, make_case, rel_err

pytestmark = pytest.mark.gpu


def exact_capped(kv_t, q, k, v, mask, scale, D, cap):
    H, Hkv = q.shape[0], k.shape[0]
    qc = q.astype(np.float16) if kv_t == O.F16 else np.stack([O.dequantize(O.Q8_0, O.quantize_q8_0(row), D) for row in q.reshape(-1, D)]).reshape(q.shape)
    qc, K, V = qc.astype(np.float64), deq(kv_t, k, D), deq(kv_t, v, D)
    out = np.zeros((q.shape[1], H, D))
    for h in range(H):
        s = cap * np.tanh(qc[h] @ K[h // (H // Hkv)].T * (scale / cap)) + (0.0 if mask is None else mask.astype(np.float64))
        mx = np.max(s, axis=1, keepdims=True)
        mx[~np.isfinite(mx)] = 0.0
        p = np.exp(s - mx)
        l = p.sum(axis=1, keepdims=True)
        out[:, h, :] = np.where(l > 0, (p @ V[h // (H // Hkv)]) / np.where(l > 0, l, 1.0), 0.0)
    return out


CASES = [
    # kv type, D, N, H, Hkv, n_kv, mask, cap, factor of q
    (O.F16, 128, 1, 8, 2, 38, None, 2.0, 1),            # one tile, decode, packed GQA rows
    (O.F16, 128, 1, 8, 2, 300, "causal", 2.0, 1),       # split-KV + merge
    (O.F16, 128, 200, 4, 2, 200, "causal", 2.0, 1),     # prefill: two query blocks, ragged tiles, masked tiles
    (O.F16, 128, 40, 4, 2, 96, "bias", 2.0, 1),         # finite additive mask on top of the cap, fully masked tiles, one fully masked query
    (O.F16, 256, 130, 2, 1, 130, "causal", 50.0, 40),   # the Gemma cap at the one-workgroup-per-CU size
    (O.F16, 256, 1, 4, 2, 300, None, 50.0, 40),
    (O.Q8_0, 128, 96, 8, 2, 160, "causal", 2.0, 1),     # quantized caches at both sizes
    (O.Q8_0, 256, 1, 4, 2, 200, None, 30.0, 40),
    (O.F16, 128, 16, 4, 2, 70, None, 0.5, 40),          # saturation: |scale / cap * K.Q| far past 44, where exp2 overflows: scores exactly +-cap, no NaN
]


def parity(gpu, kv_t, D, N, H, Hkv, n_kv, mask_mode, cap, qmul):
    q, k, v, mask = make_case(kv_t, D, N, H, Hkv, n_kv, n_kv - N, mask_mode, seed=n_kv * 7 + N)
    q = q * np.float32(qmul)
    scale = 1.0 / np.sqrt(D)
    ref = exact_capped(kv_t, q, k, v, mask, scale, D, cap)
    assert rel_err(exact(kv_t, q, k, v, mask, scale, D), ref) > 10 * FA_EXACT          # the case can see the cap
    T = gpu.Tensor
    dq = T.from_numpy(q, gpu.F32, [D, N, H])
    dk = T.from_numpy(k if kv_t == O.F16 else k.reshape(-1), kv_t, [D, n_kv, Hkv])
    dv = T.from_numpy(v if kv_t == O.F16 else v.reshape(-1), kv_t, [D, n_kv, Hkv])
    dm = T.from_numpy(mask, gpu.F16, [n_kv, N]) if mask is not None else None
    got = gpu.ops.flash_attention(dq, dk, dv, dm, scale, logit_softcap=cap).numpy().reshape(N, H, D)
    assert np.all(np.isfinite(got))
    e = rel_err(got, ref)
    print(f"rel_err / FA_EXACT: {e / FA_EXACT:.3f}")
    assert e < FA_EXACT, e
    if mask_mode == "bias":
        assert np.all(got[N // 2] == 0.0)                # nothing visible -> exact zeros


def test_flash_attn_ext_logit_softcap(gpu):
    """every case of the table (a failure names its case), then the declines: a cap at head sizes 64 and 96, and a negative cap"""
    for case in CASES:
        try:
            parity(gpu, *case)
        except AssertionError as err:
            raise AssertionError(f"case {case}: {err}") from err
    T = gpu.Tensor
    for D, cap in ((64, 2.0), (96, 2.0), (128, -1.0)):
        q = T.from_numpy(np.zeros((2, 1, D), np.float32), gpu.F32, [D, 1, 2])
        k = T.from_numpy(np.zeros((2, 4, D), np.float16), gpu.F16, [D, 4, 2])
        with pytest.raises(Exception):
            gpu.ops.flash_attention(q, k, k, None, 1.0, logit_softcap=cap)
