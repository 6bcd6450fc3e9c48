"""flash attention (k_fattn, fattn.h) at head sizes 96 / 128 / 256 at equal H * D = 6144 (equal Q.K and P.V FLOPs): prefill 4096 x 4096 with a causal mask tensor, decode
1 x 4096 cached positions; F16 and Q8_0.  Device events, 3 warm-up launches, median of 20 timed windows (decode: 10 launches per window).

Then (alone with the argument `112`) the head size 112 (F16 rows only) beside the kernel whose P.V work it issues, 128, at equal H * D = 7168 (H 64 | 56),
and 96 at 5760 (H 60) for the line through the two unpadded kernels; H % 4 == 0, three rounds, the sizes alternating inside a round.  The rates count
useful FLOPs (D, not the padded feature count).

With the argument `softcap` alone: the prefill at 128 and 256 with logit_softcap 50 and with 0, alternating, three runs each."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402
import fattn_model as FM  # noqa: E402

gpu = load_package()
L = gpu.lib.get()
gpu.lib.require_gpu()
T, ops = gpu.Tensor, gpu.ops


def median_ms(fn, per=1, reps=20):
    for _ in range(3):
        fn()
    ev = []
    for _ in range(reps):
        a, b = C.c_void_p(), C.c_void_p()
        gpu.lib.check(L.cllm_event_create(C.byref(a)), "ev"); gpu.lib.check(L.cllm_event_create(C.byref(b)), "ev")
        gpu.lib.check(L.cllm_event_record(a, None), "rec")
        for _ in range(per):
            fn()
        gpu.lib.check(L.cllm_event_record(b, None), "rec")
        ev.append((a, b))
    out = []
    for a, b in ev:
        gpu.lib.check(L.cllm_event_sync(b), "sync")
        ms = C.c_float()
        gpu.lib.check(L.cllm_event_elapsed_ms(a, b, C.byref(ms)), "el")
        out.append(ms.value / per)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def kv(r, kv_t, D, n_kv, Hkv, s):
    x = (r.standard_normal((Hkv, n_kv, D)) * s).astype(np.float32)
    if kv_t == FM.F16:
        return T.from_numpy(x.astype(np.float16), gpu.F16, [D, n_kv, Hkv]), D * 2
    return T.from_numpy(FM.q8_0_quantize(x).reshape(-1), gpu.Q8_0, [D, n_kv, Hkv]), D // 32 * 34


def run(D, kv_t, N, n_kv, mask, HD=6144, cap=0.0):
    H = HD // D
    Hkv = H // 4
    r = np.random.default_rng(D + N)
    q = T.from_numpy(r.standard_normal((H, N, D)).astype(np.float32), gpu.F32, [D, N, H])
    k, rb = kv(r, kv_t, D, n_kv, Hkv, 0.5)
    v, _ = kv(r, kv_t, D, n_kv, Hkv, 1.0)
    dst = T(gpu.F32, [D, H, N])
    name = ("F16 " if kv_t == FM.F16 else "Q8_0") + (f" cap {cap:g}" if cap else "")
    fn = lambda: ops.flash_attention(q, k, v, mask, 1.0 / np.sqrt(D), logit_softcap=cap, dst=dst)
    if N > 1:
        med, lo, hi = median_ms(fn)
        fl = 4.0 * N * n_kv * D * H / 2
        print(f"prefill {N} x {n_kv} causal mask  D={D:3d} H={H:2d} Hkv={Hkv:2d} {name}: median {med:8.3f} ms (min {lo:.3f}, max {hi:.3f})  {fl / med / 1e9:7.1f} TFLOP/s (causal flops)", flush=True)
    else:
        med, lo, hi = median_ms(fn, per=10)
        by = 2.0 * n_kv * Hkv * rb
        print(f"decode 1 x {n_kv}                 D={D:3d} H={H:2d} Hkv={Hkv:2d} {name}: median {med * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  cache {by / 1e6:6.2f} MB  {by / med / 1e9:6.3f} TB/s", flush=True)


N = 4096
m = np.zeros((N, N), np.float16)
m[np.triu_indices(N, 1)] = -np.inf
dm = T.from_numpy(m, gpu.F16, [N, N])
if sys.argv[1:] == ["softcap"]:           # what the logit soft-cap costs: the same shapes with cap 50 and without, alternating, three runs each
    for D in (128, 256):
        for _ in range(3):
            for cap in (50.0, 0.0):
                run(D, FM.F16, N, N, dm, cap=cap)
    sys.exit(0)
if sys.argv[1:] != ["112"]:
    for kv_t in (FM.F16, FM.Q8_0):
        for D in (128, 96, 256):
            run(D, kv_t, N, N, dm)
    for kv_t in (FM.F16, FM.Q8_0):
        for D in (128, 96, 256):
            run(D, kv_t, 1, N, None)
PAIRS = ((96, 5760), (112, 7168), (128, 7168))
for n, mask in ((N, dm), (1, None)):
    for _ in range(3):
        for D, HD in PAIRS:
            run(D, FM.F16, n, N, mask, HD)
