// fattn_pad.hip -- k_fattn (fattn.h) at a head size that is no multiple of 32: 112.  F16 rows by position only (a Q8_0 row is whole blocks of 32:
// fattn_dispatch declines it), the feature rows of the P.V product padded to fa_dp<D>() = 128 (fattn.h's D = 112 paragraph): launch_fattn (fattn.hip)
// plans, fattn_pad_launch launches.  A translation unit of its own like fattn_hs.hip, and for the same two reasons: compiled without the packed fp32
// VALU forms (the Makefile's target-specific flag), and its three kernels and one merge build beside the other two files' instead of after them.
// 80 is not here: tests/test_gpu_fattn.py holds it as the head size the entry declines.
#include "fattn.h"

int fattn_pad_launch(hipStream_t st, const fattn_args & a, int D, int ktype, int mmode, int B, bool decode) {
    if (D == 112) return fattn_dispatch<112>(st, a, ktype, 0, mmode, B, decode);
    return CLLM_E_UNSUPPORTED;
}
