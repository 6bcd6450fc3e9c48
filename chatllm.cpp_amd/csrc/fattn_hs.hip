// fattn_hs.hip -- k_fattn (fattn.h) at head sizes 96 (Phi-3-mini class, vision / audio towers) and 256 (the Gemma line), V rows by position only:
// launch_fattn (fattn.hip) plans, fattn_hs_launch launches.  A translation unit of its own for two reasons: it is compiled without the packed fp32
// VALU forms (the Makefile's target-specific flag), and its twelve kernels build beside fattn.hip's eighteen instead of after them.
#include "fattn.h"

int fattn_hs_launch(hipStream_t st, const fattn_args & a, int D, int ktype, int mmode, int B, bool decode) {
    if (D == 96) return fattn_dispatch<96>(st, a, ktype, 0, mmode, B, decode);
    if (D == 256) return fattn_dispatch<256>(st, a, ktype, 0, mmode, B, decode);
    return CLLM_E_UNSUPPORTED;
}
