// fattn_cap.hip -- k_fattn (fattn.h) with the logit soft-cap (CAP: s = cap tanh(scale / cap K.Q) + mask; Gemma-2 on caps at 50, Grok at 30) at the head sizes that
// have a caller: 128 and 256, F16 / Q8_0 rows by position, no mask or a mask tensor (the position-causal form is cllm_op_attn_prefill's, which has no
// cap): eight kernels, and k_fattn_merge at both sizes for the split-KV decode.  launch_fattn (fattn.hip) validates the cap, sets a.cap_in and a.sc2 and
// plans; fattn_cap_launch launches.  A translation unit of its own like fattn_hs.hip: it holds D = 256, so it is compiled without the packed fp32 VALU
// forms (the Makefile's target-specific flag), and fattn_hs.hip keeps the kernel count its resource test holds it to.
#include "fattn.h"

template <int D>
static int fattn_cap_dispatch(hipStream_t st, const fattn_args & a, int ktype, int mmode, int B, bool decode) {
    if (mmode == 1) return CLLM_E_UNSUPPORTED;
    if (ktype == CLLM_TYPE_Q8_0) return mmode ? fattn_go<D, CLLM_TYPE_Q8_0, 0, 2, true>(st, a, B, decode) : fattn_go<D, CLLM_TYPE_Q8_0, 0, 0, true>(st, a, B, decode);
    return mmode ? fattn_go<D, CLLM_TYPE_F16, 0, 2, true>(st, a, B, decode) : fattn_go<D, CLLM_TYPE_F16, 0, 0, true>(st, a, B, decode);
}

int fattn_cap_launch(hipStream_t st, const fattn_args & a, int D, int ktype, int mmode, int B, bool decode) {
    if (D == 128) return fattn_cap_dispatch<128>(st, a, ktype, mmode, B, decode);
    if (D == 256) return fattn_cap_dispatch<256>(st, a, ktype, mmode, B, decode);
    return CLLM_E_UNSUPPORTED;
}
