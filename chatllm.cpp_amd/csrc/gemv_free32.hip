// gemv_free32.hip -- the OPT-IN free-order tier of the decode mat-vec for the 32-weight block formats (Q4_0 / Q4_1 / Q8_0): CLLM_DECODE_FREE_ORDER=1 / cllm_set_decode_free_order(1).
//
// Everything of k_gemv_dec (gemv_decode_kernel.h: the activation built in the kernel, one row per wave, 64 blocks per step, the same prologues and epilogues) except the fp32
// fold: the exact int32 block dot products are scaled and added per lane (q32_block_free, q32.h) and the 64 lanes are summed by the wave at the end of the row -- NOT the order of
// ggml_vec_dot_q4_0_q8_0 / q4_1_q8_1 / q8_0_q8_0 (arch/x86/quants.c:543-577, 701-760, 1012-1040: eight per-AVX-lane fp32 chains over the blocks), which the default kernels
// (gemv_rows32.hip, gemv_team32.hip, k_gemv_dec) reproduce bit for bit.  It exists to PRICE that order (the review's "decide their contract": DESIGN.md section 6, round 6) and as
// a tolerance tier for hosts that ask for it; tests/test_gpu_llama.py states what it keeps (integer sums exact; ids and logits against the exact order at real shapes).
#include "gemv_decode_launch.h"

static int g_free_order = -1;               // 0 / 1 (anything above 1 is 1: the tier is the only form there is)
int decode_free_order() { if (g_free_order < 0) g_free_order = opt_int(OPT_CLLM_DECODE_FREE_ORDER); return g_free_order; }
extern "C" CLLM_API int cllm_set_decode_free_order(int on) { g_free_order = on > 0 ? 1 : 0; return CLLM_OK; }
extern "C" CLLM_API int cllm_get_decode_free_order(void) { return decode_free_order(); }

// the forms the decode step uses: pro 1 (RMS_NORM, + SiLU * up epilogue), pro 2 (plain quantize); anything else: CLLM_E_UNSUPPORTED -> the exact kernels
int launch_gemv_decode_free(hipStream_t st, int wtype, const void * W, int64_t K, int64_t nrows, int pro, const float * px, const float * pw, float eps,
                            int epi, float * dst, const float * bias, const float * resid) {
    if (wtype != CLLM_TYPE_Q4_0 && wtype != CLLM_TYPE_Q4_1 && wtype != CLLM_TYPE_Q8_0) return CLLM_E_UNSUPPORTED;
    if ((pro != 1 && pro != 2) || (epi != 0 && epi != 1) || (epi == 1 && pro != 1)) return CLLM_E_UNSUPPORTED;
    if (epi == 1 && (!gate_up_pairs_ok(nrows) || bias || resid)) return CLLM_E_UNSUPPORTED;
    gemv_dec_plan p; gemv_dec_form f; f.k_max = gemv_k_max(pro); f.units = epi == 1 ? nrows / 2 : nrows; f.grid_cap = device_cu_count();      // (the record area stays: the kernel's LDS layout is k_gemv_dec's)
    if (!gemv_dec_make_plan(p, wtype, K, nrows, f)) return CLLM_E_UNSUPPORTED;
    gemv_dec_args a;
    a.px = px; a.pw = pw; a.W = (const char *) W; a.eps = eps; a.dst = dst; a.bias = bias; a.resid = resid;
    return with_tuned_type(wtype, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        if constexpr (FMT == CLLM_TYPE_Q4_K) return CLLM_E_UNSUPPORTED;      // (refused above: the free-order tier has no Q4_K instantiation)
        else {
            const int npre = p.npre;
            if (pro == 1 && epi == 1) return npre == 1 ? gemv_dec_launch<FMT, 1, 1, 1, false, true>(st, p, a) : gemv_dec_launch<FMT, 1, 1, 4, false, true>(st, p, a);
            if (pro == 1)             return npre == 1 ? gemv_dec_launch<FMT, 1, 0, 1, false, true>(st, p, a) : gemv_dec_launch<FMT, 1, 0, 4, false, true>(st, p, a);
            return npre == 1 ? gemv_dec_launch<FMT, 2, 0, 1, false, true>(st, p, a) : npre == 4 ? gemv_dec_launch<FMT, 2, 0, 4, false, true>(st, p, a) : gemv_dec_launch<FMT, 2, 0, 8, false, true>(st, p, a);
        }
    });
}
