// gemv_decode.hip -- the launchers of the decode step's quantized mat-vec (the kernel: gemv_decode_kernel.h; plan, named arguments and launch: gemv_decode_launch.h).  The sparse-MoE forms (router, down + combine)
// are instantiated in gemv_moe.hip: their code stays out of this code object, whose layout the decode step's launch-to-launch time is sensitive to
// (the same kernels, bit for bit, measured 1.8 % slower per decode step with the MoE instantiations placed among them).
#include "gemv_decode_launch.h"

static unsigned long long * g_gemv_ts = nullptr;
extern "C" __attribute__((visibility("default"))) void cllm_debug_set_mmvq_ts(unsigned long long * dev_buf) { g_gemv_ts = dev_buf; }   // tools only

// K a multiple of the block size, K <= 16384 (32768 for the plain-quantize prologue), nrows * row bytes < 4 GiB; returns
// CLLM_E_UNSUPPORTED for shapes the general kernels must take
int launch_gemv_decode(hipStream_t st, int wtype, const void * W, int64_t K, int64_t nrows, int pro, const float * px, const float * pw, float eps,
                       int epi, float * dst, const float * bias, const float * resid, const float * padd, float * xout) {
    if (!is_quant_type(wtype)) return CLLM_E_UNSUPPORTED;
    if (wtype != CLLM_TYPE_Q4_K && !padd && !g_gemv_ts && decode_free_order()) {      // opt-in: the free-order tier of the 32-weight block formats (gemv_free32.hip)
        const int rc = launch_gemv_decode_free(st, wtype, W, K, nrows, pro, px, pw, eps, epi, dst, bias, resid);
        if (rc != CLLM_E_UNSUPPORTED) return rc;
    }
    if (wtype == CLLM_TYPE_Q4_K && !padd && !g_gemv_ts) {          // the LDS-staged form (gemv_rows.hip) where the shape suits it
        const int rc = launch_gemv_rows(st, W, K, nrows, pro, px, pw, eps, epi, dst, bias, resid);
        if (rc != CLLM_E_UNSUPPORTED) return rc;
    }
    if (wtype != CLLM_TYPE_Q4_K && !padd && !g_gemv_ts) {          // Q4_0 / Q4_1 / Q8_0: the LDS-staged one-lane-group-per-row form (gemv_rows32.hip)
        int rc = launch_gemv_rows32(st, wtype, W, K, nrows, pro, px, pw, eps, epi, dst, bias, resid);
        if (rc != CLLM_E_UNSUPPORTED) return rc;
        rc = launch_gemv_team32(st, wtype, W, K, nrows, pro, px, pw, eps, epi, dst, bias, resid);      // few rows per CU: teams of waves per 8 rows (gemv_team32.hip)
        if (rc != CLLM_E_UNSUPPORTED) return rc;
    }
    if (pro < 1 || pro > 4) return CLLM_E_UNSUPPORTED;
    gemv_dec_plan p; gemv_dec_form f; f.k_max = gemv_k_max(pro); f.units = epi == 1 ? nrows / 2 : nrows; f.grid_cap = device_cu_count();
    if (!gemv_dec_make_plan(p, wtype, K, nrows, f)) return CLLM_E_UNSUPPORTED;
    if (padd && (pro != 1 || K > 4096 || !xout || xout == px)) return CLLM_E_UNSUPPORTED;
    if (epi == 1 && (pro != 1 || !gate_up_pairs_ok(nrows) || bias || resid)) FAIL(CLLM_E_UNSUPPORTED, "gemv_decode: SiLU epilogue needs gate/up row pairs, features %% 8 == 0");
    gemv_dec_args a;
    a.px = px; a.pw = pw; a.padd = padd; a.W = (const char *) W; a.eps = eps; a.dst = dst; a.xout = xout; a.bias = bias; a.resid = resid; a.ts = g_gemv_ts;
    return with_tuned_type(wtype, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        const int npre = p.npre;
        if (pro == 1 && epi == 1) return npre == 1 ? gemv_dec_launch<FMT, 1, 1, 1>(st, p, a) : gemv_dec_launch<FMT, 1, 1, 4>(st, p, a);
        if (pro == 1)             return npre == 1 ? gemv_dec_launch<FMT, 1, 0, 1>(st, p, a) : gemv_dec_launch<FMT, 1, 0, 4>(st, p, a);
        if (pro == 2)             return npre == 1 ? gemv_dec_launch<FMT, 2, 0, 1>(st, p, a) : npre == 4 ? gemv_dec_launch<FMT, 2, 0, 4>(st, p, a) : gemv_dec_launch<FMT, 2, 0, 8>(st, p, a);
        if (pro == 4)             return npre == 1 ? gemv_dec_launch<FMT, 4, 0, 1>(st, p, a) : npre == 4 ? gemv_dec_launch<FMT, 4, 0, 4>(st, p, a) : gemv_dec_launch<FMT, 4, 0, 8>(st, p, a);
        return                           npre == 1 ? gemv_dec_launch<FMT, 3, 0, 1>(st, p, a) : gemv_dec_launch<FMT, 3, 0, 4>(st, p, a);
    });
}

// MUL_MAT_ID for ONE token: n_slots x (dst[:, slot] = W_expert(ids[slot]) . quantize(px + slot * px_slot_stride)), the activation quantized inside
// the kernel (prologue 2) -- one launch instead of quantize + mat-vec, and the decode kernel's streaming.  CLLM_E_UNSUPPORTED: general path.
// epi 1: every expert's rows alternate gate_u, up_u (cllm_pack_rows, interleave); dst[u, slot] = silu(gate_u . x) * (up_u . x), u < nrows / 2
int launch_gemv_decode_id(hipStream_t st, int wtype, const void * W, size_t w_expert_bytes, int64_t K, int64_t nrows, const float * px, int64_t px_slot_stride,
                          const int32_t * ids, int n_slots, float * dst, int64_t dst_slot_stride, int epi) {
    if (n_slots < 1 || n_slots > 64 || px_slot_stride > INT32_MAX || dst_slot_stride > INT32_MAX) return CLLM_E_UNSUPPORTED;
    if (epi != 0 && (epi != 1 || !gate_up_pairs_ok(nrows))) return CLLM_E_UNSUPPORTED;
    gemv_dec_plan p; gemv_dec_form f; f.k_max = 32768; f.units = epi == 1 ? nrows / 2 : nrows; f.grid_cap = device_cu_count() / n_slots; f.grid_y = n_slots;
    if (!gemv_dec_make_plan(p, wtype, K, nrows, f)) return CLLM_E_UNSUPPORTED;
    gemv_dec_args a;
    a.px = px; a.W = (const char *) W; a.dst = dst; a.w_expert_bytes = w_expert_bytes;
    a.moe_ids(ids); a.act_slot_stride(px_slot_stride); a.out_slot_stride(dst_slot_stride);
    return with_tuned_type(wtype, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        const int npre = p.npre;
        if (epi == 1) return npre == 1 ? gemv_dec_launch<FMT, 2, 1, 1, true>(st, p, a) : npre == 4 ? gemv_dec_launch<FMT, 2, 1, 4, true>(st, p, a) : gemv_dec_launch<FMT, 2, 1, 8, true>(st, p, a);
        return               npre == 1 ? gemv_dec_launch<FMT, 2, 0, 1, true>(st, p, a) : npre == 4 ? gemv_dec_launch<FMT, 2, 0, 4, true>(st, p, a) : gemv_dec_launch<FMT, 2, 0, 8, true>(st, p, a);
    });
}
