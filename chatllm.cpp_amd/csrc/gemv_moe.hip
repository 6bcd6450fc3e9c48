// gemv_moe.hip -- the sparse-MoE forms of the decode mat-vec (k_gemv_dec EPI 2: router, EPI 3: down projection + combine), instantiated apart from
// the dense decode kernels (see gemv_decode.hip).
#include "gemv_decode_launch.h"

// The router of a sparse-MoE block for ONE token as one launch of one workgroup (the reference's nodes RMS_NORM -> MUL -> MUL_MAT(gate) -> SOFT_MAX ->
// TOP_K, GenericSparseMLP::forward src/layers.cpp:3792-3830): xnorm[K] = RMS_NORM(px) * pw, probs[n] = SOFT_MAX(W . quantize(xnorm)), ids[k] = TOP_K(probs).
// Same reductions in the same order as the separate kernels: bit-identical.  n <= 64 experts, K <= 16384; CLLM_E_UNSUPPORTED otherwise.
int launch_moe_router(hipStream_t st, int wtype, const void * W, int64_t K, int64_t n, const float * px, const float * pw, float eps,
                      float * xnorm, float * probs, int32_t * ids, int k) {
    if (K % 4 || n > 64 || k < 1 || k > n) return CLLM_E_UNSUPPORTED;
    gemv_dec_plan p; gemv_dec_form f; f.k_max = 16384; f.units = n; f.grid_cap = 1; f.extra_lds = 2 * 64 * sizeof(float);      // ONE workgroup; + logits, probabilities
    if (!gemv_dec_make_plan(p, wtype, K, n, f)) return CLLM_E_UNSUPPORTED;
    gemv_dec_args a;
    a.px = px; a.pw = pw; a.W = (const char *) W; a.eps = eps; a.dst = probs;
    a.xnorm_out(xnorm); a.topk_out(ids); a.topk_k(k);
    return with_tuned_type(wtype, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        return p.npre == 1 ? gemv_dec_launch<FMT, 1, 2, 1>(st, p, a) : gemv_dec_launch<FMT, 1, 2, 4>(st, p, a);
    });
}

// MUL_MAT_ID(down experts) for ONE token with TWO slots + the tail of the sparse-MoE block in one launch (EPI 3 above):
//   dst[r] = (W[ids[0]][r] . quantize(px[:, 0])) * w0 + (W[ids[1]][r] . quantize(px[:, 1])) * w1 (+ resid[r]),  w_j = probs[ids[j]] / (probs[ids[0]] + probs[ids[1]])
// the arithmetic of MUL_MAT_ID -> GET_ROWS -> SUM_ROWS -> DIV -> MUL -> ADD (-> ADD) in their order: bit-identical.  dst may be resid; CLLM_E_UNSUPPORTED otherwise
int launch_gemv_decode_id_combine(hipStream_t st, int wtype, const void * W, size_t w_expert_bytes, int64_t K, int64_t nrows, const float * px, int64_t px_slot_stride,
                                  const int32_t * ids, const float * probs, const float * resid, float * dst) {
    if (px_slot_stride > INT32_MAX || px_slot_stride % 4) return CLLM_E_UNSUPPORTED;
    gemv_dec_plan p; gemv_dec_form f; f.k_max = 32768; f.units = nrows; f.grid_cap = device_cu_count(); f.act_rows = 2;      // the two slots' activation rows
    if (!gemv_dec_make_plan(p, wtype, K, nrows, f)) return CLLM_E_UNSUPPORTED;
    gemv_dec_args a;
    a.px = px; a.W = (const char *) W; a.dst = dst; a.resid = resid; a.w_expert_bytes = w_expert_bytes;
    a.moe_ids(ids); a.moe_probs(probs); a.act_slot_stride(px_slot_stride);
    return with_tuned_type(wtype, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        return p.npre == 1 ? gemv_dec_launch<FMT, 2, 3, 1>(st, p, a) : p.npre == 4 ? gemv_dec_launch<FMT, 2, 3, 4>(st, p, a) : gemv_dec_launch<FMT, 2, 3, 8>(st, p, a);
    });
}

// The head of a sparse-MoE block AND its experts' gate / up projections for ONE token as one launch (EPI 5 above): RMS_NORM -> MUL -> MUL_MAT(router) -> SOFT_MAX -> TOP_K ->
// {MUL_MAT_ID(gate), MUL_MAT_ID(up)} -> SiLU -> MUL (GenericSparseMLP::forward src/layers.cpp:3792-3872) -- every workgroup redoes the router behind its norm prologue, slot
// blockIdx.y streams the rows of expert ids[slot].  probs[ne] / ids[k] are published for the down + combine launch.  W: the per-expert interleaved gate / up pack (rows 2u = gate_u,
// 2u + 1 = up_u), nrows = 2 F; dst[u + slot * dst_slot_stride].  The same reductions in the same order as the separate launches: bit-identical.  CLLM_E_UNSUPPORTED otherwise.
int launch_gemv_decode_id_router_silu(hipStream_t st, int wtype, const void * W, size_t w_expert_bytes, int64_t K, int64_t nrows, const float * px, const float * pw, float eps,
                                      const void * Wr, int ne, int k, float * probs, int32_t * ids, float * dst, int64_t dst_slot_stride) {
    if (K % 4 || ne < 1 || ne > 64 || k < 1 || k > ne || !gate_up_pairs_ok(nrows) || dst_slot_stride > INT32_MAX) return CLLM_E_UNSUPPORTED;
    gemv_dec_plan p; gemv_dec_form f; f.k_max = 16384; f.units = nrows / 2; f.grid_cap = device_cu_count() / k; f.grid_y = k; f.extra_lds = 3 * 64 * sizeof(float);      // + logits, probabilities, ids
    if (!gemv_dec_make_plan(p, wtype, K, nrows, f)) return CLLM_E_UNSUPPORTED;
    gemv_dec_args a;
    a.px = px; a.pw = pw; a.W = (const char *) W; a.eps = eps; a.dst = dst; a.w_expert_bytes = w_expert_bytes;
    a.router_w(Wr); a.n_experts(ne); a.probs_out(probs); a.topk_out(ids); a.out_slot_stride(dst_slot_stride);
    return with_tuned_type(wtype, [&](auto fmt) {
        constexpr int FMT = decltype(fmt)::value;
        return p.npre == 1 ? gemv_dec_launch<FMT, 1, 5, 1, true>(st, p, a) : gemv_dec_launch<FMT, 1, 5, 4, true>(st, p, a);
    });
}
