#pragma once
// gemv_decode_launch.h -- the host side of k_gemv_dec (gemv_decode_kernel.h), shared by its eight launchers (gemv_decode.hip, gemv_free32.hip, gemv_moe.hip, gemv_tp.hip):
//   gemv_dec_form / gemv_dec_plan + gemv_dec_make_plan()  the shape refusals every form shares, the ONE LDS sum (refused and launched with), the deal of units to waves, npre
//   gemv_dec_args                         the kernel's arguments by name; the three slots a family overloads are set through setters named as the kernel names them
//   gemv_dec_launch<...>()                the attribute (once per device and instantiation) + the launch
// The four-way ladder over the weight type is with_tuned_type() of types.h: leaf(std::integral_constant<int, FMT>), the leaf names the (PRO, EPI, NPRE) forms of its launcher.
// Host code only: which instantiations a translation unit holds, and in which order, is decided by the leaves its launchers name -- see gemv_decode.hip on why that matters.
#include <type_traits>
#include "gemv_decode_kernel.h"

// nblk / kfull / nrem are kernel arguments (units = kfull rounds of 16 * grid_x waves + nrem); lds = activation rows + the 16 waves' chain records + the form's extra
struct gemv_dec_plan { int nblk, kfull, nrem, npre; unsigned grid_x, grid_y; size_t lds; };

static inline bool gate_up_pairs_ok(int64_t nrows) { return nrows % 2 == 0 && (nrows / 2) % 8 == 0; }      // EPI 1 / 5: rows alternate gate_u, up_u; a wave's stores cover 8 features

// What a form asks of the plan.  k_max: its K bound (gemv_k_max(pro), or its own); units: rows, or gate / up pairs; grid_cap: workgroups along x (the CUs, shared by the slots
// where there are some); grid_y: slots; act_rows: activation rows in LDS (2: the combine's two slots); extra_lds: what the form keeps behind the chain records
struct gemv_dec_form { int64_t k_max = 0, units = 0, grid_cap = 1; int grid_y = 1, act_rows = 1; size_t extra_lds = 0; };

// false: CLLM_E_UNSUPPORTED.  (Within every form's K bound the LDS sum stays below the limit -- 129280 bytes at most, the combine of a 32-weight format at K 32768:
//  tests/moe_model.py -- so that refusal decides nothing today; it is the guard of the next form.)
static inline bool gemv_dec_make_plan(gemv_dec_plan & p, int wtype, int64_t K, int64_t nrows, const gemv_dec_form & f) {
    const int kind = wtype_blck(wtype);
    if (!is_quant_type(wtype) || K % kind || K > f.k_max || nrows <= 0 || (uint64_t) nrows * (uint64_t) cllm_row_size(wtype, K) >= (1ull << 32)) return false;
    p.lds = f.act_rows * act_row_bytes(K, kind) + 16 * (size_t)(wtype == CLLM_TYPE_Q4_K ? Q4K_CHAIN_BYTES : Q32_CHAIN_BYTES) + f.extra_lds;
    if (p.lds > K_GEMV_DEC_MAX_DYN_LDS) return false;
    int64_t grid = (f.units + 15) / 16;
    if (grid > f.grid_cap) grid = f.grid_cap;
    if (grid < 1) grid = 1;                   // (no units, or no CU to a slot: a launcher's own refusal may follow the plan)
    const int64_t nwaves = grid * 16;
    p.nblk = (int)(K / kind); p.kfull = (int)(f.units / nwaves); p.nrem = (int)(f.units % nwaves); p.npre = gemv_npre(K);
    p.grid_x = (unsigned) grid; p.grid_y = (unsigned) f.grid_y;
    return true;
}

// The kernel's parameters that are not the plan's, zero until a launcher sets them.  px / pw / padd / xout / ids and the two strides mean different things by family: the
// setters below are the host's side of the "argument slots BY FAMILY" table at the top of the kernel body, under the same names.
struct gemv_dec_args {
    const float * px = nullptr, * pw = nullptr, * padd = nullptr;
    const char * W = nullptr;
    float eps = 0.0f;
    float * dst = nullptr, * xout = nullptr;
    const float * bias = nullptr, * resid = nullptr;
    unsigned long long * ts = nullptr;
    const int32_t * ids = nullptr;
    unsigned long long w_expert_bytes = 0;
    int px_slot_stride = 0, dst_slot_stride = 0;
    // sparse MoE
    void moe_ids(const int32_t * picked)   { ids = picked; }                          // MOE / EPI 3: the experts picked by an earlier launch
    void topk_out(int32_t * picks)         { ids = picks; }                           // EPI 2 / 5: where this launch writes its picks
    void topk_k(int k)                     { dst_slot_stride = k; }                   // EPI 2
    void n_experts(int n)                  { px_slot_stride = n; }                    // EPI 5
    void router_w(const void * rows)       { padd = (const float *) rows; }           // EPI 5
    void moe_probs(const float * probs)    { pw = probs; }                            // EPI 3
    void probs_out(float * probs)          { xout = probs; }                          // EPI 5
    void xnorm_out(float * xnorm)          { xout = xnorm; }                          // EPI 2: the normalised activation
    void act_slot_stride(int64_t s)        { px_slot_stride = (int) s; }              // MOE / EPI 3 (the launcher has refused s > INT32_MAX)
    void out_slot_stride(int64_t s)        { dst_slot_stride = (int) s; }             // MOE / EPI 5
    // tensor parallel
    void tp_ctx(const void * ctx_dev)      { ids = (const int32_t *) ctx_dev; }       // PRO 5 / EPI 4: the tp_fuse_dev context
    void tp_site_in(int site)              { px_slot_stride = site; }                 // PRO 5: the site gathered
    void tp_site_out(int site)             { dst_slot_stride = site; }                // EPI 4: the site scattered to
};

template <int FMT, int PRO, int EPI, int NPRE, bool MOE = false, bool FREE = false>
static int gemv_dec_launch(hipStream_t st, const gemv_dec_plan & p, const gemv_dec_args & a) {
    static uint64_t attr = 0;
    if (p.lds > 64 * 1024) if (const int rc = lds_opt_in(k_gemv_dec<FMT, PRO, EPI, NPRE, MOE, FREE>, attr, K_GEMV_DEC_MAX_DYN_LDS)) return rc;
    hipLaunchKernelGGL((k_gemv_dec<FMT, PRO, EPI, NPRE, MOE, FREE>), dim3(p.grid_x, p.grid_y), dim3(1024), p.lds, st, a.px, a.pw, a.padd, a.W, p.nblk, p.kfull, p.nrem, a.eps,
                       a.dst, a.xout, a.bias, a.resid, a.ts, a.ids, a.w_expert_bytes, a.px_slot_stride, a.dst_slot_stride);
    LAUNCH_CHECK();
    return CLLM_OK;
}
