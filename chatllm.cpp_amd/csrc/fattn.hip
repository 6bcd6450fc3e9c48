// fattn.hip -- flash attention's entry points (launch_fattn: validation and the split plan for every head size; launch_attn_long_flash: the
// long-context decode step) and the instantiations of k_fattn (fattn.h) at head sizes 64 and 128; 96 and 256 are fattn_hs.hip, 112 is fattn_pad.hip,
// the logit soft-cap at 128 and 256 is fattn_cap.hip.
#include "fattn.h"

static int g_flash_min = -1;             // -1: not read yet
int flash_prefill_min_cols() {
    if (g_flash_min < 0) {
        // the same threshold as the MFMA mat-muls it replaces (matmul_f.hip): <= 32 columns stay exact
        g_flash_min = opt_int(OPT_CLLM_FLASH_PREFILL) == 0 ? 1 << 30 : opt_int(OPT_CLLM_MMA_MIN_COLS);
    }
    return g_flash_min;
}
// tests: switch the runner's prefill attention between the flash kernel and the node sequence inside one process (<= 0: back to the environment)
extern "C" __attribute__((visibility("default"))) void cllm_debug_set_attn_prefill_min_cols(int n) { g_flash_min = n > 0 ? n : -1; }
// split-KV partials exist only on the decode path (N * (H / Hkv) <= 32 query rows per KV head, so N <= 32): a prompt needs no scratch at all
// (it used to be sized for every N: 8.9 GB for a 2048-token -fa prefill that never touched it)
size_t fattn_wsize(int64_t N, int64_t H, int64_t B, int64_t D) { return N > 32 ? 0 : (size_t) B * H * N * FA_MAX_SPLITS * (D + 4) * 4; }

// q F32 [D, N, H, B]; k [D, n_kv, Hkv, B]; v: vl 0 [D, n_kv, Hkv, B], vl 1 [n_kv(ML), D, Hkv, B] (F16); mask F16 [n_kv, N, ..] or null;
// causal_past >= 0 (no mask tensor): position kv is visible to query n iff kv <= causal_past + n.
// dst element (dv, h, n, b) at dst.data + n * nbn + h * nbh + b * nbb.  CLLM_E_UNSUPPORTED: a shape / layout this kernel does not take.
// cap: the logit soft-cap (0: none); fattn_cap.hip has it at D = 128 / 256 with V rows by position and no causal_past.
int launch_fattn(hipStream_t st, const tview & q, const tview & k, int ktype, const tview & v, int vl, const tview * mask, int causal_past,
                 char * dst, int64_t nbn, int64_t nbh, int64_t nbb, float scale, float cap, void * wdata, size_t wsize) {
    const int64_t D = q.ne[0], N = q.ne[1], H = q.ne[2], B = q.ne[3], n_kv = k.ne[1], Hkv = k.ne[2];
    const bool hs = D == 96 || D == 256;                   // fattn_hs.hip (V rows by position only)
    const bool pad = D == 112;                             // fattn_pad.hip (V rows by position only, F16)
    if (!(cap >= 0.0f) || isinf(cap) || (cap != 0.0f && !isfinite(scale / cap))) FAIL(CLLM_E_INVALID, "flash_attn_ext: logit_softcap %g (scale %g)", (double) cap, (double) scale);
    if (cap != 0.0f && !((D == 128 || D == 256) && vl == 0 && causal_past < 0)) return CLLM_E_UNSUPPORTED;
    if (D != 64 && D != 128 && !((hs || pad) && vl == 0)) return CLLM_E_UNSUPPORTED;
    if (k.ne[0] != D || (vl == 0 ? v.ne[0] != D || v.ne[1] != n_kv : v.ne[1] != D || v.ne[0] < n_kv) || v.ne[2] != Hkv || Hkv <= 0 || H % Hkv || k.ne[3] != B || v.ne[3] != B) return CLLM_E_UNSUPPORTED;
    if (ktype != CLLM_TYPE_F16 && ktype != CLLM_TYPE_Q8_0) return CLLM_E_UNSUPPORTED;
    if (vl == 1 && ktype != CLLM_TYPE_F16) return CLLM_E_UNSUPPORTED;
    if (N <= 0 || n_kv <= 0 || N > (1 << 24) || n_kv > (1 << 30) || H > 65535 || B > 65535) return CLLM_E_UNSUPPORTED;
    if (q.nb[0] != 4 || (((uintptr_t) q.data | (uintptr_t) q.nb[1] | (uintptr_t) q.nb[2] | (uintptr_t) q.nb[3]) & 15)) return CLLM_E_UNSUPPORTED;
    if ((((uintptr_t) dst | (uintptr_t) nbn | (uintptr_t) nbh | (uintptr_t) nbb) & 15)) return CLLM_E_UNSUPPORTED;
    if (ktype == CLLM_TYPE_F16) {
        if ((((uintptr_t) k.data | (uintptr_t) k.nb[1] | (uintptr_t) k.nb[2] | (uintptr_t) k.nb[3]) & 15)) return CLLM_E_UNSUPPORTED;
        if ((((uintptr_t) v.data | (uintptr_t) v.nb[1] | (uintptr_t) v.nb[2] | (uintptr_t) v.nb[3]) & 15)) return CLLM_E_UNSUPPORTED;
    } else {
        if ((((uintptr_t) k.data | (uintptr_t) k.nb[1] | (uintptr_t) k.nb[2] | (uintptr_t) k.nb[3] | (uintptr_t) v.data | (uintptr_t) v.nb[1] | (uintptr_t) v.nb[2] | (uintptr_t) v.nb[3]) & 1)) return CLLM_E_UNSUPPORTED;
    }
    fattn_args a;
    a.q = q.data; a.q_nb1 = q.nb[1]; a.q_nb2 = q.nb[2]; a.q_nb3 = q.nb[3];
    a.k = k.data; a.k_nb1 = k.nb[1]; a.k_nb2 = k.nb[2]; a.k_nb3 = k.nb[3];
    a.v = v.data; a.v_nb1 = v.nb[1]; a.v_nb2 = v.nb[2]; a.v_nb3 = v.nb[3];
    a.mask = nullptr; a.m_nb1 = a.m_nb2 = a.m_nb3 = 0; a.m_ne2 = a.m_ne3 = 1; a.m_al = 0;
    int mmode = 0;
    if (mask) {
        if (mask->nb[0] != 2 || mask->ne[0] < n_kv || mask->ne[1] < N || ((uintptr_t) mask->data & 1)) return CLLM_E_UNSUPPORTED;
        a.mask = mask->data; a.m_nb1 = mask->nb[1]; a.m_nb2 = mask->nb[2]; a.m_nb3 = mask->nb[3]; a.m_ne2 = (int) mask->ne[2]; a.m_ne3 = (int) mask->ne[3];
        a.m_al = n_kv % 4 == 0 && (((uintptr_t) mask->data | (uintptr_t) mask->nb[1] | (uintptr_t) mask->nb[2] | (uintptr_t) mask->nb[3]) & 7) == 0;
        mmode = 2;
    } else if (causal_past >= 0) mmode = 1;
    a.dst = dst; a.d_nbn = nbn; a.d_nbh = nbh; a.d_nbb = nbb;
    a.N = (int) N; a.H = (int) H; a.Hkv = (int) Hkv; a.n_kv = (int) n_kv; a.n_past = causal_past; a.sc2 = scale * FA_LOG2E; a.cap_in = 0.0f;
    if (cap != 0.0f) { a.cap_in = scale / cap; a.sc2 = cap * FA_LOG2E; }      // the kernel's scores are tanh(s cap_in): their scale is the cap
    const int r = (int)(H / Hkv);
    const bool decode = N * r <= 32;
    a.R = decode ? r : 1;
    a.splits = 1; a.chunk = (int)((n_kv + 63) / 64 * 64); a.part = nullptr; a.n_kv_dev = nullptr;
    if (decode && n_kv > 64) {
        const int tiles = (int)((n_kv + 63) / 64);      // ~2 workgroups per CU, each walking `per` tiles with the next tile's loads in flight
        static const int div = opt_int(OPT_CLLM_FA_DIV);
        int per = tiles / div; if (per < 1) per = 1; if (per < (tiles + FA_MAX_SPLITS - 1) / FA_MAX_SPLITS) per = (tiles + FA_MAX_SPLITS - 1) / FA_MAX_SPLITS;
        a.chunk = per * 64; a.splits = (tiles + per - 1) / per;
        if (a.splits > 1 && !wdata) { a.splits = 1; a.chunk = (int)((n_kv + 63) / 64 * 64); }      // a caller without scratch (cllm_op_attn_prefill): one workgroup walks the whole cache
        if (a.splits > 1) {
            if (wsize < (size_t) B * H * N * a.splits * (D + 4) * 4 || ((uintptr_t) wdata & 15)) FAIL(CLLM_E_INVALID, "flash_attn_ext: wdata too small");
            a.part = (float *) wdata;
        }
    }
    if (vl == 1 && (v.nb[1] / 2) % 8) return CLLM_E_UNSUPPORTED;
    if (cap != 0.0f) return fattn_cap_launch(st, a, (int) D, ktype, mmode, (int) B, decode);
    if (hs) return fattn_hs_launch(st, a, (int) D, ktype, mmode, (int) B, decode);
    if (pad) return fattn_pad_launch(st, a, (int) D, ktype, mmode, (int) B, decode);
    if (D == 128) return fattn_dispatch<128>(st, a, ktype, vl, mmode, (int) B, decode);
    return fattn_dispatch<64>(st, a, ktype, vl, mmode, (int) B, decode);
}

// ---- single-token attention above attn_long_threshold() cached positions inside a captured decode step (the runner's graph, the module's
//      launch list): RoPE of q and k + both cache writes in one small launch (the same arithmetic as k_attn_dec: bit-identical cache contents),
//      then the split-KV flash kernel with the number of positions read on the device, then the merge.  Tolerance tier (like attn_long.hip, which
//      it replaces unless CLLM_ATTN_LONG_FLASH=0): ~2x faster at 4K-16K positions.
template <int HD, int MODE>
__global__ void __launch_bounds__(HD) k_rope_kv_prep(const float * __restrict__ qkv, const int32_t * __restrict__ pos_dev, const float * __restrict__ rope_cs, int nh, int nkv,
                                                     uint16_t * __restrict__ k_cache, uint16_t * __restrict__ v_cache, int ML, float * __restrict__ qrot) {
    constexpr int half = HD / 2, off = rope_pair(MODE, 0, half).off;
    const int tid = threadIdx.x, blk = blockIdx.x, pos = pos_dev[0], KD = nkv * HD, QD = nh * HD;
    const bool is_q = blk < nh;
    const int g = blk - nh;
    const float * x = is_q ? qkv + blk * HD : qkv + QD + g * HD;
    if (tid < half) {
        const int ic = rope_pair(MODE, tid, half).ic;
        const float x0 = x[ic], x1 = x[ic + off], c = rope_cs[2 * tid], sn = rope_cs[2 * tid + 1];
        const float y0 = rope_rot_a(x0, x1, c, sn), y1 = rope_rot_b(x0, x1, c, sn);
        if (is_q) { qrot[blk * HD + ic] = y0; qrot[blk * HD + ic + off] = y1; }
        else { *k_slot(k_cache, pos, KD, g, HD, ic) = f2h(y0); *k_slot(k_cache, pos, KD, g, HD, ic + off) = f2h(y1); }
    }
    if (!is_q) *v_slot(v_cache, g, HD, tid, ML, pos) = f2h(qkv[QD + KD + g * HD + tid]);
}

int launch_attn_long_flash(hipStream_t st, const float * qkv, const int32_t * pos_dev, const float * rope_cs, int nh, int nkv, int hd, int mode,
                           uint16_t * k_cache, uint16_t * v_cache, int64_t ML, float * S, size_t s_bytes, float * att) {
    // opt-in (CLLM_ATTN_LONG_FLASH=1): this form keeps the flash kernel's own summation order (tolerance tier); the default beyond attn_long_threshold() is
    // attn_long.hip, which accumulates in the reference's order
    static const bool on = opt_int(OPT_CLLM_ATTN_LONG_FLASH) == 1;
    if (!on || !rope_cs || (hd != 64 && hd != 128) || nkv <= 0 || nh % nkv || (int64_t) nh / nkv > 32 || ML % 8 || ML > (1 << 30) || ((uintptr_t) S & 15)) return CLLM_E_UNSUPPORTED;
    const size_t q_bytes = ((size_t) nh * hd * 4 + 255) & ~(size_t) 255;
    if (s_bytes <= q_bytes) return CLLM_E_UNSUPPORTED;
    int max_splits = (int)((s_bytes - q_bytes) / ((size_t) nh * (hd + 4) * 4));
    if (max_splits > FA_MAX_SPLITS) max_splits = FA_MAX_SPLITS;
    if (max_splits < 4) return CLLM_E_UNSUPPORTED;
    float * qrot = S;
    const int rc = with_head_dim(hd, [&](auto hd_c) { return with_rope_mode(mode, [&](auto mode_c) -> int {
        constexpr int HD = decltype(hd_c)::value;
        hipLaunchKernelGGL((k_rope_kv_prep<HD, decltype(mode_c)::value>), dim3(nh + nkv), dim3(HD), 0, st, qkv, pos_dev, rope_cs, nh, nkv, k_cache, v_cache, (int) ML, qrot);
        LAUNCH_CHECK();
        return CLLM_OK;
    }); });
    if (rc) return rc;
    const int KD = nkv * hd;
    fattn_args a;
    a.q = (const char *) qrot; a.q_nb1 = (int64_t) nh * hd * 4; a.q_nb2 = (int64_t) hd * 4; a.q_nb3 = a.q_nb1;
    a.k = (const char *) k_cache; a.k_nb1 = (int64_t) KD * 2; a.k_nb2 = (int64_t) hd * 2; a.k_nb3 = a.k_nb1 * ML;
    a.v = (const char *) v_cache; a.v_nb1 = ML * 2; a.v_nb2 = ML * hd * 2; a.v_nb3 = a.v_nb2 * nkv;
    a.mask = nullptr; a.m_nb1 = a.m_nb2 = a.m_nb3 = 0; a.m_ne2 = a.m_ne3 = 1; a.m_al = 0;
    a.dst = (char *) att; a.d_nbn = (int64_t) nh * hd * 4; a.d_nbh = (int64_t) hd * 4; a.d_nbb = a.d_nbn;
    a.part = (float *)((char *) S + q_bytes);
    a.N = 1; a.H = nh; a.Hkv = nkv; a.R = nh / nkv; a.n_kv = (int) ML; a.n_past = -1; a.sc2 = (1.0f / sqrtf((float) hd)) * FA_LOG2E; a.cap_in = 0.0f;
    a.n_kv_dev = pos_dev;
    const int tiles = (int)((ML + 63) / 64);
    int per = (tiles + max_splits - 1) / max_splits; if (per < tiles / 32) per = tiles / 32; if (per < 1) per = 1;
    a.chunk = per * 64; a.splits = (tiles + per - 1) / per;
    const dim3 grid((unsigned) a.splits, (unsigned) nkv, 1);
    return with_head_dim(hd, [&](auto hd_c) -> int {
        constexpr int HD = decltype(hd_c)::value;
        hipLaunchKernelGGL((k_fattn<HD, CLLM_TYPE_F16, 1, 0>), grid, dim3(256), fa_lds_bytes<HD>(), st, a);
        LAUNCH_CHECK();
        hipLaunchKernelGGL((k_fattn_merge<HD>), dim3(1, (unsigned) nh, 1), dim3(1024), 0, st, a);
        LAUNCH_CHECK();
        return CLLM_OK;
    });
}
