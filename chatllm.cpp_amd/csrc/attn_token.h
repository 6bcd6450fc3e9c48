// attn_token.h -- the steps the exact (bit-identical) single-token attention kernels share, each stated once: k_attn_decode / k_attn_dec
// (decode_fused.hip), the four kernels of attn_long.hip, k_rope_kv_prep (fattn.hip) and, for the reduce tree, k_mul_mat_f_vd (matmul_f.hip).
// These kernels agree with each other and with libggml-cpu.so bit for bit BECAUSE they take the steps below from here.  Device code only.
#pragma once
#include "common.h"
#include "q4k.h"

// per-workgroup time stamps of the tools (tools/attn_phase_probe.py, tools/attn_long_probe.py): `ts` is the kernel's stamp buffer, nullptr outside the tools
#define TS(k) do { if (ts && threadIdx.x == 0) ts[(blockIdx.y * gridDim.x + blockIdx.x) * 8 + (k)] = wall_clock64(); } while (0)

// GGML_F32x8_REDUCE (simd-mappings.h:545-560) over the 32 accumulators of ggml_vec_dot_f16, held two per lane by 16 lanes (accumulator
// a = 8 j + l in lane a / 2): x0 += x2, x1 += x3 (lanes c ^ 8); x0 += x1 (c ^ 4); lo + hi halves (c ^ 2); hadd, hadd (in-lane, c ^ 1)
__device__ __forceinline__ float vd32_reduce(float a0, float a1) {
    a0 = a0 + dpp_f<DPP_ROW_ROR8>(a0); a1 = a1 + dpp_f<DPP_ROW_ROR8>(a1);
    a0 = a0 + lane_xor4_f(a0);         a1 = a1 + lane_xor4_f(a1);
    a0 = a0 + dpp_f<DPP_QUAD_XOR2>(a0); a1 = a1 + dpp_f<DPP_QUAD_XOR2>(a1);
    const float u = a0 + a1;
    return u + dpp_f<DPP_QUAD_XOR1>(u);
}

// The tail of a V.P row: `res` is vd32_reduce's sum over the whole chunks of 32 cached positions; the ntail = n_kv mod 32 leftovers follow one by one in double, as
// ggml_vec_dot_f16's scalar tail adds them (products rounded to fp32 first).  Lane c16 of the row's 16 lanes stages the products of leftovers 2 c16 and 2 c16 + 1
// (prod(t), t = 0, 1: the product at position (n_kv & ~31) + 2 c16 + t, evaluated only below n_kv) in the row's 32-float LDS `slot`; lane 0 adds them in order and stores *dst.
// REUSE: the caller stages another row in the same slot afterwards (the row loops of k_attn_decode / k_attn_dec), so lane 0's reads are fenced from the next row's
// stores; the long kernels own a slot per row and end behind the store: no trailing fence.
template <bool REUSE, class Prod>
__device__ __forceinline__ void vd_tail_store(float res, Prod && prod, float * slot, int c16, int ntail, float * dst) {
#pragma unroll
    for (int t = 0; t < 2; t++) if (2 * c16 + t < ntail) slot[2 * c16 + t] = prod(t);
    wave_lds_fence();
    if (c16 == 0) {
        double s = (double) res;
        for (int t = 0; t < ntail; t++) s += (double) slot[t];
        *dst = (float) s;
    }
    if (REUSE) wave_lds_fence();
}

// one chunk of a V.P chain with both operands as fp16 pairs in registers: fma((float) v, (float) p, acc) is one v_fma_mix_f32 per half (the conversions are exact:
// the cvt + fma of the other kernels bit for bit)
__device__ __forceinline__ void fma_mix_pair(float & a0, float & a1, uint32_t vw, uint32_t pw) {
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,1,0]" : "+v"(a0) : "v"(vw), "v"(pw));      // low halves
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(a1) : "v"(vw), "v"(pw));      // high halves
}

// maximum over a workgroup of 16 waves through red_f[16].  barrier(): the caller's -- lds_barrier() where global prefetches must stay in flight (k_attn_dec),
// __syncthreads() elsewhere.  red_f may be rewritten only behind the caller's next barrier.
template <class Barrier>
__device__ __forceinline__ float block_max16(float mx, float * red_f, int lane, int wave, Barrier && barrier) {
    mx = wave_max(mx);
    if (lane == 0) red_f[wave] = mx;
    barrier();
    mx = red_f[0];
#pragma unroll
    for (int w = 1; w < 16; w++) mx = fmaxf(mx, red_f[w]);
    return mx;
}

// the new token's q / k pair (x0, x1) = elements (ic, ic + off) of its head: rotated, rounded to fp16 (q: src1 of K.Q is rounded to fp16; k: the cache is fp16)
__device__ __forceinline__ void token_rope_round(float x0, float x1, int ic, int off, float c, float s, float * out) {
    out[ic] = h2f(f2h(rope_rot_a(x0, x1, c, s))); out[ic + off] = h2f(f2h(rope_rot_b(x0, x1, c, s)));
}

// THE cache layouts: K rows by position [pos][kv head g][d]; V transposed, rows by element [kv head g][d][pos] with max_len ML positions per row
template <class T> __device__ __forceinline__ T * k_slot(T * k_cache, int pos, int KD, int g, int HD, int d) { return k_cache + (int64_t) pos * KD + g * HD + d; }
template <class T> __device__ __forceinline__ T * v_slot(T * v_cache, int g, int HD, int d, int64_t ML, int pos) { return v_cache + ((int64_t) g * HD + d) * ML + pos; }

// SOFT_MAX of one head's row for the long forms, by a workgroup of 1024 threads: sc[0 .. n_kv) (LDS, 16-byte aligned) holds the scores and `mx` the maximum over this
// thread's share of them.  Every wave exponentiates (sc <- the exponentials, gsum[] <- the float sum of every group of 8: 16-byte LDS accesses, the 32-byte lane
// stride is 8-way conflicted for dwords); ONE wave then adds the group sums in k_soft_max's order (lane l owns groups l, l + 64, ...; double; DPP tree) and
// exponentiates the n_kv mod 8 leftovers -> the node kernel's bits.  Returns 1 / total in every thread; sc is complete behind it.
__device__ __forceinline__ float long_soft_max(float mx, float * sc, float * gsum, int n_kv, float * red_f, double * red_d, int tid, int lane, int wave) {
    const int nv = n_kv & ~7;
    mx = block_max16(mx, red_f, lane, wave, [] { __syncthreads(); });
    for (int gi = tid * 8; gi < nv; gi += 1024 * 8) {
        const f32x4 s0 = *(const f32x4 *)(sc + gi), s1 = *(const f32x4 *)(sc + gi + 4);
        float e[8] = { ggml_expf_poly(s0.x - mx), ggml_expf_poly(s0.y - mx), ggml_expf_poly(s0.z - mx), ggml_expf_poly(s0.w - mx),
                       ggml_expf_poly(s1.x - mx), ggml_expf_poly(s1.y - mx), ggml_expf_poly(s1.z - mx), ggml_expf_poly(s1.w - mx) };
        *(f32x4 *)(sc + gi) = f32x4{e[0], e[1], e[2], e[3]}; *(f32x4 *)(sc + gi + 4) = f32x4{e[4], e[5], e[6], e[7]};
        gsum[gi >> 3] = soft_group8_sum(e);
    }
    __syncthreads();
    if (wave == 0) {
        const double rinv = soft_total_rinv_groups(gsum, nv >> 3, sc, nv, n_kv, mx, n_kv >> 3, lane);
        if (lane == 0) red_d[0] = rinv;
    }
    __syncthreads();
    return (float) red_d[0];
}
