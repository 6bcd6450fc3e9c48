#pragma once
// gemv_act.h -- the activation prologue of k_gemv_rows and k_gemv_rows32, defined once (device code): gemv_act_load / gemv_act_store are sections (1) and (3) of those
// kernels, gemv_hsum8 / gemv_bias_resid the end of a unit of rows (k_gemv_team32 uses the sum).  k_gemv_dec's generic branch and k_gemv_team32 keep their own text of the
// same prologue: with this one they measured slower per launch than the parent's spread allows (profiles/gemv_row_kernels_shared.txt, section 5)
#include "common.h"
#include "quant_dev.h"

// PRO 1 / 5: (v * scale) * g;  PRO 3: v, g = (g0, u0, g1, u1), (g2, u2, g3, u3) -> SiLU(g_i) * u_i;  PRO 4: SiLU(v) * g;  PRO 2: v.
// e: index of v.x, nv: ggml_vec_silu_f32's polynomial body lies below it, the libm tail behind
template <int PRO>
__device__ __forceinline__ f32x4 gemv_act_group(f32x4 v, const f32x4 g, float scale, int e, int nv) {
    if (PRO == 3) {
        const f32x4 p0 = v, p1 = g;
        v.x = silu_any(p0.x, e + 0 < nv) * p0.y; v.y = silu_any(p0.z, e + 1 < nv) * p0.w;
        v.z = silu_any(p1.x, e + 2 < nv) * p1.y; v.w = silu_any(p1.z, e + 3 < nv) * p1.w;
    }
    if (PRO == 4) { v.x = silu_any(v.x, e + 0 < nv) * g.x; v.y = silu_any(v.y, e + 1 < nv) * g.y; v.z = silu_any(v.z, e + 2 < nv) * g.z; v.w = silu_any(v.w, e + 3 < nv) * g.w; }
    if (PRO == 1 || PRO == 5) { v.x = (v.x * scale) * g.x; v.y = (v.y * scale) * g.y; v.z = (v.z * scale) * g.z; v.w = (v.w * scale) * g.w; }
    return v;
}

// (1) this thread's activation groups (values e0 + 4096 u ..+3; past the row's end: group 0 again, never used).  Call it before the weight requests go out
template <int PRO, int NPRE>
__device__ __forceinline__ void gemv_act_load(f32x4 (&vv)[NPRE], f32x4 (&gg)[NPRE], const float * px, const float * pw, int K, int e0) {
    const float * gp = (PRO == 1 || PRO == 4) ? pw : PRO == 3 ? px + 4 : px;
    constexpr int vmul = PRO == 3 ? 2 : 1;
#pragma unroll
    for (int u = 0; u < NPRE; u++) {
        const int e = e0 + u * 4096, ec = e < K ? e : 0;
        vv[u] = *(const f32x4 *)(px + ec * vmul);
        if (PRO != 2) gg[u] = *(const f32x4 *)(gp + ec * vmul);
    }
}

// (3) the activation row: [RMS_NORM * weight | SiLU * up |] quantize -> LDS (act layout of common.h; Q81: the Q8_1 flavour).  C0: behind the row, Q4_0's plane
// c0[block][AVX lane] = (-8, -8, -8, -8) . a  ((nib - 8) . a = nib . a + c0).  part: the kernel's own __shared__ double[16] (PRO 1).  The caller's barrier follows
template <int KIND, bool Q81, bool C0, int PRO, int NPRE>
__device__ __forceinline__ void gemv_act_store(char * lds, const f32x4 (&vv)[NPRE], const f32x4 (&gg)[NPRE], const float * px, int K, float eps, int e0, int lane, double * part) {
    float scale = 1.0f;
    if (PRO == 1) {
        const double sum = NPRE == 1 ? rms_block_sumsq_1024_one(vv[0], e0 < K, part) : rms_block_sumsq_1024(px, K, vv[0], part);
        scale = rms_scale(sum, K, eps, px, nullptr, part);
    }
    const int nv = K & ~7;
#pragma unroll
    for (int u = 0; u < NPRE; u++) {
        const int e = e0 + u * 4096;
        if (e < K) {
            quant4_store<KIND, Q81>(lds, K, e, lane, gemv_act_group<PRO>(vv[u], gg[u], scale, e, nv));
            if (C0) *(int *)(lds + (unsigned) act_row_bytes(K, Q81 ? ACT_Q8_1 : ACT_Q8_0) + e) = dot4(0xf8f8f8f8u, *(const uint32_t *)(lds + e), 0);
        }
    }
}

// hsum_float_8 over the 8 slots [A0 A4 A2 A6 | A1 A5 A3 A7] of a row (neighbour exchanges)
__device__ __forceinline__ float gemv_hsum8(float h) { h = h + dpp_f<DPP_QUAD_XOR1>(h); h = h + dpp_f<DPP_QUAD_XOR2>(h); return h + dpp_f<DPP_HALF_MIRROR>(h); }

// v + bias[row] + resid[row] for row r of a unit of RPW rows starting at row0: the unit's values come through the scalar cache (their own counter, no wait on the weight stream)
template <int RPW>
__device__ __forceinline__ float gemv_bias_resid(float v, const float * bias, const float * resid, size_t row0, int r) {
    float bsel = 0.0f, rsel = 0.0f;
#pragma unroll
    for (int q = 0; q < RPW; q++) {
        if (bias)  { const float x = uniform_load_f32(bias  + row0 + q); bsel = r == q ? x : bsel; }
        if (resid) { const float x = uniform_load_f32(resid + row0 + q); rsel = r == q ? x : rsel; }
    }
    if (bias)  v = v + bsel;
    if (resid) v = v + rsel;
    return v;
}
