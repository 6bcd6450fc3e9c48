// ops.hip -- the non-matmul nodes of one chatllm.cpp forward graph, written for gfx950.
// Each kernel cites the reference CPU function whose arithmetic (operation order, rounding points,
// accumulation width) it reproduces; see include/chatllm_hip.h for the op contracts.
// What the kernels and entries share is stated once: a row's or an element's coordinates and their address (t_row_coord, t_elem_coord, t_at), the 1-D grid (grid_1d)
// and the norms' store tail (map4, rms_store4) in common.h; the row-wise entries' argument checks in row_op_args below.
#include "common.h"
#include "quant_dev.h"

#include <float.h>
#include <math.h>
#include <mutex>
#include <vector>

// The argument checks of the row-wise entries (src and dst of one shape, F32 rows), in the order every one of them has them; `checks` names the steps to run.
// A row with nb[0] != 4 is CLLM_E_INVALID "shape" to RMS_NORM, SOFT_MAX and ROPE and CLLM_E_UNSUPPORTED to the norms that came after them: both stay as callers rely on them.
// An empty tensor passes the row limit: it is no launch, and its entry returns CLLM_OK.
enum { ROW_F32_SHAPE = 1, ROW_DENSE_INVALID = 2, ROW_DENSE_UNSUPPORTED = 4, ROW_LIMIT = 8 };
static int row_op_args(const char * op, const cllm_tensor * src, const cllm_tensor * dst, int checks) {
    if (checks & ROW_F32_SHAPE) {
        if (!src || !dst) FAIL(CLLM_E_INVALID, "%s: null", op);
        if (src->type != CLLM_TYPE_F32 || dst->type != CLLM_TYPE_F32) FAIL(CLLM_E_UNSUPPORTED, "%s: type (F32 only)", op);
        if (!t_same_shape(src, dst)) FAIL(CLLM_E_INVALID, "%s: shape", op);
    }
    if ((checks & (ROW_DENSE_INVALID | ROW_DENSE_UNSUPPORTED)) && (src->nb[0] != 4 || dst->nb[0] != 4)) {
        if (checks & ROW_DENSE_INVALID) FAIL(CLLM_E_INVALID, "%s: shape", op);
        FAIL(CLLM_E_UNSUPPORTED, "%s: rows must be dense", op);
    }
    if ((checks & ROW_LIMIT) && src->ne[0] != 0 && t_nrows(src) > 0x7fffffff) FAIL(CLLM_E_UNSUPPORTED, "%s: more than 2^31 - 1 rows", op);
    return CLLM_OK;
}

// ================================================================================================
// RMS_NORM (+ MUL)      ggml_compute_forward_rms_norm_f32, ggml-cpu/ops.cpp:3710-3759
//   sum of x*x in double, mean -> float, scale = 1/sqrtf(mean+eps), y = x*scale   [, y *= w as a second rounding]
// one workgroup per row; HBM/L2-bound, float4 traffic.
// ================================================================================================
template <bool MUL>
__global__ void __launch_bounds__(1024) k_rms_norm(tview s, tview d, const float * __restrict__ w, int64_t w_ne0, float eps) {
    const tcoord c = t_row_coord(s, blockIdx.x);
    const float * x = (const float *) t_at(s, c);
    float *       y = (float *) t_at(d, c);
    const int64_t n = s.ne[0];
    __shared__ double part[16];
    const bool aligned = (((uintptr_t) x) & 15) == 0;
    const f32x4 first = (int64_t) threadIdx.x < (n >> 2) ? rms_load4(x, threadIdx.x, aligned) : f32x4{0, 0, 0, 0};
    const double sum = rms_block_sumsq_1024(x, n, first, part);
    const float scale = rms_scale(sum, n, eps, x, nullptr, part);
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        float v = x[i] * scale;
        if (MUL) v = v * w[i % w_ne0];
        y[i] = v;
    }
}

static int rms_norm_impl(void * stream, const cllm_tensor * src, const cllm_tensor * weight, cllm_tensor * dst, float eps) {
    if (const int rc = row_op_args("rms_norm", src, dst, ROW_F32_SHAPE | ROW_DENSE_INVALID)) return rc;
    if (weight && (weight->type != CLLM_TYPE_F32 || weight->nb[0] != 4 || weight->ne[0] != src->ne[0] || t_nrows(weight) != 1))
        FAIL(CLLM_E_UNSUPPORTED, "rms_norm_mul: weight must be a dense F32 [ne0] vector");
    const int64_t rows = t_nrows(src);
    if (rows == 0 || src->ne[0] == 0) return CLLM_OK;
    hipStream_t st = (hipStream_t) stream;
    if (weight) hipLaunchKernelGGL(k_rms_norm<true>,  dim3((unsigned) rows), dim3(1024), 0, st, tv(src), tv(dst), (const float *) weight->data, weight->ne[0], eps);
    else        hipLaunchKernelGGL(k_rms_norm<false>, dim3((unsigned) rows), dim3(1024), 0, st, tv(src), tv(dst), (const float *) nullptr, (int64_t) 1, eps);
    LAUNCH_CHECK();
    return CLLM_OK;
}
extern "C" int cllm_op_rms_norm(void * stream, const cllm_tensor * src, cllm_tensor * dst, float eps) { return rms_norm_impl(stream, src, nullptr, dst, eps); }
extern "C" int cllm_op_rms_norm_mul(void * stream, const cllm_tensor * src, const cllm_tensor * weight, cllm_tensor * dst, float eps) {
    if (!weight) FAIL(CLLM_E_INVALID, "rms_norm_mul: null weight");
    return rms_norm_impl(stream, src, weight, dst, eps);
}

// ================================================================================================
// NORM        ggml_compute_forward_norm_f32, ggml-cpu/ops.cpp:3643-3688 (LayerNorm before its affine: MUL and ADD stay nodes of their own)
//   sum of x in double, mean -> float; the centred squares in float groups of 8, their sum in double, variance -> float;
//   scale = 1/sqrtf(variance+eps), y = (x - mean) * scale.  The arithmetic and its order: norm_order.h; the workgroup's trees and fallbacks: common.h.
// one workgroup per row, three passes over the row (the second and third hit the cache; a thread's first group of 8 stays in registers); float4 traffic where
// the row start is 16-byte aligned.  dst may be src: every store comes after the last barrier of norm_variance, behind every read of the two sums.
// ================================================================================================
__global__ void __launch_bounds__(1024) k_norm(tview s, tview d, float eps) {
    const tcoord c = t_row_coord(s, blockIdx.x);
    const float * x = (const float *) t_at(s, c);
    float *       y = (float *) t_at(d, c);
    const int64_t n = s.ne[0], ng = n >> 3;
    const int tid = threadIdx.x;
    __shared__ double part[3][16];
    __shared__ double slot[2];
    const bool aligned = (((uintptr_t) x) & 15) == 0, y_aligned = (((uintptr_t) y) & 15) == 0;
    const norm_g8 first = tid < ng ? norm_load8(x, tid, aligned) : norm_g8{ f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0} };
    double S, A;
    norm_block_sum_1024(x, n, aligned, first, part[0], part[1], S, A);
    const float mean = norm_mean(S, A, n, x, &slot[0]);
    const double V = norm_block_var_sum_1024(x, n, aligned, first, mean, part[2]);
    const float scale = nm_scale(norm_variance(V, n, mean, x, &slot[1]), eps);
    const auto out = [&](float e) { return nm_out(e, mean, scale); };
    norm_g8 v = first;
    for (int64_t g = tid; g < ng; g += 1024) {
        if (g != tid) v = norm_load8(x, g, aligned);
        const f32x4 lo = map4(v.lo, out), hi = map4(v.hi, out);
        rms_store4(y, 2 * g, y_aligned, lo); rms_store4(y, 2 * g + 1, y_aligned, hi);
    }
    if (8 * ng + tid < n) y[8 * ng + tid] = out(x[8 * ng + tid]);
}

extern "C" int cllm_op_norm(void * stream, const cllm_tensor * src, cllm_tensor * dst, float eps) {
    if (const int rc = row_op_args("norm", src, dst, ROW_F32_SHAPE)) return rc;
    if (!(eps >= 0.0f)) FAIL(CLLM_E_INVALID, "norm: eps must be >= 0");             // (NaN included) the reference asserts eps >= 0, ops.cpp:3661; an unusable eps is reported before a row that is not dense
    if (const int rc = row_op_args("norm", src, dst, ROW_DENSE_UNSUPPORTED | ROW_LIMIT)) return rc;
    const int64_t rows = t_nrows(src);
    if (rows == 0 || src->ne[0] == 0) return CLLM_OK;
    hipLaunchKernelGGL(k_norm, dim3((unsigned) rows), dim3(1024), 0, (hipStream_t) stream, tv(src), tv(dst), eps);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// ================================================================================================
// L2_NORM     ggml_compute_forward_l2_norm_f32, ggml-cpu/ops.cpp:4051-4092 (ggml::norm_p2: the query and key of a gated delta net's linear attention, per head)
//   sum of x*x in double, scale = 1/fmaxf(sqrtf((float) sum), eps), y = x*scale.  The arithmetic and its order: norm_order.h; the trees and fallbacks: common.h.
// Two launch shapes.  Rows longer than L2_WAVE_ROW_MAX: k_rms_norm's shape, one 1024-thread workgroup per row.  Shorter rows (128 per head, heads x tokens of them): one
// wave per row, four rows per 256-thread workgroup, the row in registers between the sum and the store, no barrier and no LDS anywhere (the interval test's outcome
// differs from wave to wave).  dst may be src in both: a row is stored by those who summed it, behind the last barrier (workgroup) or by the same wave (wave per row).
// ================================================================================================
static constexpr int64_t L2_WAVE_ROW_MAX = 512;       // the longest row the wave-per-row shape takes (8 elements per lane and a leftover): DESIGN.md has the measurement
static constexpr int     L2_WAVE_ROWS    = 4;         // rows (waves) per workgroup of that shape

__global__ void __launch_bounds__(1024) k_l2_norm(tview s, tview d, float eps) {
    const tcoord c = t_row_coord(s, blockIdx.x);
    const float * x = (const float *) t_at(s, c);
    float *       y = (float *) t_at(d, c);
    const int64_t n = s.ne[0], nq = n >> 2;
    const int tid = threadIdx.x;
    __shared__ double part[16];
    const bool aligned = (((uintptr_t) x) & 15) == 0, y_aligned = (((uintptr_t) y) & 15) == 0;
    const f32x4 first = tid < nq ? rms_load4(x, tid, aligned) : f32x4{0, 0, 0, 0};
    const double sum = rms_block_sumsq_1024(x, n, first, part);
    const float scale = l2_block_scale(sum, n, eps, x, part);
    const auto out = [&](float e) { return nm_l2_out(e, scale); };
    f32x4 v = first;
    for (int64_t q = tid; q < nq; q += 1024) {
        if (q != tid) v = rms_load4(x, q, aligned);
        rms_store4(y, q, y_aligned, map4(v, out));
    }
    if (4 * nq + tid < n) y[4 * nq + tid] = out(x[4 * nq + tid]);
}

__global__ void __launch_bounds__(64 * L2_WAVE_ROWS) k_l2_norm_wave(tview s, tview d, int64_t rows, float eps) {
    const int64_t row = (int64_t) blockIdx.x * L2_WAVE_ROWS + (threadIdx.x >> 6);
    if (row >= rows) return;                                    // a wave past the last row: nothing below waits for it
    const tcoord c = t_row_coord(s, row);
    const float * x = (const float *) t_at(s, c);
    float *       y = (float *) t_at(d, c);
    const int64_t n = s.ne[0];
    const int lane = threadIdx.x & 63, nq = (int)(n >> 2);
    const bool y_aligned = (((uintptr_t) y) & 15) == 0;
    const l2_wave_row r = l2_wave_load(x, n, (((uintptr_t) x) & 15) == 0);
    const float scale = l2_wave_scale(r, n, eps, x);
    const auto out = [&](float e) { return nm_l2_out(e, scale); };
    if (lane < nq)      rms_store4(y, lane, y_aligned, map4(r.v0, out));
    if (lane + 64 < nq) rms_store4(y, lane + 64, y_aligned, map4(r.v1, out));
    if (4 * nq + lane < n) y[4 * nq + lane] = out(r.t);
}

extern "C" int cllm_op_l2_norm(void * stream, const cllm_tensor * src, cllm_tensor * dst, float eps) {
    if (const int rc = row_op_args("l2_norm", src, dst, ROW_F32_SHAPE | ROW_DENSE_UNSUPPORTED)) return rc;
    if (!(eps >= 0.0f)) FAIL(CLLM_E_INVALID, "l2_norm: eps must be >= 0");          // (NaN included) the reference asserts eps >= 0, ops.cpp:4069
    if (const int rc = row_op_args("l2_norm", src, dst, ROW_LIMIT)) return rc;
    const int64_t rows = t_nrows(src);
    if (rows == 0 || src->ne[0] == 0) return CLLM_OK;
    if (src->ne[0] <= L2_WAVE_ROW_MAX)
        hipLaunchKernelGGL(k_l2_norm_wave, dim3((unsigned)((rows + L2_WAVE_ROWS - 1) / L2_WAVE_ROWS)), dim3(64 * L2_WAVE_ROWS), 0, (hipStream_t) stream, tv(src), tv(dst), rows, eps);
    else
        hipLaunchKernelGGL(k_l2_norm, dim3((unsigned) rows), dim3(1024), 0, (hipStream_t) stream, tv(src), tv(dst), eps);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// ================================================================================================
// GROUP_NORM  ggml_compute_forward_group_norm_f32, ggml-cpu/ops.cpp:3956-4029 (GroupNorm::forward before its affine: MUL and ADD by a [1, 1, C] view stay nodes of their own)
//   per (group, i03), over the group's ne01 * step rows: S in double, a chain per row and a chain over the rows; mean = (float)(S / N); the centred squares in float,
//   V in double the same way; variance = (float)(V / N); scale = 1/sqrtf(variance+eps), y = (x - mean) * scale.  The arithmetic and its order: norm_order.h; the
//   workgroup's trees and fallbacks: common.h.
// one workgroup per (group, i03), three passes over the group (S with A, V, the stores; a thread's first item stays in registers, which is the whole group where it has at
// most 1024 items); float4 traffic where a row's start is 16-byte aligned, decided per row on either side.  dst may be src (group_norm_inplace is what the host uses):
// every store comes after the last barrier of gn_variance, behind every read of both sums and of both fallbacks.
// ================================================================================================
__global__ void __launch_bounds__(1024) k_group_norm(tview s, tview d, int64_t cpg, int64_t groups, float eps) {
    const int64_t g = blockIdx.x % groups, i3 = blockIdx.x / groups;
    const int64_t start = g * cpg, end = start + cpg < s.ne[2] ? start + cpg : s.ne[2], step = end - start;
    if (step <= 0) return;                                      // an empty group (C = 5 in 4 groups: the last one) touches nothing; the launcher starts none
    gn_group G;
    G.x = t_at(s, tcoord{0, 0, start, i3}); G.y = t_at(d, tcoord{0, 0, start, i3});
    G.ne0 = s.ne[0]; G.ne1 = s.ne[1]; G.rows = s.ne[1] * step; G.nb1 = s.nb[1]; G.nb2 = s.nb[2]; G.dnb1 = d.nb[1]; G.dnb2 = d.nb[2];
    G.nq = G.ne0 >> 2; G.ipr = G.nq + (G.ne0 & 3); G.items = G.rows * G.ipr; G.N = G.ne0 * G.rows;
    const int tid = threadIdx.x;
    __shared__ double part[3][16];
    __shared__ double slot[2];
    const gn_item first = tid < G.items ? gn_load(G, tid) : gn_item{ f32x4{0, 0, 0, 0}, 1, 0, 0 };
    double S, A;
    gn_block_sum_1024(G, first, part[0], part[1], S, A);
    const float mean = gn_mean(S, A, G, &slot[0]);
    const double V = gn_block_var_sum_1024(G, first, mean, part[2]);
    const float scale = nm_scale(gn_variance(V, mean, G, &slot[1]), eps);
    const auto out = [&](float e) { return nm_out(e, mean, scale); };
    gn_item it = first;
    for (int64_t i = tid; i < G.items; i += 1024) {
        if (i != tid) it = gn_load(G, i);
        float * yr = (float *)(G.y + (it.row % G.ne1) * G.dnb1 + (it.row / G.ne1) * G.dnb2) + it.col;
        if (it.cnt == 4) rms_store4(yr, 0, (((uintptr_t) yr) & 15) == 0, map4(it.v, out));
        else yr[0] = out(it.v.x);
    }
}

extern "C" int cllm_op_group_norm(void * stream, const cllm_tensor * src, cllm_tensor * dst, int n_groups, float eps) {
    if (const int rc = row_op_args("group_norm", src, dst, ROW_F32_SHAPE | ROW_DENSE_UNSUPPORTED)) return rc;
    if (n_groups <= 0) FAIL(CLLM_E_INVALID, "group_norm: n_groups must be > 0");
    if (src->ne[2] > 0x7fffffff || src->ne[3] > 0x7fffffff || src->ne[2] * src->ne[3] > 0x7fffffff) FAIL(CLLM_E_UNSUPPORTED, "group_norm: more than 2^31 - 1 (channel, batch) pairs");
    if (t_nrows(src) == 0 || src->ne[0] == 0) return CLLM_OK;
    const int64_t C = src->ne[2], cpg = nm_gn_channels_per_group(C, n_groups), groups = (C + cpg - 1) / cpg;      // (the groups that hold a channel: the others are empty)
    hipLaunchKernelGGL(k_group_norm, dim3((unsigned)(groups * src->ne[3])), dim3(1024), 0, (hipStream_t) stream, tv(src), tv(dst), cpg, groups, eps);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// ================================================================================================
// ROPE        ggml_compute_forward_rope_flt<float>, ggml-cpu/ops.cpp:5589-5865
//   theta_i built by ITERATED fp32 multiplication (rope_theta, common.h), cos/sin per (token, pair),
//   YaRN mixing (rope_yarn :5596-5611).  One workgroup per token: the first n_dims/2 threads build
//   the cos/sin cache in LDS, then all threads rotate that token's heads.  In-place safe.
// ================================================================================================
struct rope_k_params { int n_dims, mode; float theta_scale, freq_scale, ext_factor, attn_factor, corr0, corr1, mscale_yarn; };

__global__ void __launch_bounds__(256) k_rope(tview s, tview d, const int32_t * __restrict__ pos, const float * __restrict__ ff, rope_k_params p) {
    extern __shared__ float cache[];                 // [n_dims]: cos, sin interleaved
    const int64_t i2 = blockIdx.x % s.ne[2], i3 = blockIdx.x / s.ne[2];
    const int half = p.n_dims / 2;
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
        const float theta = rope_theta(pos[i2], i, p.theta_scale);
        const float f = ff ? ff[i] : 1.0f;
        const float theta_extrap = theta / f;
        const float theta_interp = p.freq_scale * theta_extrap;
        float th = theta_interp, mscale = p.attn_factor;
        if (p.ext_factor != 0.0f) {
            const float y = ((float) i - p.corr0) / fmaxf(0.001f, p.corr1 - p.corr0);      // i == i0/2
            const float ramp = (1.0f - fminf(1.0f, fmaxf(0.0f, y))) * p.ext_factor;
            th = __builtin_fmaf(theta_interp, 1 - ramp, theta_extrap * ramp);      // (gcc contracts the reference's statement into this fma: oracle rope_yarn)
            mscale = p.mscale_yarn;                                                // attn_factor * fma(0.1f, logf(1 / freq_scale), 1.0f): the host's libm (launcher)
        }
        float cs, sn;
        rope_cos_sin(th, &cs, &sn);
        cache[2*i]     = cs * mscale;
        cache[2*i + 1] = sn * mscale;
    }
    __syncthreads();
    const int64_t ne0 = s.ne[0], nh = s.ne[1];
    const int64_t off = rope_pair(p.mode, 0, half).off;
    // rotated pairs
    for (int64_t t = threadIdx.x; t < nh * half; t += blockDim.x) {
        const int64_t h = t / half; const int i = (int)(t % half);
        const float * x = (const float *) t_at(s, tcoord{0, h, i2, i3});
        float *       y = (float *) t_at(d, tcoord{0, h, i2, i3});
        const int64_t ic = rope_pair(p.mode, i, half).ic;
        const float c = cache[2*i], sn = cache[2*i + 1];
        const float x0 = x[ic], x1 = x[ic + off];
        y[ic]       = rope_rot_a(x0, x1, c, sn);
        y[ic + off] = rope_rot_b(x0, x1, c, sn);
    }
    // pass-through channels
    if (p.n_dims < ne0 && s.data != d.data) {
        const int64_t rest = ne0 - p.n_dims;
        for (int64_t t = threadIdx.x; t < nh * rest; t += blockDim.x) {
            const int64_t h = t / rest, i0 = p.n_dims + t % rest;
            ((float *) t_at(d, tcoord{0, h, i2, i3}))[i0] = ((const float *) t_at(s, tcoord{0, h, i2, i3}))[i0];
        }
    }
}

static float rope_corr_dim(int n_dims, int n_ctx_orig, float n_rot, float base) {       // ggml.c ggml_rope_yarn_corr_dim
    return n_dims * logf(n_ctx_orig / (n_rot * 2 * (float) M_PI)) / (2 * logf(base));
}

extern "C" int cllm_op_rope(void * stream, const cllm_tensor * src, const cllm_tensor * pos, const cllm_tensor * freq_factors,
                            cllm_tensor * dst, const cllm_rope_params * p) {
    if (!src || !pos || !dst || !p) FAIL(CLLM_E_INVALID, "rope: null");
    if (pos->type != CLLM_TYPE_I32) FAIL(CLLM_E_UNSUPPORTED, "rope: type");
    if (p->mode != 0 && p->mode != 2) FAIL(CLLM_E_UNSUPPORTED, "rope: mode %d", p->mode);
    if (const int rc = row_op_args("rope", src, dst, ROW_F32_SHAPE | ROW_DENSE_INVALID)) return rc;
    if (p->n_dims > src->ne[0] || (p->n_dims & 1) || p->n_dims <= 0) FAIL(CLLM_E_INVALID, "rope: n_dims");
    if (pos->ne[0] < src->ne[2]) FAIL(CLLM_E_INVALID, "rope: pos shorter than sequence");
    if (freq_factors && (freq_factors->type != CLLM_TYPE_F32 || freq_factors->ne[0] < p->n_dims / 2)) FAIL(CLLM_E_INVALID, "rope: freq_factors");
    if (t_nelements(src) == 0) return CLLM_OK;
    rope_k_params k;
    k.n_dims = p->n_dims; k.mode = p->mode;
    k.theta_scale = powf(p->freq_base, -2.0f / p->n_dims);
    k.freq_scale = p->freq_scale; k.ext_factor = p->ext_factor; k.attn_factor = p->attn_factor;
    const float start = floorf(rope_corr_dim(p->n_dims, p->n_ctx_orig, p->beta_fast, p->freq_base));
    const float end   = ceilf (rope_corr_dim(p->n_dims, p->n_ctx_orig, p->beta_slow, p->freq_base));
    k.corr0 = fmaxf(0.0f, start); k.corr1 = fminf((float)(p->n_dims - 1), end);
    k.mscale_yarn = p->attn_factor * fmaf(0.1f, logf(1.0f / p->freq_scale), 1.0f);      // glibc's logf on the host: the reference's own value (ops.cpp:5607)
    hipLaunchKernelGGL(k_rope, dim3((unsigned)(src->ne[2] * src->ne[3])), dim3(256), (size_t) p->n_dims * 4, (hipStream_t) stream,
                       tv(src), tv(dst), (const int32_t *) pos->data, freq_factors ? (const float *) freq_factors->data : nullptr, k);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// The runner's prefill: ROPE(k) -> SET_ROWS(k_cache), TRANSPOSE(v) -> CPY(v_cache column), ROPE(q) of one token per workgroup in ONE launch
// (KVCacheAttention::forward src/layers.cpp:2925-2945, 3082-3093).  The cos / sin values, the rotation and the fp32 -> fp16 conversions are those of
// k_rope / k_set_rows / k_cpy above (plain RoPE: no frequency factors, freq_scale 1, no YaRN -- the cllm_llama configuration): same bits in q and in
// the caches.  qkv: [q | k | v] rows of QKV floats per token; q is rotated in place, k and v are only read.
__global__ void __launch_bounds__(256) k_rope_kv_store(float * __restrict__ qkv, int64_t QKV, const int32_t * __restrict__ pos, int nh, int nkv, int hd, int mode, float theta_scale,
                                                       uint16_t * __restrict__ k_cache, uint16_t * __restrict__ v_cache, int64_t ML) {
    extern __shared__ float cache[];                 // [hd]: cos, sin interleaved
    const int64_t tok = blockIdx.x;
    const int half = hd / 2, p = pos[tok];
    rope_table_fill(cache, p, half, theta_scale, threadIdx.x, blockDim.x);
    __syncthreads();
    const int64_t QD = (int64_t) nh * hd, KD = (int64_t) nkv * hd;
    const int off = rope_pair(mode, 0, half).off;
    float * q = qkv + tok * QKV;
    const float * k = q + QD, * v = k + KD;
    for (int t = threadIdx.x; t < nh * half; t += blockDim.x) {
        const int h = t / half, i = t % half, ic = rope_pair(mode, i, half).ic;
        const float c = cache[2*i], sn = cache[2*i + 1];
        float * x = q + (int64_t) h * hd;
        const float x0 = x[ic], x1 = x[ic + off];
        x[ic] = rope_rot_a(x0, x1, c, sn); x[ic + off] = rope_rot_b(x0, x1, c, sn);
    }
    if (p < 0 || p >= ML) return;                    // (the CPU asserts; never write out of bounds)
    uint16_t * kr = k_cache + (int64_t) p * KD;
    for (int t = threadIdx.x; t < nkv * half; t += blockDim.x) {
        const int h = t / half, i = t % half, ic = rope_pair(mode, i, half).ic;
        const float c = cache[2*i], sn = cache[2*i + 1];
        const float * x = k + (int64_t) h * hd;
        const float x0 = x[ic], x1 = x[ic + off];
        kr[(int64_t) h * hd + ic] = f2h(rope_rot_a(x0, x1, c, sn)); kr[(int64_t) h * hd + ic + off] = f2h(rope_rot_b(x0, x1, c, sn));
    }
    for (int64_t d = threadIdx.x; d < KD; d += blockDim.x) v_cache[d * ML + p] = f2h(v[d]);
}
int launch_rope_kv_store(hipStream_t st, float * qkv, int64_t QKV, const int32_t * pos, int64_t n_tok, int nh, int nkv, int hd, int mode, float freq_base,
                         void * k_cache, void * v_cache, int64_t ML) {
    if ((mode != 0 && mode != 2) || hd <= 0 || (hd & 1) || n_tok <= 0) return CLLM_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_rope_kv_store, dim3((unsigned) n_tok), dim3(256), (size_t) hd * 4, st, qkv, QKV, pos, nh, nkv, hd, mode, powf(freq_base, -2.0f / hd),
                       (uint16_t *) k_cache, (uint16_t *) v_cache, ML);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// ================================================================================================
// SOFT_MAX (+ SCALE + DIAG_MASK_INF)   ggml_compute_forward_soft_max_f32 ops.cpp:5225-5335,
//   ggml_vec_soft_max_f32 vec.cpp:547- (groups of 8 through ggml_v_expf, f32 tree hsum, total in double; expf tail)
// one wave per row; lane handles groups of 8 consecutive elements (the CPU's AVX2 vector), so the
// exponentials AND the per-group partial sums are bit-identical to the CPU's.
// ================================================================================================
template <int MODE>   // 0: plain (+scale, +mask tensor)   1: fused scale + causal mask(n_past)
__global__ void __launch_bounds__(256) k_soft_max(tview s, tview d, const char * __restrict__ mask, int mask_f16, int64_t m_nb1, int64_t m_nb2, int64_t m_nb3,
                                                  int64_t m_ne2, int64_t m_ne3, float scale, int n_past) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nrows = s.ne[1] * s.ne[2] * s.ne[3];
    if (row >= nrows) return;
    const tcoord c = t_row_coord(s, row);
    const int64_t i1 = c.i1;
    const float * x = (const float *) t_at(s, c);
    float *       y = (float *) t_at(d, c);
    const char * mp = mask ? mask + i1*m_nb1 + (c.i2 % m_ne2)*m_nb2 + (c.i3 % m_ne3)*m_nb3 : nullptr;
    const int64_t n = s.ne[0];

    auto val = [&](int64_t i) -> float {
        float v = x[i] * scale;
        if (MODE == 1) { if (i > (int64_t) n_past + i1) v = -INFINITY; }
        else if (mp)   { v += 1.0f * (mask_f16 ? h2f(((const uint16_t *) mp)[i]) : ((const float *) mp)[i]); }
        return v;
    };
    // MODE 1: everything from n_vis on is masked (-inf -> probability exactly 0): those entries are neither read nor
    // exponentiated, whole groups of 8 beyond it contribute an exact 0.0 to the sum, and zeros are stored for them
    const int64_t n_vis = MODE == 1 ? (n_past + i1 + 1 < n ? n_past + i1 + 1 : n) : n;
    float mx = -INFINITY;
    for (int64_t i = lane; i < n_vis; i += 64) mx = fmaxf(mx, val(i));
    mx = wave_max(mx);

    const int64_t nv = n & ~(int64_t) 7;
    const int64_t nv_vis = MODE == 1 ? (((n_vis + 7) & ~(int64_t) 7) < nv ? ((n_vis + 7) & ~(int64_t) 7) : nv) : nv;
    double sum = 0.0;
    if (MODE == 1) for (int64_t i = nv_vis + lane; i < nv; i += 64) y[i] = 0.0f;
    for (int64_t g = (int64_t) lane * 8; g < nv_vis; g += 64 * 8) {
        float e[8];
#pragma unroll
        for (int l = 0; l < 8; l++) { e[l] = ggml_expf_poly(val(g + l) - mx); y[g + l] = e[l]; }
        sum += (double) soft_group8_sum(e);
    }
    if (lane == 0) for (int64_t i = nv; i < n; i++) { const float e = libm_expf(val(i) - mx); y[i] = e; sum += (double) e; }
    sum = wave_sum_d(sum);
    double rinv = 1.0 / sum;                                 // (ORDER: soft_total_order_safe, common.h)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // e[] written by other lanes of this wave
    if (__builtin_expect(!soft_total_order_safe(rinv, (int)(n >> 3)), 0)) rinv = 1.0 / soft_sum_serial(y, (int) nv, (int) n);      // (masked entries hold exact zeros)
    const float inv = (float) rinv;
    const int64_t n_live = MODE == 1 ? (nv_vis < nv ? nv_vis : n) : n;      // the stored zeros stay zeros
    for (int64_t i = lane; i < n_live; i += 64) y[i] = y[i] * inv;
}

// fused scale + causal mask + soft_max with the row held in registers (prefill score rows: one read, one write instead of
// two of each).  Same lane -> group-of-8 mapping, same max set, same summation order as k_soft_max<1>: bit-identical.
// Needs n % 8 == 0, n <= 512 * NG, 16-byte aligned rows.
// OUT16: the probabilities are stored as fp16 (RNE of the float product: exactly what ggml's from_float makes of them when V.P takes them as src1), at the start of the
// row they came from -- the prompt's exact attention block (mmf_exact.hip) then reads half the bytes and converts nothing
template <int NG, bool OUT16 = false>
__global__ void __launch_bounds__(256) k_soft_max_causal_reg(tview s, tview d, float scale, int n_past) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nrows = s.ne[1] * s.ne[2] * s.ne[3];
    if (row >= nrows) return;
    const tcoord c = t_row_coord(s, row);
    const float * x = (const float *) t_at(s, c);
    float *       y = (float *) t_at(d, c);
    const int n = (int) s.ne[0];
    const int n_vis = n_past + (int) c.i1 + 1 < n ? n_past + (int) c.i1 + 1 : n;   // entries >= n_vis are masked
    float e[NG][8];
    float mx = -INFINITY;
    // every group's loads are issued before the first value is used (unconditional, clamped to the row's start where the group is masked: inside the
    // `if` the compiler waited for each group's pair of loads before requesting the next -- NG memory round trips per row)
    f32x4 lo[NG], hi[NG];
#pragma unroll
    for (int t = 0; t < NG; t++) {
        const int g0 = (lane + 64 * t) * 8, gc = g0 < n_vis ? g0 : 0;
        lo[t] = *(const f32x4 *)(x + gc); hi[t] = *(const f32x4 *)(x + gc + 4);
    }
#pragma unroll
    for (int t = 0; t < NG; t++) {
        const int g0 = (lane + 64 * t) * 8;
        if (g0 < n_vis) {
            const float v[8] = { lo[t].x, lo[t].y, lo[t].z, lo[t].w, hi[t].x, hi[t].y, hi[t].z, hi[t].w };
#pragma unroll
            for (int l = 0; l < 8; l++) { e[t][l] = g0 + l < n_vis ? v[l] * scale : -INFINITY; mx = fmaxf(mx, e[t][l]); }
        }
    }
    mx = wave_max(mx);
    double sum = 0.0;
#pragma unroll
    for (int t = 0; t < NG; t++) {
        const int g0 = (lane + 64 * t) * 8;
        if (g0 < n_vis) {
#pragma unroll
            for (int l = 0; l < 8; l++) e[t][l] = ggml_expf_poly(e[t][l] - mx);
            sum += (double) soft_group8_sum(e[t]);
        }
    }
    sum = wave_sum_d(sum);
    double rinv = 1.0 / sum;                                 // (ORDER: soft_total_order_safe, common.h)
    if (__builtin_expect(!soft_total_order_safe(rinv, n >> 3), 0)) {        // the exponentials go to the output row first (it is rewritten below), then lane 0 adds them serially
        float * yy = (float *) y;
#pragma unroll
        for (int t = 0; t < NG; t++) {
            const int g0 = (lane + 64 * t) * 8;
            if (g0 < n) {
#pragma unroll
                for (int l = 0; l < 8; l++) yy[g0 + l] = g0 < n_vis ? e[t][l] : 0.0f;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        rinv = 1.0 / soft_sum_serial(yy, n, n);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }
    const float inv = (float) rinv;
#pragma unroll
    for (int t = 0; t < NG; t++) {
        const int g0 = (lane + 64 * t) * 8;
        if (g0 < n) {
            f32x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
            if (g0 < n_vis) { lo = f32x4{e[t][0] * inv, e[t][1] * inv, e[t][2] * inv, e[t][3] * inv}; hi = f32x4{e[t][4] * inv, e[t][5] * inv, e[t][6] * inv, e[t][7] * inv}; }
            if constexpr (OUT16) {
                *(u32x4 *)((char *) y + (size_t) g0 * 2) = u32x4{ (uint32_t) f2h(lo.x) | ((uint32_t) f2h(lo.y) << 16), (uint32_t) f2h(lo.z) | ((uint32_t) f2h(lo.w) << 16),
                                                                  (uint32_t) f2h(hi.x) | ((uint32_t) f2h(hi.y) << 16), (uint32_t) f2h(hi.z) | ((uint32_t) f2h(hi.w) << 16) };
            } else { *(f32x4 *)(y + g0) = lo; *(f32x4 *)(y + g0 + 4) = hi; }
        }
    }
}

// the same for rows too long for registers (8192 < n <= 32768): one 256-thread workgroup per row, the row staged in LDS.
// All four waves exponentiate; the per-group float sums are accumulated by ONE wave in k_soft_max's order (lane l owns groups
// l, l + 64, ...; double; DPP tree), so the result is still bit-identical to the single-wave kernel.
__global__ void __launch_bounds__(256) k_soft_max_causal_lds(tview s, tview d, float scale, int n_past) {
    extern __shared__ __attribute__((aligned(16))) float sm[];      // [n] values | [n / 8] group sums
    __shared__ float red_f[4];
    __shared__ double red_d[1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const tcoord c = t_row_coord(s, blockIdx.x);
    const float * x = (const float *) t_at(s, c);
    float *       y = (float *) t_at(d, c);
    const int n = (int) s.ne[0];
    const int n_vis = n_past + (int) c.i1 + 1 < n ? n_past + (int) c.i1 + 1 : n;
    const int nv_vis = (n_vis + 7) & ~7;                              // n % 8 == 0: whole groups
    float * gsum = sm + n;
    float mx = -INFINITY;
    for (int g0 = tid * 8; g0 < nv_vis; g0 += 256 * 8) {
        const f32x4 lo = *(const f32x4 *)(x + g0), hi = *(const f32x4 *)(x + g0 + 4);
        const float v[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
#pragma unroll
        for (int l = 0; l < 8; l++) { const float t = g0 + l < n_vis ? v[l] * scale : -INFINITY; sm[g0 + l] = t; mx = fmaxf(mx, t); }
    }
    mx = wave_max(mx);
    if (lane == 0) red_f[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red_f[0], red_f[1]), fmaxf(red_f[2], red_f[3]));
    for (int g0 = tid * 8; g0 < nv_vis; g0 += 256 * 8) {              // each thread re-reads what it wrote
        float e[8];
#pragma unroll
        for (int l = 0; l < 8; l++) { e[l] = ggml_expf_poly(sm[g0 + l] - mx); sm[g0 + l] = e[l]; }
        gsum[g0 >> 3] = soft_group8_sum(e);
    }
    __syncthreads();
    if (wave == 0) {                                                  // (no leftovers: n % 8 == 0; groups beyond nv_vis are exact zeros in the reference's sum of n / 8 terms)
        const double rinv = soft_total_rinv_groups(gsum, nv_vis >> 3, sm, 0, 0, mx, n >> 3, lane);
        if (lane == 0) red_d[0] = rinv;
    }
    __syncthreads();
    const float inv = (float) red_d[0];
    for (int g0 = tid * 8; g0 < n; g0 += 256 * 8) {
        f32x4 lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};
        if (g0 < nv_vis) { lo = f32x4{sm[g0] * inv, sm[g0 + 1] * inv, sm[g0 + 2] * inv, sm[g0 + 3] * inv}; hi = f32x4{sm[g0 + 4] * inv, sm[g0 + 5] * inv, sm[g0 + 6] * inv, sm[g0 + 7] * inv}; }
        *(f32x4 *)(y + g0) = lo; *(f32x4 *)(y + g0 + 4) = hi;
    }
}

// SCALE + DIAG_MASK_INF + SOFT_MAX over f32 rows [n, rows ...] IN PLACE, the probabilities left as fp16 at the start of each row (see k_soft_max_causal_reg<.., true>);
// CLLM_E_UNSUPPORTED: shapes the register-resident kernel does not take (the caller keeps f32)
int launch_soft_max_causal_f16out(hipStream_t st, const tview & sv, float scale, int n_past) {
    const int64_t n = sv.ne[0], rows = sv.ne[1] * sv.ne[2] * sv.ne[3];
    if (n % 8 || n < 512 || n > 8192 || rows <= 0 || (((uintptr_t) sv.data | (uintptr_t) sv.nb[1] | (uintptr_t) sv.nb[2] | (uintptr_t) sv.nb[3]) & 15) || sv.nb[0] != 4) return CLLM_E_UNSUPPORTED;
    const unsigned grid = (unsigned)((rows + 3) / 4);
    if (n <= 4096) hipLaunchKernelGGL((k_soft_max_causal_reg<8, true>),  dim3(grid), dim3(256), 0, st, sv, sv, scale, n_past);
    else           hipLaunchKernelGGL((k_soft_max_causal_reg<16, true>), dim3(grid), dim3(256), 0, st, sv, sv, scale, n_past);
    LAUNCH_CHECK();
    return CLLM_OK;
}

static int soft_max_impl(void * stream, const cllm_tensor * src, const cllm_tensor * mask, cllm_tensor * dst, float scale, int fused, int n_past) {
    if (const int rc = row_op_args("soft_max", src, dst, ROW_F32_SHAPE | ROW_DENSE_INVALID)) return rc;
    if (mask) {
        if (mask->type != CLLM_TYPE_F32 && mask->type != CLLM_TYPE_F16) FAIL(CLLM_E_UNSUPPORTED, "soft_max: mask type");
        if (mask->ne[0] != src->ne[0] || mask->ne[1] < src->ne[1] || src->ne[2] % mask->ne[2] || src->ne[3] % mask->ne[3]) FAIL(CLLM_E_INVALID, "soft_max: mask shape");
    }
    const int64_t rows = t_nrows(src);
    if (rows == 0 || src->ne[0] == 0) return CLLM_OK;
    const unsigned grid = (unsigned)((rows + 3) / 4);
    hipStream_t st = (hipStream_t) stream;
    const int64_t n = src->ne[0];
    const bool al16 = !((((uintptr_t) src->data | src->nb[1] | src->nb[2] | src->nb[3] | (uintptr_t) dst->data | dst->nb[1] | dst->nb[2] | dst->nb[3])) & 15);
    if (fused && n % 8 == 0 && n >= 512 && n <= 8192 && al16) {      // long (prefill) rows: register-resident single pass
        if (n <= 4096) hipLaunchKernelGGL(k_soft_max_causal_reg<8>,  dim3(grid), dim3(256), 0, st, tv(src), tv(dst), scale, n_past);
        else           hipLaunchKernelGGL(k_soft_max_causal_reg<16>, dim3(grid), dim3(256), 0, st, tv(src), tv(dst), scale, n_past);
        LAUNCH_CHECK();
        return CLLM_OK;
    }
    if (fused && n % 8 == 0 && n > 8192 && n <= 32768 && al16 && rows <= 0x7fffffff) {      // very long rows: one workgroup per row, row in LDS
        const size_t lds = (size_t)(n + n / 8) * 4;
        static uint64_t attr = 0;
        if (const int rc = lds_opt_in(k_soft_max_causal_lds, attr)) return rc;
        hipLaunchKernelGGL(k_soft_max_causal_lds, dim3((unsigned) rows), dim3(256), lds, st, tv(src), tv(dst), scale, n_past);
        LAUNCH_CHECK();
        return CLLM_OK;
    }
    if (fused) hipLaunchKernelGGL(k_soft_max<1>, dim3(grid), dim3(256), 0, st, tv(src), tv(dst), (const char *) nullptr, 0, (int64_t) 0, (int64_t) 0, (int64_t) 0, (int64_t) 1, (int64_t) 1, scale, n_past);
    else       hipLaunchKernelGGL(k_soft_max<0>, dim3(grid), dim3(256), 0, st, tv(src), tv(dst), mask ? (const char *) mask->data : nullptr, mask && mask->type == CLLM_TYPE_F16 ? 1 : 0,
                                  mask ? (int64_t) mask->nb[1] : 0, mask ? (int64_t) mask->nb[2] : 0, mask ? (int64_t) mask->nb[3] : 0, mask ? mask->ne[2] : 1, mask ? mask->ne[3] : 1, scale, 0);
    LAUNCH_CHECK();
    return CLLM_OK;
}
extern "C" int cllm_op_soft_max(void * stream, const cllm_tensor * src, const cllm_tensor * mask, cllm_tensor * dst, float scale, float max_bias) {
    if (max_bias != 0.0f) FAIL(CLLM_E_UNSUPPORTED, "soft_max: ALiBi (max_bias != 0) is not on this path");
    return soft_max_impl(stream, src, mask, dst, scale, 0, 0);
}
extern "C" int cllm_op_scale_mask_soft_max(void * stream, const cllm_tensor * src, cllm_tensor * dst, float scale, int n_past) {
    if (n_past < 0) FAIL(CLLM_E_INVALID, "soft_max: n_past");
    return soft_max_impl(stream, src, nullptr, dst, scale, 1, n_past);
}

// ================================================================================================
// element-wise family: generic strided, one thread per element of dst (t_elem_coord), src1 broadcast over it
// ================================================================================================
enum { EW_DIAG_MASK = 0, EW_SCALE = 1, EW_SILU = 2, EW_ADD = 3, EW_MUL = 4, EW_SILU_MUL = 5, EW_DIV = 6,
       EW_SIGMOID = 7, EW_TANH = 8, EW_RELU = 9, EW_SQR = 10, EW_GELU = 11, EW_GELU_QUICK = 12 };

// ggml_table_gelu_f16 / ggml_table_gelu_quick_f16 (vec.cpp:5-9), built on the host by gm_build_gelu_tables and uploaded once per device
__device__ uint16_t g_gelu_tab[2][1 << 16];
static int gelu_tables_upload() {
    static std::mutex m;
    static uint64_t up = 0;
    static std::vector<uint16_t> tab;
    std::lock_guard<std::mutex> lock(m);
    if (!dev_flag_unset(up)) return CLLM_OK;
    if (tab.empty()) { tab.resize(2 << 16); gm_build_gelu_tables(tab.data(), tab.data() + (1 << 16)); }
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_gelu_tab), tab.data(), tab.size() * sizeof(uint16_t)));
    dev_flag_set(up);
    return CLLM_OK;
}

template <int OP>
__global__ void __launch_bounds__(256) k_elementwise(tview a, tview b, tview d, float f0, float f1, int i0p) {
    const int64_t n = d.ne[0] * d.ne[1] * d.ne[2] * d.ne[3];
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t) gridDim.x * blockDim.x) {
        const tcoord c = t_elem_coord(d, e);
        const int64_t i0 = c.i0, i1 = c.i1;
        const float x = *(const float *) t_at(a, c);
        float y;
        if (OP == EW_DIAG_MASK)      y = (i0 > (int64_t) i0p + i1) ? -INFINITY : x;      // ops.cpp:5137-5185
        // ggml_vec_scale_f32 / ggml_vec_mad1_f32 (vec.h:667-712): with a bias the reference build rounds once in every element of a row, the
        // _mm256_fmadd_ps body and the leftovers alike (gcc contracts their x[i]*s + b): tests/test_elementwise_model.py
        else if (OP == EW_SCALE)     y = (f1 == 0.0f) ? x * f0 : __builtin_fmaf(x, f0, f1);
        else if (OP == EW_SILU) {
            // ggml_vec_silu_f32 (vec.cpp:396-431): AVX2 body for i0 < (ne0 & ~7), scalar expf tail
            y = (i0 < (d.ne[0] & ~(int64_t) 7)) ? x / (1.0f + ggml_expf_poly(0.0f - x)) : x / (1.0f + libm_expf(-x));
        }
        else if (OP == EW_SIGMOID)   y = gm_sigmoidf(x);                                 // op_sigmoid (unary-ops.cpp:31-33): no vector body, libm expf
        else if (OP == EW_TANH)      y = gm_tanhf(x);                                    // op_tanh (unary-ops.cpp:19-21): libm tanhf
        else if (OP == EW_RELU)      y = (x > 0.0f) ? x : 0.0f;                          // op_relu (unary-ops.cpp:27-29)
        else if (OP == EW_SQR)       y = x * x;                                          // op_sqr (unary-ops.cpp:47-49)
        else if (OP == EW_GELU)      y = gm_gelu_lookup(g_gelu_tab[0], x);                 // ggml_vec_gelu_f32 (vec.h:996-1009)
        else if (OP == EW_GELU_QUICK) y = gm_gelu_quick_lookup(g_gelu_tab[1], x);          // ggml_vec_gelu_quick_f32 (vec.h:1037-1044)
        else {
            const float z = *(const float *) t_at(b, tcoord{ i0 % b.ne[0], i1 % b.ne[1], c.i2 % b.ne[2], c.i3 % b.ne[3] });
            if (OP == EW_ADD)      y = x + z;
            else if (OP == EW_MUL) y = x * z;
            else if (OP == EW_DIV) y = __fdiv_rn(x, z);                                     // IEEE division (ggml_vec_div_f32)
            else {                                                                          // silu(gate) * up
                const float sl = (i0 < (d.ne[0] & ~(int64_t) 7)) ? x / (1.0f + ggml_expf_poly(0.0f - x)) : x / (1.0f + libm_expf(-x));
                y = sl * z;
            }
        }
        *(float *) t_at(d, c) = y;
    }
}

template <int OP>
static int ew_launch(void * stream, const cllm_tensor * a, const cllm_tensor * b, cllm_tensor * d, float f0, float f1, int ip, const char * name) {
    if (!a || !d) FAIL(CLLM_E_INVALID, "%s: null", name);
    if (a->type != CLLM_TYPE_F32 || d->type != CLLM_TYPE_F32 || (b && b->type != CLLM_TYPE_F32)) FAIL(CLLM_E_UNSUPPORTED, "%s: type", name);
    if (!t_same_shape(a, d)) FAIL(CLLM_E_INVALID, "%s: shape", name);
    if (b) for (int i = 0; i < 4; i++) if (b->ne[i] <= 0 || a->ne[i] % b->ne[i]) FAIL(CLLM_E_INVALID, "%s: src1 not broadcastable", name);
    const int64_t n = t_nelements(d);
    if (n == 0) return CLLM_OK;
    hipLaunchKernelGGL(k_elementwise<OP>, dim3(grid_1d(n, 8192)), dim3(256), 0, (hipStream_t) stream, tv(a), b ? tv(b) : tv(a), tv(d), f0, f1, ip);
    LAUNCH_CHECK();
    return CLLM_OK;
}
extern "C" int cllm_op_diag_mask_inf(void * stream, const cllm_tensor * src, cllm_tensor * dst, int n_past) {
    if (n_past < 0) FAIL(CLLM_E_INVALID, "diag_mask_inf: n_past");
    return ew_launch<EW_DIAG_MASK>(stream, src, nullptr, dst, 0, 0, n_past, "diag_mask_inf");
}
extern "C" int cllm_op_scale(void * stream, const cllm_tensor * src, cllm_tensor * dst, float s, float b) { return ew_launch<EW_SCALE>(stream, src, nullptr, dst, s, b, 0, "scale"); }
extern "C" int cllm_op_unary(void * stream, int op, const cllm_tensor * src, cllm_tensor * dst) {
    if (src && dst && (src->nb[0] != 4 || dst->nb[0] != 4)) FAIL(CLLM_E_UNSUPPORTED, "unary: rows must be dense");
    switch (op) {
        case CLLM_UNARY_TANH:    return ew_launch<EW_TANH>(stream, src, nullptr, dst, 0, 0, 0, "tanh");
        case CLLM_UNARY_RELU:    return ew_launch<EW_RELU>(stream, src, nullptr, dst, 0, 0, 0, "relu");
        case CLLM_UNARY_SIGMOID: return ew_launch<EW_SIGMOID>(stream, src, nullptr, dst, 0, 0, 0, "sigmoid");
        case CLLM_UNARY_GELU:       if (int rc = gelu_tables_upload()) return rc; return ew_launch<EW_GELU>(stream, src, nullptr, dst, 0, 0, 0, "gelu");
        case CLLM_UNARY_GELU_QUICK: if (int rc = gelu_tables_upload()) return rc; return ew_launch<EW_GELU_QUICK>(stream, src, nullptr, dst, 0, 0, 0, "gelu_quick");
        case CLLM_UNARY_SILU:    return ew_launch<EW_SILU>(stream, src, nullptr, dst, 0, 0, 0, "silu");
        default:                 FAIL(CLLM_E_UNSUPPORTED, "unary: op %d", op);
    }
}
extern "C" int cllm_op_sqr(void * stream, const cllm_tensor * src, cllm_tensor * dst) {
    if (src && dst && (src->nb[0] != 4 || dst->nb[0] != 4)) FAIL(CLLM_E_UNSUPPORTED, "sqr: rows must be dense");
    return ew_launch<EW_SQR>(stream, src, nullptr, dst, 0, 0, 0, "sqr");
}
extern "C" int cllm_op_add(void * stream, const cllm_tensor * a, const cllm_tensor * b, cllm_tensor * dst) { if (!b) FAIL(CLLM_E_INVALID, "add: null"); return ew_launch<EW_ADD>(stream, a, b, dst, 0, 0, 0, "add"); }
extern "C" int cllm_op_mul(void * stream, const cllm_tensor * a, const cllm_tensor * b, cllm_tensor * dst) { if (!b) FAIL(CLLM_E_INVALID, "mul: null"); return ew_launch<EW_MUL>(stream, a, b, dst, 0, 0, 0, "mul"); }
extern "C" int cllm_op_div(void * stream, const cllm_tensor * a, const cllm_tensor * b, cllm_tensor * dst) { if (!b) FAIL(CLLM_E_INVALID, "div: null"); return ew_launch<EW_DIV>(stream, a, b, dst, 0, 0, 0, "div"); }
extern "C" int cllm_op_silu_mul(void * stream, const cllm_tensor * g, const cllm_tensor * u, cllm_tensor * dst) { if (!u) FAIL(CLLM_E_INVALID, "silu_mul: null"); return ew_launch<EW_SILU_MUL>(stream, g, u, dst, 0, 0, 0, "silu_mul"); }

// ================================================================================================
// SUM_ROWS / TOP_K: the router of a sparse-MoE block (GenericSparseMLP::forward, src/layers.cpp:3755-3815): rows of n_expert values
// ================================================================================================
// ggml_compute_forward_sum_rows_f32 (ops.cpp:1451-1482) -> ggml_vec_sum_f32 (vec.h:1510-1520): sequential, accumulated in double
__global__ void __launch_bounds__(256) k_sum_rows(tview s, tview d) {
    const int64_t rows = s.ne[1] * s.ne[2] * s.ne[3];
    for (int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t) gridDim.x * blockDim.x) {
        const tcoord c = t_row_coord(s, r);
        const float * x = (const float *) t_at(s, c);
        double sum = 0.0;
        for (int64_t i = 0; i < s.ne[0]; i++) sum += (double) x[i];
        *(float *) t_at(d, c) = (float) sum;
    }
}
extern "C" int cllm_op_sum_rows(void * stream, const cllm_tensor * src, cllm_tensor * dst) {
    if (!src || !dst) FAIL(CLLM_E_INVALID, "sum_rows: null");
    if (src->type != CLLM_TYPE_F32 || dst->type != CLLM_TYPE_F32 || src->nb[0] != 4 || dst->nb[0] != 4) FAIL(CLLM_E_UNSUPPORTED, "sum_rows: dense F32 rows");
    if (dst->ne[0] != 1 || dst->ne[1] != src->ne[1] || dst->ne[2] != src->ne[2] || dst->ne[3] != src->ne[3]) FAIL(CLLM_E_INVALID, "sum_rows: shape");
    const int64_t rows = src->ne[1] * src->ne[2] * src->ne[3];
    if (rows == 0) return CLLM_OK;
    hipLaunchKernelGGL(k_sum_rows, dim3(grid_1d(rows, 4096)), dim3(256), 0, (hipStream_t) stream, tv(src), tv(dst));
    LAUNCH_CHECK();
    return CLLM_OK;
}
// ggml_compute_forward_top_k_f32 (ops.cpp:8057-8094): the indices of the k largest values in descending order (std::partial_sort with
// data[a] > data[b]), then the first two swapped ("the order is not important").  Equal values: the lower index first (the reference
// leaves that to its heap; softmax probabilities of distinct logits do not tie).  One thread per row: rows are n_expert long.
__global__ void __launch_bounds__(256) k_top_k(tview s, tview d, int k) {
    const int64_t rows = s.ne[1] * s.ne[2] * s.ne[3];
    const int n = (int) s.ne[0];
    for (int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t) gridDim.x * blockDim.x) {
        const tcoord c = t_row_coord(s, r);
        top_k_row((const float *) t_at(s, c), n, k, (int32_t *) t_at(d, c));
    }
}
extern "C" int cllm_op_top_k(void * stream, const cllm_tensor * src, cllm_tensor * dst) {
    if (!src || !dst) FAIL(CLLM_E_INVALID, "top_k: null");
    if (src->type != CLLM_TYPE_F32 || dst->type != CLLM_TYPE_I32 || src->nb[0] != 4 || dst->nb[0] != 4) FAIL(CLLM_E_UNSUPPORTED, "top_k: F32 rows -> I32 rows");
    const int64_t k = dst->ne[0];
    if (k < 1 || k > src->ne[0] || dst->ne[1] != src->ne[1] || dst->ne[2] != src->ne[2] || dst->ne[3] != src->ne[3]) FAIL(CLLM_E_INVALID, "top_k: shape");
    if (src->ne[0] > 4096) FAIL(CLLM_E_UNSUPPORTED, "top_k: rows of %lld values", (long long) src->ne[0]);
    const int64_t rows = src->ne[1] * src->ne[2] * src->ne[3];
    if (rows == 0) return CLLM_OK;
    hipLaunchKernelGGL(k_top_k, dim3(grid_1d(rows, 4096)), dim3(256), 0, (hipStream_t) stream, tv(src), tv(dst), (int) k);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// The tail of GenericSparseMLP::forward / forward_with_experts (src/layers.cpp:3792-3872) as one launch:
//   weights = GET_ROWS(probs, ids); weights /= SUM_ROWS(weights)  [norm_topk_prob]; experts *= weights; out = experts[:,0] + experts[:,1] + ... (+ resid)
// Same operations in the same order as the nodes (double-accumulated sum, IEEE division, left-to-right adds): bit-identical.
__global__ void __launch_bounds__(256) k_moe_combine(tview e, tview p, tview ids, tview r, tview d, int k, int has_resid) {
    const int64_t H = d.ne[0], n = d.ne[0] * d.ne[1];
    for (int64_t x = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (int64_t) gridDim.x * blockDim.x) {
        const int64_t h = x % H, t = x / H;
        double s = 0.0;
        for (int j = 0; j < k; j++) {
            const int32_t id = *(const int32_t *)(ids.data + j*ids.nb[0] + t*ids.nb[1]);
            s += (double) *(const float *)(p.data + (int64_t) id*4 + t*p.nb[1]);
        }
        const float sum = (float) s;
        float acc = 0.0f;
        for (int j = 0; j < k; j++) {
            const int32_t id = *(const int32_t *)(ids.data + j*ids.nb[0] + t*ids.nb[1]);
            const float w = __fdiv_rn(*(const float *)(p.data + (int64_t) id*4 + t*p.nb[1]), sum);
            const float y = *(const float *)(e.data + h*4 + j*e.nb[1] + t*e.nb[2]) * w;
            acc = j == 0 ? y : acc + y;
        }
        if (has_resid) acc = acc + *(const float *)(r.data + h*4 + t*r.nb[1]);
        *(float *)(d.data + h*4 + t*d.nb[1]) = acc;
    }
}
extern "C" int cllm_op_moe_combine(void * stream, const cllm_tensor * experts, const cllm_tensor * probs, const cllm_tensor * ids, const cllm_tensor * resid,
                                   cllm_tensor * dst) {
    if (!experts || !probs || !ids || !dst) FAIL(CLLM_E_INVALID, "moe_combine: null");
    if (experts->type != CLLM_TYPE_F32 || probs->type != CLLM_TYPE_F32 || ids->type != CLLM_TYPE_I32 || dst->type != CLLM_TYPE_F32 || (resid && resid->type != CLLM_TYPE_F32))
        FAIL(CLLM_E_UNSUPPORTED, "moe_combine: types");
    const int64_t H = experts->ne[0], k = experts->ne[1], T = experts->ne[2];
    if (k < 1 || k > 64 || ids->ne[0] != k || ids->ne[1] != T || probs->ne[1] != T || dst->ne[0] != H || dst->ne[1] != T || experts->ne[3] != 1 ||
        experts->nb[0] != 4 || probs->nb[0] != 4 || dst->nb[0] != 4 || (resid && (resid->ne[0] != H || resid->ne[1] != T || resid->nb[0] != 4)))
        FAIL(CLLM_E_INVALID, "moe_combine: shapes");
    if (H * T == 0) return CLLM_OK;
    hipLaunchKernelGGL(k_moe_combine, dim3(grid_1d(H * T, 8192)), dim3(256), 0, (hipStream_t) stream, tv(experts), tv(probs), tv(ids), resid ? tv(resid) : tv(dst), tv(dst), (int) k, resid ? 1 : 0);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// ================================================================================================
// SET_ROWS (K-cache write)   ggml_compute_forward_set_rows_f32, ops.cpp:4892-4940
// ================================================================================================
// the destination row of the source row at c: the index tensor [ne1, ...] is broadcast over dimensions 2 and 3 of the source
template <typename IDX>
__device__ __forceinline__ int64_t set_rows_row(const tview & idx, const tcoord & c) {
    return (int64_t) *(const IDX *) t_at(idx, tcoord{ c.i1, c.i2 % idx.ne[1], c.i3 % idx.ne[2], 0 });
}
template <typename IDX, bool F16>
__global__ void __launch_bounds__(256) k_set_rows(tview s, tview idx, tview d) {
    const int64_t n = s.ne[0] * s.ne[1] * s.ne[2] * s.ne[3];
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t) gridDim.x * blockDim.x) {
        const tcoord c = t_elem_coord(s, e);
        const int64_t row = set_rows_row<IDX>(idx, c);
        if (row < 0 || row >= d.ne[1]) continue;     // the CPU asserts; never write out of bounds
        const float v = ((const float *) t_row_at(s, c))[c.i0];
        char * dp = t_at(d, tcoord{0, row, c.i2, c.i3});
        if (F16) ((uint16_t *) dp)[c.i0] = f2h(v); else ((float *) dp)[c.i0] = v;
    }
}
// Q8_0 rows (--cache_dtype q8_0, src/layers.cpp:2925-2945): from_float of the CPU traits = quantize_row_q8_0 (x86 branch), 8 lanes per 32-block
template <typename IDX>
__global__ void __launch_bounds__(256) k_set_rows_q8_0(tview s, tview idx, tview d) {
    const int64_t nb = s.ne[0] / 32, nblk = nb * s.ne[1] * s.ne[2] * s.ne[3];
    const int sub = threadIdx.x & 7;
    for (int64_t g0 = ((int64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 3; g0 - ((threadIdx.x & 63) >> 3) < nblk; g0 += ((int64_t) gridDim.x * blockDim.x) >> 3) {
        const bool live = g0 < nblk;                            // whole waves stay in the loop: the 8-lane reductions read their neighbours by DPP
        const tcoord c = t_unit_coord(nb, s, live ? g0 : nblk - 1);      // i0: the 32-block of the row
        const int64_t blk = c.i0, row = set_rows_row<IDX>(idx, c);
        const f32x4 v = *(const f32x4 *)(t_row_at(s, c) + (blk * 32 + sub * 4) * 4);
        float dd; int ss;
        const uint32_t p = quant4_q8_0<false, true>(v, &dd, &ss);      // SAT: an inverse scale that overflows gives 32 quants of -128, as the CPU's saturating packs do
        if (!live || row < 0 || row >= d.ne[1]) continue;
        char * dp = t_at(d, tcoord{0, row, c.i2, c.i3}) + blk * 34;
        if (sub == 0) *(uint16_t *) dp = f2h(dd);
        *(uint16_t *)(dp + 2 + sub * 4) = (uint16_t) p; *(uint16_t *)(dp + 4 + sub * 4) = (uint16_t)(p >> 16);
    }
}
// leaf(IDX()) with the element type of an index tensor that its caller has checked to be I32 or I64
template <class Leaf> static inline void with_idx_type(int type, Leaf && leaf) { if (type == CLLM_TYPE_I64) leaf(int64_t()); else leaf(int32_t()); }
extern "C" int cllm_op_set_rows(void * stream, const cllm_tensor * src, const cllm_tensor * idx, cllm_tensor * dst) {
    if (!src || !idx || !dst) FAIL(CLLM_E_INVALID, "set_rows: null");
    hipStream_t st = (hipStream_t) stream;
    if (src->type == CLLM_TYPE_F32 && dst->type == CLLM_TYPE_Q8_0) {
        if (idx->type != CLLM_TYPE_I32 && idx->type != CLLM_TYPE_I64) FAIL(CLLM_E_UNSUPPORTED, "set_rows: index type");
        if (dst->ne[0] != src->ne[0] || dst->ne[2] != src->ne[2] || dst->ne[3] != src->ne[3] || src->nb[0] != 4 || dst->nb[0] != 34 || src->ne[0] % 32) FAIL(CLLM_E_INVALID, "set_rows: shape");
        if (idx->ne[0] != src->ne[1] || src->ne[2] % idx->ne[1] || src->ne[3] % idx->ne[2]) FAIL(CLLM_E_INVALID, "set_rows: index shape");
        if ((((uintptr_t) src->data | src->nb[1] | src->nb[2] | src->nb[3]) & 15) || (((uintptr_t) dst->data | dst->nb[1] | dst->nb[2] | dst->nb[3]) & 1)) FAIL(CLLM_E_UNSUPPORTED, "set_rows: alignment");
        const int64_t nblk = t_nelements(src) / 32;
        if (nblk == 0) return CLLM_OK;
        with_idx_type(idx->type, [&](auto i) { hipLaunchKernelGGL((k_set_rows_q8_0<decltype(i)>), dim3(grid_1d(nblk * 8, 8192)), dim3(256), 0, st, tv(src), tv(idx), tv(dst)); });
        LAUNCH_CHECK();
        return CLLM_OK;
    }
    if (src->type != CLLM_TYPE_F32 || (dst->type != CLLM_TYPE_F16 && dst->type != CLLM_TYPE_F32)) FAIL(CLLM_E_UNSUPPORTED, "set_rows: type");
    if (idx->type != CLLM_TYPE_I32 && idx->type != CLLM_TYPE_I64) FAIL(CLLM_E_UNSUPPORTED, "set_rows: index type");
    if (dst->ne[0] != src->ne[0] || dst->ne[2] != src->ne[2] || dst->ne[3] != src->ne[3] || src->nb[0] != 4 || dst->nb[0] != cllm_type_size(dst->type)) FAIL(CLLM_E_INVALID, "set_rows: shape");
    if (idx->ne[0] != src->ne[1] || src->ne[2] % idx->ne[1] || src->ne[3] % idx->ne[2]) FAIL(CLLM_E_INVALID, "set_rows: index shape");
    const int64_t n = t_nelements(src);
    if (n == 0) return CLLM_OK;
    with_idx_type(idx->type, [&](auto i) {
        if (dst->type == CLLM_TYPE_F16) hipLaunchKernelGGL((k_set_rows<decltype(i), true>),  dim3(grid_1d(n, 8192)), dim3(256), 0, st, tv(src), tv(idx), tv(dst));
        else                            hipLaunchKernelGGL((k_set_rows<decltype(i), false>), dim3(grid_1d(n, 8192)), dim3(256), 0, st, tv(src), tv(idx), tv(dst));
    });
    LAUNCH_CHECK();
    return CLLM_OK;
}

// ================================================================================================
// CPY / DUP / CONT    ggml_compute_forward_dup, ops.cpp:47-330,526: element e of src (row-major over ne) -> element e of dst
// ================================================================================================
template <typename TS, typename TD>
__global__ void __launch_bounds__(256) k_cpy(tview s, tview d) {
    const int64_t n = s.ne[0] * s.ne[1] * s.ne[2] * s.ne[3];
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t) gridDim.x * blockDim.x) {
        const TS v = *(const TS *) t_at(s, t_elem_coord(s, e));
        TD o;
        if constexpr (sizeof(TS) == sizeof(TD)) o = (TD) v;
        else if constexpr (sizeof(TS) == 4) o = f2h(v);          // F32 -> F16, RNE
        else o = h2f(v);                                         // F16 -> F32
        *(TD *) t_at(d, t_elem_coord(d, e)) = o;
    }
}
// same quantized type on both sides (CONT of the permuted Q8_0 K-cache view, src/layers.cpp:3144-3146): whole rows move, 2 bytes per thread step
__global__ void __launch_bounds__(256) k_cpy_qrows(tview s, tview d, int row_bytes) {
    const int64_t h = row_bytes / 2, n = h * s.ne[1] * s.ne[2] * s.ne[3];
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t) gridDim.x * blockDim.x) {
        const tcoord cs = t_unit_coord(h, s, e), cd = t_unit_coord(h, d, e);      // i0: the byte pair of the row, the same on both sides
        ((uint16_t *) t_row_at(d, cd))[cd.i0] = ((const uint16_t *) t_row_at(s, cs))[cs.i0];
    }
}
extern "C" int cllm_op_cpy(void * stream, const cllm_tensor * src, cllm_tensor * dst) {
    if (!src || !dst) FAIL(CLLM_E_INVALID, "cpy: null");
    if (src->type == dst->type && (is_quant_type(src->type) || is_kq_type(src->type))) {
        const size_t rb = cllm_row_size(src->type, src->ne[0]);
        if (src->ne[0] != dst->ne[0] || t_nelements(src) != t_nelements(dst) || src->nb[0] != cllm_type_size(src->type) || dst->nb[0] != src->nb[0] || rb % 2) FAIL(CLLM_E_UNSUPPORTED, "cpy: quantized rows must stay whole");
        if ((((uintptr_t) src->data | src->nb[1] | src->nb[2] | src->nb[3] | (uintptr_t) dst->data | dst->nb[1] | dst->nb[2] | dst->nb[3]) & 1)) FAIL(CLLM_E_UNSUPPORTED, "cpy: alignment");
        const int64_t n = (int64_t)(rb / 2) * src->ne[1] * src->ne[2] * src->ne[3];
        if (n == 0) return CLLM_OK;
        hipLaunchKernelGGL(k_cpy_qrows, dim3(grid_1d(n, 16384)), dim3(256), 0, (hipStream_t) stream, tv(src), tv(dst), (int) rb);
        LAUNCH_CHECK();
        return CLLM_OK;
    }
    const bool s32 = src->type == CLLM_TYPE_F32 || src->type == CLLM_TYPE_I32, s16 = src->type == CLLM_TYPE_F16;
    const bool d32 = dst->type == CLLM_TYPE_F32 || dst->type == CLLM_TYPE_I32, d16 = dst->type == CLLM_TYPE_F16;
    if (!(s32 || s16) || !(d32 || d16)) FAIL(CLLM_E_UNSUPPORTED, "cpy: type %d -> %d", src->type, dst->type);
    if ((src->type == CLLM_TYPE_I32) != (dst->type == CLLM_TYPE_I32)) FAIL(CLLM_E_UNSUPPORTED, "cpy: I32 only to I32");
    if (t_nelements(src) != t_nelements(dst)) FAIL(CLLM_E_INVALID, "cpy: element count");
    const int64_t n = t_nelements(src);
    if (n == 0) return CLLM_OK;
    const dim3 grid(grid_1d(n, 16384));
    hipStream_t st = (hipStream_t) stream;
    if (s32 && d32)      hipLaunchKernelGGL((k_cpy<uint32_t, uint32_t>), grid, dim3(256), 0, st, tv(src), tv(dst));
    else if (s16 && d16) hipLaunchKernelGGL((k_cpy<uint16_t, uint16_t>), grid, dim3(256), 0, st, tv(src), tv(dst));
    else if (s32 && d16) hipLaunchKernelGGL((k_cpy<float, uint16_t>),    grid, dim3(256), 0, st, tv(src), tv(dst));
    else                 hipLaunchKernelGGL((k_cpy<uint16_t, float>),    grid, dim3(256), 0, st, tv(src), tv(dst));
    LAUNCH_CHECK();
    return CLLM_OK;
}

// ================================================================================================
// GET_ROWS / dequantize    ops.cpp:4653-4700,4820 ; dequantize_row_* ggml-quants.c:307-325,401-414,1352-1373
// ================================================================================================
#include "dequant.h"
__global__ void __launch_bounds__(256) k_get_rows(int type, tview s, tview idx, tview d) {
    const int64_t n = d.ne[0] * d.ne[1] * d.ne[2] * d.ne[3];
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t) gridDim.x * blockDim.x) {
        const tcoord c = t_elem_coord(d, e);
        const int64_t row = *(const int32_t *) t_at(idx, tcoord{c.i1, c.i2, c.i3, 0});
        float v = 0.0f;
        if (row >= 0 && row < s.ne[1]) v = dequant_elem(type, t_at(s, tcoord{0, row, c.i2, c.i3}), c.i0);
        ((float *) t_row_at(d, c))[c.i0] = v;
    }
}
extern "C" int cllm_op_get_rows(void * stream, const cllm_tensor * src, const cllm_tensor * idx, cllm_tensor * dst) {
    if (!src || !idx || !dst) FAIL(CLLM_E_INVALID, "get_rows: null");
    if (idx->type != CLLM_TYPE_I32 || dst->type != CLLM_TYPE_F32) FAIL(CLLM_E_UNSUPPORTED, "get_rows: type");
    if (!wtype_has_get_rows(src->type)) FAIL(CLLM_E_UNSUPPORTED, "get_rows: src type %d", src->type);
    if (dst->ne[0] != src->ne[0] || dst->ne[1] != idx->ne[0] || dst->ne[2] != idx->ne[1] || dst->ne[3] != idx->ne[2] || dst->nb[0] != 4) FAIL(CLLM_E_INVALID, "get_rows: shape");
    const int64_t n = t_nelements(dst);
    if (n == 0) return CLLM_OK;
    hipLaunchKernelGGL(k_get_rows, dim3(grid_1d(n, 8192)), dim3(256), 0, (hipStream_t) stream, src->type, tv(src), tv(idx), tv(dst));
    LAUNCH_CHECK();
    return CLLM_OK;
}
extern "C" int cllm_dequantize_row(void * stream, int type, const void * blocks, float * y, int64_t k) {
    if (!blocks || !y || k <= 0) FAIL(CLLM_E_INVALID, "dequantize_row: args");
    const int bs = cllm_blck_size(type);
    if (bs == 0 || k % bs) FAIL(CLLM_E_INVALID, "dequantize_row: k");
    // a 1-row table gathered with index 0
    static thread_local int32_t * zero_idx = nullptr;
    if (!zero_idx) { HIP_TRY(hipMalloc((void **) &zero_idx, 4)); HIP_TRY(hipMemset(zero_idx, 0, 4)); }
    cllm_tensor s = { type, {k, 1, 1, 1}, {cllm_type_size(type), cllm_row_size(type, k), cllm_row_size(type, k), cllm_row_size(type, k)}, (void *) blocks };
    cllm_tensor i = { CLLM_TYPE_I32, {1, 1, 1, 1}, {4, 4, 4, 4}, zero_idx };
    cllm_tensor d = { CLLM_TYPE_F32, {k, 1, 1, 1}, {4, (size_t) k*4, (size_t) k*4, (size_t) k*4}, y };
    return cllm_op_get_rows(stream, &s, &i, &d);
}

// ================================================================================================
// IM2COL    ggml_compute_forward_im2col_f16 / _f32, ops.cpp:6117-6283 (shape rule: ggml_im2col, ggml.c:4365-4407): the first node of ggml_conv_1d / _2d
//   dst[(n*OH*OW + oh*OW + ow) * (IC*KH*KW) + ic*KH*KW + kh*KW + kw] = src[n, ic, oh*s1 + kh*d1 - p1, ow*s0 + kw*d0 - p0], +0 outside the image
// Pure data movement with a KH*KW-fold expansion: the stores are the traffic.  A dst row (one output position) is cut into units of 16 bytes; a team of
// 2^tpr_shift consecutive lanes owns a row (256 >> tpr_shift rows per workgroup) and lane q of it the units q, q + team, ...: consecutive lanes store
// consecutive 16-byte pieces.  A row's (ow, oh, n) is split once per row (t_row_coord over dst), a unit's (ic, kh, kw) once per unit and then carried;
// the bounds test and the gather load come from the source plane.  A row that does not start on 16 bytes, and a row's leftover tail, store element by element.
// ================================================================================================
struct im2col_geom {
    int64_t IW, IH, KW, KH, RL, U, rows, ofs0, ofs1;      // RL = IC*KH*KW elements per dst row, U units per row; ofs0 / ofs1: the batch / channel stride in bytes
    int s0, s1, p0, p1, d0, d1, is_2d, tpr_shift;
};
// GGML_CPU_FP32_TO_FP16 of the reference's x86 build is the portable ggml_compute_fp32_to_fp16 (ggml-impl.h:401-425): round to nearest even, and every NaN becomes sign | 0x7e00
__device__ __forceinline__ uint16_t im2col_half(uint32_t w) {
    if ((w & 0x7fffffffu) > 0x7f800000u) return (uint16_t)(((w >> 16) & 0x8000u) | 0x7e00u);
    return f2h(__uint_as_float(w));
}
// TD: uint16_t (F16 dst) or uint32_t (F32 dst: the source word as it is).  The index inside a row is 32 bits wide (the entry declines rows of 2^31 elements or more:
// a kernel tensor of that size per output channel does not occur); rows, offsets and addresses are 64-bit
template <typename TD>
__global__ void __launch_bounds__(256) k_im2col(const char * __restrict__ src, tview d, im2col_geom G) {
    constexpr int VEC = 16 / (int) sizeof(TD);
    const int team = 1 << G.tpr_shift, rpb = 256 >> G.tpr_shift;
    const int lr = (int) threadIdx.x >> G.tpr_shift, q0 = (int) threadIdx.x & (team - 1);
    typedef uint32_t IX;
    const IX RL = (IX) G.RL, U = (IX) G.U, KW = (IX) G.KW, KH = (IX) G.KH, khkw = KH * KW;
    for (int64_t row = (int64_t) blockIdx.x * rpb + lr; row < G.rows; row += (int64_t) gridDim.x * rpb) {
        const tcoord c = t_row_coord(d, row);                  // dst is [RL, OW, OH, N] (2-D) or [RL, OW, N, 1] (1-D)
        const int64_t n = G.is_2d ? c.i3 : c.i2;
        const int64_t iw0 = c.i1 * G.s0 - G.p0, ih0 = (G.is_2d ? c.i2 : 0) * G.s1 - G.p1;
        const char * img = src + n * G.ofs0;
        TD * drow = (TD *) d.data + row * G.RL;
        const bool al16 = ((uintptr_t) drow & 15) == 0;
        for (IX q = (IX) q0; q < U; q += (IX) team) {
            const IX j = q * VEC;
            IX ic = j / khkw, kh = (j - ic * khkw) / KW, kw = j - ic * khkw - kh * KW;
            const int cnt = RL - j < (IX) VEC ? (int)(RL - j) : VEC;
            TD v[VEC];
#pragma unroll
            for (int e = 0; e < VEC; e++) {
                v[e] = 0;
                if (e < cnt) {
                    const int64_t iiw = iw0 + (int64_t) kw * G.d0, iih = ih0 + (int64_t) kh * G.d1;
                    if (iih >= 0 && iih < G.IH && iiw >= 0 && iiw < G.IW) {
                        const uint32_t w = *(const uint32_t *)(img + (int64_t) ic * G.ofs1 + (iih * G.IW + iiw) * 4);
                        if (sizeof(TD) == 2) v[e] = (TD) im2col_half(w); else v[e] = (TD) w;
                    }
                    if (++kw == KW) { kw = 0; if (++kh == KH) { kh = 0; ic++; } }
                }
            }
            TD * dp = drow + j;
            if (al16 && cnt == VEC) {
                u32x4 o;
                if (sizeof(TD) == 2) o = u32x4{ (uint32_t) v[0] | (uint32_t) v[1] << 16, (uint32_t) v[2] | (uint32_t) v[3] << 16, (uint32_t) v[4 % VEC] | (uint32_t) v[5 % VEC] << 16, (uint32_t) v[6 % VEC] | (uint32_t) v[7 % VEC] << 16 };
                else                 o = u32x4{ (uint32_t) v[0], (uint32_t) v[1], (uint32_t) v[2], (uint32_t) v[3] };
                *(u32x4 *) dp = o;
            } else {
#pragma unroll
                for (int e = 0; e < VEC; e++) if (e < cnt) dp[e] = v[e];
            }
        }
    }
}
static int64_t conv_out_size(int64_t ins, int64_t ks, int s, int p, int d) { return (ins + 2 * (int64_t) p - (int64_t) d * (ks - 1) - 1) / s + 1; }      // ggml_calc_conv_output_size
extern "C" int cllm_op_im2col(void * stream, const cllm_tensor * kernel, const cllm_tensor * src, cllm_tensor * dst, int s0, int s1, int p0, int p1, int d0, int d1, int is_2d) {
    if (!kernel || !src || !dst) FAIL(CLLM_E_INVALID, "im2col: null");
    if (src->type != CLLM_TYPE_F32 || (dst->type != CLLM_TYPE_F16 && dst->type != CLLM_TYPE_F32)) FAIL(CLLM_E_UNSUPPORTED, "im2col: type (F32 -> F16 | F32)");
    if (dst->type == CLLM_TYPE_F16 && kernel->type != CLLM_TYPE_F16) FAIL(CLLM_E_UNSUPPORTED, "im2col: type (an F16 dst takes an F16 kernel)");       // the reference's assert, ops.cpp:6200
    if (is_2d != 0 && is_2d != 1) FAIL(CLLM_E_INVALID, "im2col: is_2d");
    if (s0 <= 0 || d0 <= 0 || p0 < 0 || p1 < 0 || (is_2d && (s1 <= 0 || d1 <= 0))) FAIL(CLLM_E_INVALID, "im2col: stride, padding or dilation");
    if (src->nb[0] != 4) FAIL(CLLM_E_UNSUPPORTED, "im2col: rows must be dense");
    const int64_t IW = src->ne[0], IH = is_2d ? src->ne[1] : 1, IC = is_2d ? src->ne[2] : src->ne[1], N = is_2d ? src->ne[3] : src->ne[2];
    const int64_t KW = kernel->ne[0], KH = is_2d ? kernel->ne[1] : 1;
    if (is_2d ? kernel->ne[2] != src->ne[2] : (kernel->ne[1] != src->ne[1] || src->ne[3] != 1)) FAIL(CLLM_E_INVALID, "im2col: shape (kernel against src)");
    if (IW <= 0 || IH <= 0 || KW <= 0 || KH <= 0) FAIL(CLLM_E_INVALID, "im2col: shape");
    const int64_t OW = conv_out_size(IW, KW, s0, p0, d0), OH = is_2d ? conv_out_size(IH, KH, s1, p1, d1) : 1, RL = IC * KH * KW;
    if (OW <= 0 || OH <= 0) FAIL(CLLM_E_INVALID, "im2col: shape (src too small for the kernel)");
    if (dst->ne[0] != RL || dst->ne[1] != OW || dst->ne[2] != (is_2d ? OH : N) || dst->ne[3] != (is_2d ? N : 1)) FAIL(CLLM_E_INVALID, "im2col: shape (dst)");
    if (!t_is_contiguous(dst)) FAIL(CLLM_E_UNSUPPORTED, "im2col: dst must be contiguous");
    // the reference indexes a plane as iih*IW + iiw and keeps the channel and batch strides in an int (ops.cpp:6151-6152)
    if (is_2d && IH > 1 && src->nb[1] != (size_t) IW * 4) FAIL(CLLM_E_UNSUPPORTED, "im2col: the rows of a plane must be dense");
    const size_t ofs0 = is_2d ? src->nb[3] : src->nb[2], ofs1 = is_2d ? src->nb[2] : src->nb[1];
    if (ofs0 > 0x7fffffff || ofs1 > 0x7fffffff) FAIL(CLLM_E_UNSUPPORTED, "im2col: channel and batch strides beyond 2^31 - 1");
    if (((uintptr_t) src->data | ofs0 | ofs1) % 4 || (uintptr_t) dst->data % cllm_type_size(dst->type)) FAIL(CLLM_E_UNSUPPORTED, "im2col: alignment");
    if (RL > 0x7fffffff) FAIL(CLLM_E_UNSUPPORTED, "im2col: rows of 2^31 elements or more");
    const int64_t rows = OW * OH * N;
    if (rows == 0 || RL == 0) return CLLM_OK;
    const int vec = 16 / (int) cllm_type_size(dst->type);
    im2col_geom G = { IW, IH, KW, KH, RL, (RL + vec - 1) / vec, rows, (int64_t) ofs0, (int64_t) ofs1, s0, is_2d ? s1 : 0, p0, is_2d ? p1 : 0, d0, is_2d ? d1 : 0, is_2d, 0 };
    while (G.tpr_shift < 8 && ((int64_t) 1 << G.tpr_shift) < G.U) G.tpr_shift++;
    const dim3 grid(grid_1d(rows << G.tpr_shift, 16384));      // a team of 2^tpr_shift threads per row: 256 >> tpr_shift rows per workgroup
    hipStream_t st = (hipStream_t) stream;
    const char * sp = (const char *) src->data;
    if (dst->type == CLLM_TYPE_F16) hipLaunchKernelGGL((k_im2col<uint16_t>), grid, dim3(256), 0, st, sp, tv(dst), G);
    else                            hipLaunchKernelGGL((k_im2col<uint32_t>), grid, dim3(256), 0, st, sp, tv(dst), G);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// ================================================================================================
// POOL_1D / POOL_2D    ggml_compute_forward_pool_1d_ksp / _pool_2d, ops.cpp:7182-7352 (shape rules: ggml_pool_1d / _2d, ggml.c:4848-4911): avg_pool_1d / _2d of the
// audio and vision towers.  One thread per output element walks its window serially in the reference's order (ky outer, kx inner), skipping what lies outside the plane.
//   AVG: a float sum from 0.0f; the 1-D form divides by the number of positions inside (none: 0.0f), the 2-D form by (float)(k0*k1) always; IEEE division
//   MAX: from -FLT_MAX, std::max(v, res) = (v < res) ? res : v -- a NaN stays only while nothing follows it; a window of -inf alone, or wholly in the padding: -FLT_MAX
// The 1-D form is the 2-D one over planes of one row (k1 = s1 = 1, p1 = 0) with the other divisor.
// ================================================================================================
struct pool_geom { int64_t IW, IH, OW, OH, planes; int op, k0, k1, s0, s1, p0, p1, by_count; };
__global__ void __launch_bounds__(256) k_pool(const float * __restrict__ src, float * __restrict__ dst, pool_geom G) {
    const int64_t n = G.OW * G.OH * G.planes;
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t) gridDim.x * blockDim.x) {
        const int64_t ox = e % G.OW, oy = (e / G.OW) % G.OH, pl = e / (G.OW * G.OH);
        const float * plane = src + pl * G.IH * G.IW;
        const int64_t ix = ox * G.s0 - G.p0, iy = oy * G.s1 - G.p1;
        float res = G.op == CLLM_POOL_AVG ? 0.0f : -FLT_MAX;
        int count = 0;
        for (int ky = 0; ky < G.k1; ky++) {
            if (iy + ky < 0 || iy + ky >= G.IH) continue;
            const float * srow = plane + (iy + ky) * G.IW;
            for (int kx = 0; kx < G.k0; kx++) {
                const int64_t j = ix + kx;
                if (j < 0 || j >= G.IW) continue;
                const float v = srow[j];
                if (G.op == CLLM_POOL_AVG) res = res + v; else res = (v < res) ? res : v;
                count++;
            }
        }
        if (G.op == CLLM_POOL_AVG) {
            if (G.by_count) res = count > 0 ? __fdiv_rn(res, (float) count) : 0.0f;
            else            res = __fdiv_rn(res, (float)(G.k0 * G.k1));
        }
        dst[e] = res;
    }
}
// ggml_calc_pool_output_size: (ins + 2*p - ks) / s + 1 in float (p is a float there), truncated
static int64_t pool_out_size(int64_t ins, int ks, int s, int p) { return (int64_t)(((float) ins + 2.0f * (float) p - (float) ks) / (float) s + 1.0f); }
static int pool_launch(void * stream, const char * name, int op, const cllm_tensor * src, cllm_tensor * dst, int k0, int k1, int s0, int s1, int p0, int p1, bool is_2d) {
    if (!src || !dst) FAIL(CLLM_E_INVALID, "%s: null", name);
    if (src->type != CLLM_TYPE_F32 || dst->type != CLLM_TYPE_F32) FAIL(CLLM_E_UNSUPPORTED, "%s: type (F32 only)", name);
    if (op != CLLM_POOL_MAX && op != CLLM_POOL_AVG) FAIL(CLLM_E_INVALID, "%s: op %d", name, op);
    if (k0 <= 0 || k1 <= 0 || s0 <= 0 || s1 <= 0 || p0 < 0 || p1 < 0) FAIL(CLLM_E_INVALID, "%s: kernel, stride or padding", name);
    if (!t_is_contiguous(src) || !t_is_contiguous(dst)) FAIL(CLLM_E_UNSUPPORTED, "%s: src and dst must be contiguous", name);
    const int64_t IW = src->ne[0], IH = is_2d ? src->ne[1] : 1;
    // the reference walks a window in int (ops.cpp:7217, 7316-7317) and multiplies k0 * k1 in int
    if (IW + 2 * (int64_t) p0 + k0 > 0x7fffffff || IH + 2 * (int64_t) p1 + k1 > 0x7fffffff || (int64_t) k0 * k1 > 0x7fffffff) FAIL(CLLM_E_UNSUPPORTED, "%s: extent beyond 2^31 - 1", name);
    const int64_t OW = IW > 0 ? pool_out_size(IW, k0, s0, p0) : 0, OH = is_2d ? (IH > 0 ? pool_out_size(IH, k1, s1, p1) : 0) : 1;
    const bool empty = t_nelements(src) == 0;
    if (!empty && (OW <= 0 || OH <= 0)) FAIL(CLLM_E_INVALID, "%s: shape (src too small for the window)", name);
    if (dst->ne[0] != OW || dst->ne[1] != (is_2d ? OH : src->ne[1]) || dst->ne[2] != src->ne[2] || dst->ne[3] != src->ne[3]) FAIL(CLLM_E_INVALID, "%s: shape", name);
    if (empty || t_nelements(dst) == 0) return CLLM_OK;
    pool_geom G = { IW, IH, OW, OH, is_2d ? src->ne[2] * src->ne[3] : t_nrows(src), op, k0, k1, s0, s1, p0, p1, is_2d ? 0 : 1 };
    hipLaunchKernelGGL(k_pool, dim3(grid_1d(t_nelements(dst), 8192)), dim3(256), 0, (hipStream_t) stream, (const float *) src->data, (float *) dst->data, G);
    LAUNCH_CHECK();
    return CLLM_OK;
}
extern "C" int cllm_op_pool_1d(void * stream, int op, const cllm_tensor * src, cllm_tensor * dst, int k0, int s0, int p0) {
    return pool_launch(stream, "pool_1d", op, src, dst, k0, 1, s0, 1, p0, 0, false);
}
extern "C" int cllm_op_pool_2d(void * stream, int op, const cllm_tensor * src, cllm_tensor * dst, int k0, int k1, int s0, int s1, int p0, int p1) {
    return pool_launch(stream, "pool_2d", op, src, dst, k0, k1, s0, s1, p0, p1, true);
}

// ================================================================================================
// PAD / PAD_REFLECT_1D / UPSCALE / CONV_TRANSPOSE_1D: what the audio and vision front ends put around their convolutions (the left pad of a causal Conv1D, the
// Conformer's chunking, Conv1D's reflect padding, ggml::interpolate, the vocoder's ConvTransposed1D).  The destination of all four is contiguous.
// The two pads share k_im2col's store shape: a thread owns 4 consecutive words of a dst row (unit q of row r is item r * U + q of the 1-D walk, so consecutive lanes
// store consecutive 16-byte pieces); a row that does not start on 16 bytes, and a row's leftover tail, store word by word.  Words are moved as words: NaN payloads stay.
// ================================================================================================
__device__ __forceinline__ void pad_store4(uint32_t * dp, bool al16, int cnt, const uint32_t (&v)[4]) {
    if (al16 && cnt == 4) { *(u32x4 *) dp = u32x4{ v[0], v[1], v[2], v[3] }; return; }
#pragma unroll
    for (int e = 0; e < 4; e++) if (e < cnt) dp[e] = v[e];
}
// PAD       ggml_compute_forward_pad_f32<false>, ops.cpp:7696-7758 (shape rule: ggml_pad_ext, ggml.c:5016-5049): dst is addressed densely, the source through its four
// byte strides (nb00 too); inside [lp, ne - rp) on every axis the source word, +0.0f elsewhere
struct pad_geom { int64_t U; int lp0, lp1, lp2, lp3; };
__global__ void __launch_bounds__(256) k_pad(tview s, tview d, pad_geom G) {
    const int64_t n = G.U * d.ne[1] * d.ne[2] * d.ne[3];
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t) gridDim.x * blockDim.x) {
        const tcoord c = t_unit_coord(G.U, d, e);
        const int64_t j = c.i0 * 4;
        uint32_t * drow = (uint32_t *) d.data + (e / G.U) * d.ne[0];
        const tcoord sc = { 0, c.i1 - G.lp1, c.i2 - G.lp2, c.i3 - G.lp3 };
        const bool inside = sc.i1 >= 0 && sc.i1 < s.ne[1] && sc.i2 >= 0 && sc.i2 < s.ne[2] && sc.i3 >= 0 && sc.i3 < s.ne[3];
        const char * srow = t_row_at(s, inside ? sc : tcoord{ 0, 0, 0, 0 });
        const int cnt = d.ne[0] - j < 4 ? (int)(d.ne[0] - j) : 4;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int64_t i00 = j + k - G.lp0;
            v[k] = 0;
            if (k < cnt && inside && i00 >= 0 && i00 < s.ne[0]) v[k] = *(const uint32_t *)(srow + i00 * s.nb[0]);
        }
        pad_store4(drow + j, ((uintptr_t) drow & 15) == 0, cnt, v);
    }
}
extern "C" int cllm_op_pad(void * stream, const cllm_tensor * src, cllm_tensor * dst, int lp0, int rp0, int lp1, int rp1, int lp2, int rp2, int lp3, int rp3) {
    if (!src || !dst) FAIL(CLLM_E_INVALID, "pad: null");
    if (src->type != CLLM_TYPE_F32 || dst->type != CLLM_TYPE_F32) FAIL(CLLM_E_UNSUPPORTED, "pad: type (F32 only)");
    const int lp[4] = { lp0, lp1, lp2, lp3 }, rp[4] = { rp0, rp1, rp2, rp3 };
    for (int i = 0; i < 4; i++) if (lp[i] < 0 || rp[i] < 0) FAIL(CLLM_E_INVALID, "pad: negative padding");
    for (int i = 0; i < 4; i++) if (dst->ne[i] != src->ne[i] + lp[i] + rp[i]) FAIL(CLLM_E_INVALID, "pad: shape");
    if (!t_is_contiguous(dst)) FAIL(CLLM_E_UNSUPPORTED, "pad: dst must be contiguous");
    if (((uintptr_t) src->data | (uintptr_t) dst->data | src->nb[0] | src->nb[1] | src->nb[2] | src->nb[3]) % 4) FAIL(CLLM_E_UNSUPPORTED, "pad: alignment");
    if (t_nelements(dst) == 0) return CLLM_OK;
    pad_geom G = { (dst->ne[0] + 3) / 4, lp0, lp1, lp2, lp3 };
    hipLaunchKernelGGL(k_pad, dim3(grid_1d(G.U * t_nrows(dst), 16384)), dim3(256), 0, (hipStream_t) stream, tv(src), tv(dst), G);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// PAD_REFLECT_1D    ggml_compute_forward_pad_reflect_1d, ops.cpp:7784-7815 (shape rule and asserts: ggml_pad_reflect_1d, ggml.c:5072-5099):
//   a row is src[p0], .., src[1], src[0 .. ne00 - 1], src[ne00 - 2], .., src[ne00 - 1 - p1]; the reflected index is computed per word
__global__ void __launch_bounds__(256) k_pad_reflect_1d(tview s, tview d, int64_t U, int p0) {
    const int64_t n = U * d.ne[1] * d.ne[2] * d.ne[3];
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t) gridDim.x * blockDim.x) {
        const tcoord c = t_unit_coord(U, d, e);
        const int64_t j = c.i0 * 4;
        uint32_t * drow = (uint32_t *) d.data + (e / U) * d.ne[0];
        const uint32_t * srow = (const uint32_t *) t_row_at(s, c);
        const int cnt = d.ne[0] - j < 4 ? (int)(d.ne[0] - j) : 4;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int64_t i = j + k - p0;
            i = i < 0 ? -i : (i >= s.ne[0] ? 2 * (s.ne[0] - 1) - i : i);
            v[k] = 0;
            if (k < cnt) v[k] = srow[i];
        }
        pad_store4(drow + j, ((uintptr_t) drow & 15) == 0, cnt, v);
    }
}
extern "C" int cllm_op_pad_reflect_1d(void * stream, const cllm_tensor * src, cllm_tensor * dst, int p0, int p1) {
    if (!src || !dst) FAIL(CLLM_E_INVALID, "pad_reflect_1d: null");
    if (src->type != CLLM_TYPE_F32 || dst->type != CLLM_TYPE_F32) FAIL(CLLM_E_UNSUPPORTED, "pad_reflect_1d: type (F32 only)");
    if (p0 < 0 || p1 < 0) FAIL(CLLM_E_INVALID, "pad_reflect_1d: negative padding");
    if (p0 >= src->ne[0] || p1 >= src->ne[0]) FAIL(CLLM_E_INVALID, "pad_reflect_1d: padding must be smaller than the row");      // the constructor's asserts
    if (dst->ne[0] != src->ne[0] + p0 + p1 || dst->ne[1] != src->ne[1] || dst->ne[2] != src->ne[2] || dst->ne[3] != src->ne[3]) FAIL(CLLM_E_INVALID, "pad_reflect_1d: shape");
    if (!t_is_contiguous(src) || !t_is_contiguous(dst)) FAIL(CLLM_E_UNSUPPORTED, "pad_reflect_1d: src and dst must be contiguous");
    if (((uintptr_t) src->data | (uintptr_t) dst->data) % 4) FAIL(CLLM_E_UNSUPPORTED, "pad_reflect_1d: alignment");
    if (t_nelements(dst) == 0) return CLLM_OK;
    const int64_t U = (dst->ne[0] + 3) / 4;
    hipLaunchKernelGGL(k_pad_reflect_1d, dim3(grid_1d(U * t_nrows(dst), 16384)), dim3(256), 0, (hipStream_t) stream, tv(src), tv(dst), U, p0);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// UPSCALE   ggml_compute_forward_upscale_f32, ops.cpp:7478-7672, its NEAREST and plain BILINEAR branches (what ggml::interpolate emits: no align-corners, no antialias).
//   sf_k = (float) ne_k / ne0k (a float division, done once on the host); one thread per dst element; the source through its four byte strides.
//   NEAREST:  i0k = (int64_t)(i_k / sf_k) on all four axes: the IEEE quotient, truncated
//   BILINEAR: axes 2 and 3 as in NEAREST; on axes 0 and 1 x = ((float) i + 0.5f) / sf - 0.5f, x0 = floorf(x), x1 = x0 + 1, both clamped to [0, ne0k - 1], dx = x - (float)(the
//             clamped x0) clamped to [0, 1] by std::max(0.0f, std::min(dx, 1.0f)).  a*(1-dx)*(1-dy) + b*dx*(1-dy) + c*(1-dx)*dy + d*dx*dy as gcc -O2 -march=x86-64-v3
//             compiles it (read from libggml-cpu.so, pinned by tests/test_resample_model.py): the four products with dx / (1 - dx) are rounded, b's product with (1 - dy)
//             is rounded too, and the other three enter as fmas in the order a, c, d.
// An index is kept inside the source where float rounding could carry the reference's own past its end (ne beyond 2^23): no word changes where the reference reads inside.
struct upscale_geom { float sf0, sf1, sf2, sf3; };
__device__ __forceinline__ int64_t upscale_near(int64_t i, float sf, int64_t ne) { const int64_t k = (int64_t) __fdiv_rn((float) i, sf); return k < ne ? k : ne - 1; }
__device__ __forceinline__ void upscale_lin(int64_t i, float sf, int64_t ne, int64_t & k0, int64_t & k1, float & dk) {
    const float x = __fdiv_rn((float) i + 0.5f, sf) - 0.5f;
    k0 = (int64_t) floorf(x); k1 = k0 + 1;
    k0 = k0 > ne - 1 ? ne - 1 : k0; k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > ne - 1 ? ne - 1 : k1; k1 = k1 < 0 ? 0 : k1;
    dk = x - (float) k0;
    dk = 1.0f < dk ? 1.0f : dk;          // std::min(dk, 1.0f)
    dk = 0.0f < dk ? dk : 0.0f;          // std::max(0.0f, .)
}
template <int MODE>      // 0: NEAREST, 1: BILINEAR (== enum ggml_scale_mode)
__global__ void __launch_bounds__(256) k_upscale(tview s, tview d, upscale_geom G) {
    const int64_t n = d.ne[0] * d.ne[1] * d.ne[2] * d.ne[3];
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t) gridDim.x * blockDim.x) {
        const tcoord c = t_elem_coord(d, e);
        const char * plane = s.data + upscale_near(c.i2, G.sf2, s.ne[2]) * s.nb[2] + upscale_near(c.i3, G.sf3, s.ne[3]) * s.nb[3];
        if (MODE == 0) {
            ((uint32_t *) d.data)[e] = *(const uint32_t *)(plane + upscale_near(c.i0, G.sf0, s.ne[0]) * s.nb[0] + upscale_near(c.i1, G.sf1, s.ne[1]) * s.nb[1]);
        } else {
            int64_t x0, x1, y0, y1; float dx, dy;
            upscale_lin(c.i0, G.sf0, s.ne[0], x0, x1, dx);
            upscale_lin(c.i1, G.sf1, s.ne[1], y0, y1, dy);
            const float a = *(const float *)(plane + x0 * s.nb[0] + y0 * s.nb[1]), b = *(const float *)(plane + x1 * s.nb[0] + y0 * s.nb[1]);
            const float cc = *(const float *)(plane + x0 * s.nb[0] + y1 * s.nb[1]), dd = *(const float *)(plane + x1 * s.nb[0] + y1 * s.nb[1]);
            const float mx = 1.0f - dx, my = 1.0f - dy;
            float v = (b * dx) * my;
            v = __builtin_fmaf(a * mx, my, v);
            v = __builtin_fmaf(cc * mx, dy, v);
            v = __builtin_fmaf(dd * dx, dy, v);
            ((float *) d.data)[e] = v;
        }
    }
}
extern "C" int cllm_op_upscale(void * stream, const cllm_tensor * src, cllm_tensor * dst, int mode_flags) {
    if (!src || !dst) FAIL(CLLM_E_INVALID, "upscale: null");
    if (src->type != CLLM_TYPE_F32 || dst->type != CLLM_TYPE_F32) FAIL(CLLM_E_UNSUPPORTED, "upscale: type (F32 only)");
    if (mode_flags != 0 && mode_flags != 1) FAIL(CLLM_E_UNSUPPORTED, "upscale: mode %#x (NEAREST and BILINEAR without flags only)", (unsigned) mode_flags);
    if (!t_is_contiguous(dst)) FAIL(CLLM_E_UNSUPPORTED, "upscale: dst must be contiguous");
    if (((uintptr_t) src->data | (uintptr_t) dst->data | src->nb[0] | src->nb[1] | src->nb[2] | src->nb[3]) % 4) FAIL(CLLM_E_UNSUPPORTED, "upscale: alignment");
    for (int i = 0; i < 4; i++) if (dst->ne[i] < 0 || src->ne[i] < 0) FAIL(CLLM_E_INVALID, "upscale: shape");
    if (t_nelements(dst) == 0) return CLLM_OK;
    if (t_nelements(src) == 0) FAIL(CLLM_E_INVALID, "upscale: shape (an empty source)");
    const upscale_geom G = { (float) dst->ne[0] / src->ne[0], (float) dst->ne[1] / src->ne[1], (float) dst->ne[2] / src->ne[2], (float) dst->ne[3] / src->ne[3] };
    const dim3 grid(grid_1d(t_nelements(dst), 16384));
    if (mode_flags == 0) hipLaunchKernelGGL(k_upscale<0>, grid, dim3(256), 0, (hipStream_t) stream, tv(src), tv(dst), G);
    else                 hipLaunchKernelGGL(k_upscale<1>, grid, dim3(256), 0, (hipStream_t) stream, tv(src), tv(dst), G);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// CONV_TRANSPOSE_1D     ggml_compute_forward_conv_transpose_1d_f16_f32 / _f32, ops.cpp:5915-6089 (shape rule and asserts: ggml_conv_transpose_1d, ggml.c:4501-4529).
//   kernel a [K, Cout, Cin] F16 | F32, data b [L, Cin] F32, dst [(L - 1) * s0 + K, Cout] F32.  Per output row oc, from +0.0f: for i10 ascending, for every tap i00:
//   dst[oc][i10 * s0 + i00] += v(oc, i10, i00), v = ggml_vec_dot_f16 (the data rounded to fp16 first) or ggml_vec_dot_f32 over Cin.
// One lane per output element (oc, t): it walks the i10 with 0 <= t - i10 * s0 < K ascending and adds their dot products in plain float adds; the reference's 32
// accumulators (accumulator a takes ci = a, a + 32, ..., one fma each), GGML_F32x8_REDUCE's tree and the Cin mod 32 leftovers all in that lane's registers: matmul_f.hip's
// VD order, in-lane.  No atomics, no zero-fill pass, no workspace, no repack: neighbouring lanes (neighbouring t, the same i10) read neighbouring taps a[i00, oc, ci] and
// the same data word b[i10, ci].
// ================================================================================================
template <typename T> __device__ __forceinline__ float ct1d_tap(const char * p);                // a kernel element, widened
template <> __device__ __forceinline__ float ct1d_tap<uint16_t>(const char * p) { return h2f(*(const uint16_t *) p); }
template <> __device__ __forceinline__ float ct1d_tap<float>(const char * p)    { return *(const float *) p; }
template <typename T> __device__ __forceinline__ float ct1d_dat(const char * p);                // a data element as the dot product sees it: F16 kernel -> fp16 (RNE) -> fp32
template <> __device__ __forceinline__ float ct1d_dat<uint16_t>(const char * p) { return h2f(f2h(*(const float *) p)); }
template <> __device__ __forceinline__ float ct1d_dat<float>(const char * p)    { return *(const float *) p; }
template <typename T>
__global__ void __launch_bounds__(256) k_conv_transpose_1d(tview a, tview b, tview d, int s0) {
    const int64_t K = a.ne[0], Cin = a.ne[2], L = b.ne[0], OL = d.ne[0], n = OL * d.ne[1], np = Cin & ~(int64_t) 31;
    for (int64_t e = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t) gridDim.x * blockDim.x) {
        const int64_t t = e % OL, oc = e / OL;
        const int64_t lo = t >= K ? (t - K) / s0 + 1 : 0, hi = t / s0 < L - 1 ? t / s0 : L - 1;       // the i10 whose taps reach t
        float out = 0.0f;
        for (int64_t i10 = lo; i10 <= hi; i10++) {
            const char * ap = a.data + (t - i10 * s0) * (int64_t) sizeof(T) + oc * a.nb[1];
            const char * bp = b.data + i10 * 4;
            float acc[32];
#pragma unroll
            for (int j = 0; j < 32; j++) acc[j] = 0.0f;
            for (int64_t c0 = 0; c0 < np; c0 += 32) {
#pragma unroll
                for (int j = 0; j < 32; j++) acc[j] = __builtin_fmaf(ct1d_dat<T>(bp + (c0 + j) * b.nb[1]), ct1d_tap<T>(ap + (c0 + j) * a.nb[2]), acc[j]);
            }
            // GGML_F32x8_REDUCE (simd-mappings.h:549-567) over accumulator 8 r + l of register r: x0 += x2, x1 += x3; x0 += x1; low half + high half; hadd, hadd
            float h[4];
#pragma unroll
            for (int l = 0; l < 4; l++) h[l] = ((acc[l] + acc[16 + l]) + (acc[8 + l] + acc[24 + l])) + ((acc[4 + l] + acc[20 + l]) + (acc[12 + l] + acc[28 + l]));
            float u = (h[0] + h[1]) + (h[2] + h[3]);
            if (sizeof(T) == 2) {
                double sd = (double) u;           // ggml_vec_dot_f16's leftovers: float products added in double, rounded once
                for (int64_t ci = np; ci < Cin; ci++) sd += (double)(ct1d_dat<T>(bp + ci * b.nb[1]) * ct1d_tap<T>(ap + ci * a.nb[2]));
                u = (float) sd;
            } else {
                // ggml_vec_dot_f32's `sumf += x[i]*y[i]` as gcc compiles it (matmul_f.hip:93-103): whole groups of 4 as rounded products added in order, the scalar rest as fmas
                int64_t ci = np;
                for (; ci + 4 <= Cin; ci += 4) for (int l = 0; l < 4; l++) u = u + ct1d_dat<T>(bp + (ci + l) * b.nb[1]) * ct1d_tap<T>(ap + (ci + l) * a.nb[2]);
                for (; ci < Cin; ci++) u = __builtin_fmaf(ct1d_dat<T>(bp + ci * b.nb[1]), ct1d_tap<T>(ap + ci * a.nb[2]), u);
            }
            out = out + u;
        }
        ((float *) d.data)[e] = out;
    }
}
extern "C" int cllm_op_conv_transpose_1d(void * stream, const cllm_tensor * kernel, const cllm_tensor * data, cllm_tensor * dst, int s0) {
    if (!kernel || !data || !dst) FAIL(CLLM_E_INVALID, "conv_transpose_1d: null");
    if ((kernel->type != CLLM_TYPE_F16 && kernel->type != CLLM_TYPE_F32) || data->type != CLLM_TYPE_F32 || dst->type != CLLM_TYPE_F32)
        FAIL(CLLM_E_UNSUPPORTED, "conv_transpose_1d: type (F16 | F32 kernel, F32 data and dst)");
    if (s0 <= 0) FAIL(CLLM_E_INVALID, "conv_transpose_1d: stride");
    const size_t es = cllm_type_size(kernel->type);
    if (kernel->nb[0] != es || data->nb[0] != 4) FAIL(CLLM_E_UNSUPPORTED, "conv_transpose_1d: rows must be dense");      // the reference's asserts on nb00 and nb10
    const int64_t K = kernel->ne[0], Cout = kernel->ne[1], Cin = kernel->ne[2], L = data->ne[0];
    if (kernel->ne[3] != 1 || data->ne[2] != 1 || data->ne[3] != 1 || data->ne[1] != Cin || K < 0 || Cout < 0 || Cin < 0 || L < 0) FAIL(CLLM_E_INVALID, "conv_transpose_1d: shape (kernel against data)");
    if (dst->ne[0] != (L - 1) * s0 + K || dst->ne[1] != Cout || dst->ne[2] != 1 || dst->ne[3] != 1) FAIL(CLLM_E_INVALID, "conv_transpose_1d: shape (dst)");
    if (!t_is_contiguous(dst)) FAIL(CLLM_E_UNSUPPORTED, "conv_transpose_1d: dst must be contiguous");
    if (((uintptr_t) kernel->data | kernel->nb[1] | kernel->nb[2]) % es || ((uintptr_t) data->data | (uintptr_t) dst->data | data->nb[1]) % 4) FAIL(CLLM_E_UNSUPPORTED, "conv_transpose_1d: alignment");
    if (t_nelements(dst) == 0) return CLLM_OK;
    const dim3 grid(grid_1d(t_nelements(dst), 16384));
    hipStream_t st = (hipStream_t) stream;
    if (kernel->type == CLLM_TYPE_F16) hipLaunchKernelGGL((k_conv_transpose_1d<uint16_t>), grid, dim3(256), 0, st, tv(kernel), tv(data), tv(dst), s0);
    else                               hipLaunchKernelGGL((k_conv_transpose_1d<float>),    grid, dim3(256), 0, st, tv(kernel), tv(data), tv(dst), s0);
    LAUNCH_CHECK();
    return CLLM_OK;
}
