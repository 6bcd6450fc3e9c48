// fattn.h -- what the flash attention kernels share (fattn.hip: head sizes 64 / 128; fattn_hs.hip: 96 / 256): the launch arguments, the MFMA row
// mapping, the lane-pair reductions and the split-KV merge.
#pragma once
#include "attn_token.h"      // k_slot, v_slot: the cache layouts k_rope_kv_prep writes
#include <stdlib.h>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float    f32x16 __attribute__((ext_vector_type(16)));

#define FA_VSTR 136                  // bytes per V^T row in LDS: 64 positions * 2 B + 8 B (conflict-free ds_read_b64 over 32 rows)
#define FA_LOG2E 1.4426950408889634f
#ifndef FA_PD
#define FA_PD 4                      // LDS fragment reads are issued this many MFMAs ahead (2 and 8 measured the same: the loop is not latency-bound any more)
#endif
#define FA_TAU 8.0f                  // lazy soft-max reference: rescale only when a maximum grows by more than 2^8
#define FA_MAX_SPLITS 256            // split-KV decode: at most this many partials per (head, query)

struct fattn_args {
    const char * q; int64_t q_nb1, q_nb2, q_nb3;            // F32 [D, N, H, B]
    const char * k; int64_t k_nb1, k_nb2, k_nb3;            // [D, n_kv, Hkv, B] rows (F16 | Q8_0)
    const char * v; int64_t v_nb1, v_nb2, v_nb3;            // VL 0: [D, n_kv, Hkv, B] rows;  VL 1: [n_kv, D, Hkv, B] (F16, nb1 = bytes per dv row)
    const char * mask; int64_t m_nb1, m_nb2, m_nb3;         // F16 [n_kv, N, ne2, ne3]
    int m_ne2, m_ne3, m_al;                                 // m_al: rows are 8-byte aligned and n_kv % 4 == 0
    char * dst; int64_t d_nbn, d_nbh, d_nbb;                // F32 element (dv, h, n, b) at dst + n d_nbn + h d_nbh + b d_nbb + 4 dv
    float * part;                                           // splits > 1: [B][H][N][splits][D + 4] = O (unnormalized), m (log2 domain), l
    int N, H, Hkv, R, n_kv, n_past, splits, chunk;
    const int32_t * n_kv_dev;                               // decode inside a captured step: the number of cached positions is *n_kv_dev + 1 (n_kv: the upper bound)
    float sc2;                                              // scale * log2(e)
};

__device__ __forceinline__ int fa_crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// max over the two lanes (l31, 0) and (l31, 1) of a query row
__device__ __forceinline__ float fa_pair_max(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float fa_pair_sum(float x) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// merge the split-KV partials of one (b, h, n) (ggml_flash_attn_ext_reduce_partials, ops.cpp:8642-8710): 1024 threads = D output elements x
// G = 1024 / D interleaved groups of splits, so that the loads of different splits are independent and coalesced.  D = 96: G = 10, and the last
// 64 threads (a partial eleventh group) take part in the two reductions over the splits only
template <int D>
__global__ void __launch_bounds__(1024) k_fattn_merge(const fattn_args a) {
    constexpr int G = 1024 / D;
    __shared__ float red[1024];
    __shared__ float wgt[FA_MAX_SPLITS];
    __shared__ float Lsh;
    const int tid = threadIdx.x, dv = tid % D, g = tid / D, n = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const float * pp = a.part + (((int64_t) b * a.H + h) * a.N + n) * a.splits * (D + 4);
    float m = tid < a.splits ? pp[(int64_t) tid * (D + 4) + D] : -INFINITY, l = tid < a.splits ? pp[(int64_t) tid * (D + 4) + D + 1] : 0.0f;
    red[tid] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]); __syncthreads(); }      // splits <= 256
    const float M = red[0], Ms = M == -INFINITY ? 0.0f : M;
    __syncthreads();
    const float w = tid < a.splits ? __builtin_amdgcn_exp2f(m - Ms) : 0.0f;
    if (tid < FA_MAX_SPLITS) wgt[tid] = w;
    red[tid] = w * l;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) Lsh = red[0];
    __syncthreads();
    const float L = Lsh;
    __syncthreads();
    float acc = 0.0f;
    const int s_end = 1024 % D == 0 || g < G ? a.splits : 0;
#pragma unroll 4
    for (int s = g; s < s_end; s += G) acc += wgt[s] * pp[(int64_t) s * (D + 4) + dv];
    red[tid] = acc;
    __syncthreads();
    if (g == 0) {
#pragma unroll
        for (int k = 1; k < G; k++) acc += red[dv + k * D];
        const float inv = L == 0.0f ? 0.0f : 1.0f / L;
        float * dp = (float *)(a.dst + (int64_t) n * a.d_nbn + (int64_t) h * a.d_nbh + (int64_t) b * a.d_nbb);
        dp[dv] = acc * inv;
    }
}

// fattn_hs.hip: the head sizes 96 / 256 (V rows by position only); a, decode: as launch_fattn planned them
int fattn_hs_launch(hipStream_t st, const fattn_args & a, int D, int ktype, int mmode, int B, bool decode);
