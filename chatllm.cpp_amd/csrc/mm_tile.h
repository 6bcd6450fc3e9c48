// mm_tile.h -- what the three quantized prefill tile GEMMs share: k_mmq (mmq.hip, fast mode), k_mmx (mmx.hip, the exact order) and k_mmd (dense_f16.hip, f16 mode).
// The argument struct and its fill, the raw weight-block fetches, the nibble split and byte -> fp16 helpers, the activation fetches of the 32-block types, the
// epilogue store and the launch tail.  Tile shapes, LDS maps, the unpack into LDS and the K loops stay with each kernel.
#pragma once
#include "common.h"
#include "q4k_scales.h"

typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct mm_tile_args {
    const char * W; int64_t nb01; int64_t N; int64_t K;
    const char * act; size_t act_stride; int64_t M;      // k_mmq / k_mmx: the quantized act rows (common.h); k_mmd: its fp16 copy of the activations (stride in bytes)
    float * dst; int64_t ldd;              // dst[m * ldd + n]
    const float * resid; int64_t ldr;      // optional: dst = acc + resid[m * ldr + n] (the MUL_MAT -> ADD pair; resid may be dst itself)
    int epi;                               // 1: weight rows alternate gate_u, up_u; dst[m * ldd + u] = silu(acc[2u]) * acc[2u + 1]  (UNARY(SILU) -> MUL of BaseMLP::forward)
};
// the launchers' shared front: dst rows a whole number of floats apart; epilogue 1 over row pairs only and without a residual
static inline int mm_tile_args_of(mm_tile_args & a, const char * name, const tview & w, const void * act, size_t act_stride, int64_t M, const tview & d,
                                  const float * resid, int64_t ldr, int epi) {
    if (d.nb[1] % 4) FAIL(CLLM_E_INVALID, "%s: dst stride", name);
    a.W = w.data; a.nb01 = w.nb[1]; a.N = w.ne[1]; a.K = w.ne[0];
    a.act = (const char *) act; a.act_stride = act_stride; a.M = M;
    a.dst = (float *) d.data; a.ldd = d.nb[1] / 4; a.resid = resid; a.ldr = ldr; a.epi = epi;
    if (epi && (epi != 1 || resid || a.N % 2)) FAIL(CLLM_E_INVALID, "%s: epilogue %d", name, epi);
    return CLLM_OK;
}

// the launch tail: KERNEL over tiles_m x tiles_n workgroups (a 1-D grid, common.h gemm_tile_of), its dynamic LDS allowed once per device and kernel instantiation
template <void (*KERNEL)(const mm_tile_args)>
static int mm_tile_launch(int64_t tiles_m, int64_t tiles_n, int threads, int lds, hipStream_t st, const mm_tile_args & a, const char * name) {
    static uint64_t attr = 0;
    if (tiles_m * tiles_n > 0x7fffffff) FAIL(CLLM_E_UNSUPPORTED, "%s: too many tiles", name);
    if (const int rc = lds_opt_in(KERNEL, attr, lds)) return rc;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)(tiles_m * tiles_n)), dim3(threads), lds, st, a);
    LAUNCH_CHECK();
    return CLLM_OK;
}

// ---- weights: raw fetches (nothing converted: a conversion behind the loads would make a prefetch wait for them) ----
// one Q4_0 / Q4_1 / Q8_0 block at bp: q = its first 16 quant bytes, q2 = Q8_0's second 16 (else zero), d = the raw fp16 d (Q4_1: d | m << 16)
struct wblock32_raw { u32x4 q, q2; uint32_t d; };
template <int TYPE> __device__ __forceinline__ wblock32_raw wblock32_load(const char * bp) {
    constexpr bool IS_41 = TYPE == CLLM_TYPE_Q4_1;
    struct __attribute__((packed, aligned(2))) q16 { uint32_t x, y, z, w; };
    wblock32_raw r;
    if (IS_41) r.d = *(const uint32_t *) bp; else r.d = *(const uint16_t *) bp;
    const q16 q0 = *(const q16 *)(bp + (IS_41 ? 4 : 2));
    r.q = u32x4{q0.x, q0.y, q0.z, q0.w}; r.q2 = u32x4{0, 0, 0, 0};
    if (TYPE == CLLM_TYPE_Q8_0) { const q16 q1 = *(const q16 *)(bp + 18); r.q2 = u32x4{q1.x, q1.y, q1.z, q1.w}; }
    return r;
}
// 64-weight chunk c of the Q4_K super-block at bp: the header {d, dmin, 12 packed scale / min bytes} and the chunk's 32 quant bytes
struct wchunk_q4k { u32x4 h, q, q2; };
__device__ __forceinline__ wchunk_q4k wchunk_q4k_load(const char * bp, int c) {
    return wchunk_q4k{ *(const u32x4 *) bp, *(const u32x4 *)(bp + 16 + 32 * c), *(const u32x4 *)(bp + 32 + 32 * c) };
}
// the low / high nibbles of 16 bytes, one per byte
__device__ __forceinline__ u32x4 nib_lo(u32x4 x) { return x & 0x0f0f0f0fu; }
__device__ __forceinline__ u32x4 nib_hi(u32x4 x) { return (x >> 4) & 0x0f0f0f0fu; }

// ---- bytes -> fp16.  Four bytes (unsigned, one per byte of u) -> fp16 pairs 1024 + byte: (elements 0, 1), (elements 2, 3).  0x64uu is the fp16 1024 + uu (ulp 1 in [1024, 2048))
__device__ __forceinline__ void bytes_to_h1024(uint32_t u, uint32_t & lo, uint32_t & hi) {
    lo = __builtin_amdgcn_perm(0x64646464u, u, 0x04010400u);
    hi = __builtin_amdgcn_perm(0x64646464u, u, 0x04030402u);
}
__device__ __forceinline__ uint32_t h2_sub(uint32_t x, uint32_t c) {          // per fp16 half: x - c
    const h2v r = __builtin_bit_cast(h2v, x) - __builtin_bit_cast(h2v, c);
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t h2_mul(uint32_t x, uint32_t c) {          // per fp16 half: x * c
    const h2v r = __builtin_bit_cast(h2v, x) * __builtin_bit_cast(h2v, c);
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t h2_fma(uint32_t x, uint32_t a, uint32_t c) {   // per fp16 half: x * a + c, one rounding
    const h2v r = __builtin_elementwise_fma(__builtin_bit_cast(h2v, x), __builtin_bit_cast(h2v, a), __builtin_bit_cast(h2v, c));
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t h2_splat16(uint16_t h) { return (uint32_t) h * 0x00010001u; }      // fp16 bits in both halves
__device__ __forceinline__ uint32_t h2_splat(float v) { const _Float16 h = (_Float16) v; uint16_t b; __builtin_memcpy(&b, &h, 2); return h2_splat16(b); }

// ---- activations of the 32-block types (act rows, common.h), zero outside M / K.  CPR 16-byte chunks of int8 per token and stage; NBK 32-blocks per stage ----
// task c = (token c / CPR of the tile at m0, chunk c % CPR of the stage at k0)
template <int CPR> __device__ __forceinline__ u32x4 act_chunk_load(const mm_tile_args & a, int64_t m0, int64_t k0, int c) {
    const int row = c / CPR, ch = c % CPR;
    const int64_t m = m0 + row;
    u32x4 v = u32x4{0, 0, 0, 0};
    if (m < a.M && k0 + ch * 16 < a.K) v = *(const u32x4 *)(a.act + m * a.act_stride + k0 + ch * 16);
    return v;
}
// task c = (token c % BM, plane c / BM) of the plane-major scale words: dx[NBK][m], then (Q4_1) sx[NBK][m], the f32 s plane
template <int BM, int NBK> __device__ __forceinline__ uint32_t act_scale_load(const mm_tile_args & a, int64_t m0, int64_t k0, int64_t act_d, int64_t act_s, int c) {
    const int row = c % BM, pl = c / BM, sb = pl % NBK;
    const int64_t m = m0 + row;
    uint32_t v = 0;
    if (m < a.M && k0 + sb * 32 < a.K) v = *(const uint32_t *)(a.act + m * a.act_stride + (pl < NBK ? act_d : act_s) + ((k0 / 32) + sb) * 4);
    return v;
}

// ---- the epilogue: mm_tile_store<FORM> st(a, lane), made once in front of a kernel's store loops; st(m, n, v) stores one accumulator value v of output (token m, weight row n) ----
//   MM_STORE_PLAIN    dst[m][n] = v
//   MM_STORE_RESID    dst[m][n] = v + resid[m][n] where a residual is given (else plain)
//   MM_STORE_SILU_UP  the lane pair (2u, 2u + 1) holds gate_u and up_u of the same tokens (n = the kernel's row of lane `lane`, consecutive over a quad): the even lane takes
//                     its neighbour's value and stores dst[m][u] = silu(gate) * up -- ggml_vec_silu_f32 over rows of N / 2 features: the polynomial body below nv, the libm
//                     tail from there.  Every lane of the wave must call it (the DPP read needs its source lane active).
// (nv is formed where the object is made, not per value: k_mmq sits at the VGPR limit and its register allocation follows the place of that statement)
enum { MM_STORE_PLAIN = 0, MM_STORE_RESID = 1, MM_STORE_SILU_UP = 2 };
template <int FORM> struct mm_tile_store {
    const mm_tile_args & a; const int lane; const int64_t nv;
    __device__ __forceinline__ mm_tile_store(const mm_tile_args & a_, int lane_) : a(a_), lane(lane_), nv((a_.N / 2) & ~(int64_t) 7) {}
    __device__ __forceinline__ void operator()(int64_t m, int64_t n, float v) const {
        if (FORM == MM_STORE_SILU_UP) {
            const int64_t u = n >> 1;
            const float up = dpp_f<DPP_QUAD_XOR1>(v);
            if (!(lane & 1) && n + 1 < a.N && m < a.M) a.dst[m * a.ldd + u] = silu_any(v, u < nv) * up;
        } else if (n < a.N && m < a.M) a.dst[m * a.ldd + n] = (FORM == MM_STORE_RESID && a.resid) ? v + a.resid[m * a.ldr + n] : v;
    }
};
