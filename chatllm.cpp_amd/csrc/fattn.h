// fattn.h -- the flash attention kernel, stated once for every head size: GGML_OP_FLASH_ATTN_EXT and the same tiled kernel behind the prefill attention
// block and the long-context decode step.  The score matrix never leaves the CU.  fattn.hip instantiates head sizes 64 / 128 and holds the entry
// points; fattn_hs.hip instantiates 96 / 256, fattn_pad.hip 112, fattn_cap.hip the logit soft-cap (CAP) at 128 / 256.
//
//   out[:, h, n] = sum_kv softmax_kv(scale * K[kv, h/r] . Q[n, h] + mask[kv, n]) * V[kv, h/r]
//   ggml_compute_forward_flash_attn_ext_f16 (ggml-cpu/ops.cpp:8114-8344 one query at a time, :8346-8640 tiled, :8642-8710 the
//   split-KV reduction); used by CoreAttention with `-fa` (src/layers.cpp:2634-2656) over the K / V caches of
//   src/layers.cpp:2925-2945 (F16, or Q8_0 with --cache_dtype q8_0).
//
// Numerics: TOLERANCE tier (tests/fattn_model.py bounds it per element).  The CPU op itself has three summation orders (one_chunk / tiled / split-KV,
// chosen by shape and thread count), so there is no single bit pattern to match.  What is kept from the CPU path: Q is converted to K's
// vec_dot_type first (F16 K: rounded to fp16; Q8_0 K: quantize_row_q8_0, i.e. the 8-bit rounding of Q is reproduced), K / V
// are used at their stored precision, products are exact in fp32, the soft-max runs in fp32 (online, base 2), a row that sees nothing is exact zeros.
// What differs: P is rounded to fp16 before the P.V product (the CPU keeps it in fp32 but accumulates V in fp16 for an F16 cache), and
// accumulation is in MFMA order.  K / V are walked in tiles of 64 positions at every head size: one possible rescale per 64 positions, so term (c)
// of the model's bound ((2.5 n_in + 2 tiles_per_chunk + 5) u A) counts the kernel's roundings one for one, and launch_fattn's chunk / splits
// describe every head size alike.
//
// One kernel, v_mfma_f32_32x32x16_f16, "swapped" form so that every soft-max quantity of a query row lives in one lane pair:
//   S^T[kv, q] = K[kv, :] . Q[q, :]      A = K tile (LDS, fa_k_layout<D>), B = Q (registers, loaded once)
//   lane (l31, hi) holds S^T[kv = crow(r, hi) + 32 j, q = l31], crow(r, hi) = (r & 3) + 8 (r >> 2) + 4 hi
//   O^T[dv, q] += Vt[dv, kv] . P^T[kv, q]  A = V^T tile (LDS, [dv][kv] rows), B = P: exactly the registers the lane already
//   holds (the contraction order of an MFMA is free as long as A and B agree), so P never moves between lanes.
// A workgroup is 4 waves x 32 query rows over one (kv head | head); K/V tiles of 64 positions are staged through LDS by all
// waves.  Decode (few rows): the r heads of a GQA group are packed as rows of one tile (R = r) so K/V are read once per
// group, one wave computes while all four stage (one load latency), and the positions are split over gridDim.x workgroups whose partial
// (m, l, O) are merged by k_fattn_merge.
//
// What depends on the head size is stated once each: the K tile's LDS layout (fa_k_layout), the tile-ahead prefetch and the occupancy
// (fa_tile_ahead, fa_min_blocks), the V^T-cache form (fa_has_vt), the grouping of the Q conversion (fa_q_group), the K staging's guard (fa_k_guard)
// and the feature rows of the P.V product (fa_dp).
//
// D = 112, and with it every D % 32 == 16; the figures below are given for 80 / 112, but 80 is NOT instantiated (tests/test_gpu_fattn.py holds it as the
//   head size the entry declines).  F16 rows only: a Q8_0 row needs D % 32 == 0, and the host gives such a head size an F16 cache.  The two products
//   stop sharing a block count.  S^T contracts over D in KS = 5 / 7 exact steps of 16, nothing padded.  O^T has D feature ROWS, and an MFMA's A operand has 32: the V^T tile
//   has DP = fa_dp<D>() = 96 / 128 rows, NB = DP / 32 = 3 / 4 blocks.  Row r of A reaches row r of the result and no other, so the pad rows D .. DP - 1
//   of the V^T tile are never written (no zeroing pass, no staging: whatever the LDS holds there, NaN patterns included, ends in accumulator
//   registers that are rescaled with the rest and never stored) and the epilogue skips the f32x4 groups at dv >= D (32 i + 8 g + 4 hi with
//   D % 16 == 0: a whole group is in or out, at compile time).  The pad rows are ALLOCATED, not aliased onto the K tile or the live V^T rows: an
//   alias would save 2176 B where two workgroups of 24320 / 32768 B are far from a CU's 160 KB, and nothing else (the pad rows are read either
//   way).  Price: (2 KS + 4 NB) / (2 KS + 4 D / 32) = 22 / 20 = 1.10 MFMA slots per useful one at 80, 30 / 28 = 1.07 at 112.
//   NOT built: the 16-row tail on v_mfma_f32_16x16x32_f16 (4 of them, 8 passes each, instead of 4 x 16 passes: 32 of a tile's 352 / 480 passes, 9 % /
//   7 %).  Its B operand wants 16 queries x 4 lane rows of 8 positions; the lane pair holds 32 queries x 2.  Per tile that is 8 v_permlane16_swap
//   (each pair of P fragments, 4 registers) behind the exp2 and in front of the MFMAs, 8 more live registers, and a result whose query is lane % 16:
//   alpha, and 1 / l in the epilogue, live per lane pair (query = lane % 32), so every rescale would move them across lanes as well.  Measured
//   (profiles/fattn_head_size_112.txt): what separates the head sizes at equal H D is the per-tile work outside the MFMAs, and the tail adds to it.
//   K rows are 2 D + 16 = 176 / 240 bytes, 11 / 15 chunks: odd, fa_k_layout's argument holds.  64 CPR = 640 / 896 K chunks do not divide by 256
//   threads: NKC rounds up to 3 / 4 and the surplus threads (128) load row 0 of the tile again and store nothing (fa_k_guard).  V units: 160 / 224
//   for 256 threads, as at 96.  Q: all KS fragments as one group (fa_q_group must divide KS, and 5 and 7 are prime).  Merge: G = 12 / 9 groups and
//   a remainder of 64 / 16 threads; partial rows of D + 4 floats are 336 / 464 bytes, so the f32x4 partial stores stay aligned.
//
// D = 96: KS = 6, NB = 3: 48 + 24 + 32 registers of O / Q / S, two workgroups per CU; LDS 64 * 208 + 96 * 136 = 26368 B.  K staging is three
//   chunks per thread exactly; the V^T staging has 16 * 12 = 192 units of 4 positions x 8 features for 256 threads: the last wave loads a duplicate
//   (in bounds) and stores nothing.  Q8_0 rows are 3 blocks of 34 bytes, 102 B: 2-byte aligned pieces as at every other size.
//
// D = 256: O^T alone is NB * 16 = 128 registers per lane, Q 64, S 32, FA_PD fragments 16, the tile-ahead staging 64 (F16; Q8_0 keeps 80 raw pieces):
//   over the 256 a wave has at two waves per SIMD (the tile-ahead loop at 256 and two waves: 148 .. 220 registers spilled).  Chosen: ONE workgroup of
//   four waves per CU, one wave per SIMD with the full 512-register file, and no tile-ahead prefetch, so no staging register lives over the MFMA
//   loops.  440 .. 509 registers, no scratch.  LDS 64 * 528 + 256 * 136 = 68608 B (above 64 KB: opted in once per device).  Built and dropped without
//   a run: the same at 512 registers WITH the tile-ahead prefetch -- VALU operands must sit in the 256 architectural registers, the rest is
//   reachable by MFMAs, loads and copies only, and the Q8_0 and mask-tensor instantiations went to scratch (220 .. 308 bytes per lane).  The price
//   of one wave per SIMD is known from the kernel's own history at D = 128 (0.74 ms per layer against 0.29 at two waves: a wave that waits at a
//   tile barrier has nobody to give its SIMD to); measured here: DESIGN.md section 6.  NOT built: Q fragments in LDS (a 128-row Q tile is 66 KB:
//   with the K and V^T tiles one workgroup per CU again, and two LDS reads per S MFMA); a 32-position KV tile (halves S and staging, not O, and
//   the soft-max would rescale per 32 positions, which term (c) does not count); O's dv blocks split over two waves sharing one score tile (fits
//   256 registers, needs P and the row statistics exchanged through LDS every tile) -- the candidate for closing the gap.
//
// CAP (logit_softcap != 0; fattn_cap.hip: D = 128 / 256, F16 / Q8_0 rows by position, no mask or a mask tensor):
//   s = cap tanh(scale / cap K[kv] . Q[n]) + mask[kv, n]   (ggml_compute_forward_flash_attn_ext_f16: scale /= cap, tanh, * cap, + mask)
//   Between the two MFMA blocks each of the lane's 32 score registers becomes t = fa_tanh(s a.cap_in), cap_in = scale / cap, and the host sets
//   sc2 = cap log2(e) instead of scale log2(e).  Everything downstream already speaks in "raw score times sc2" and so works in units of t unchanged:
//   mask_mul = log2(e) / sc2 is 1 / cap (the mask joins t as mask / cap and leaves the exponent as mask log2(e)), the -inf fills, the lazy maximum
//   (m_run, FA_TAU: log2 domain), exp2(fma(t, sc2, -m)), the split-KV partials and the merge.  A row of a ragged tile beyond kv_hi is a re-read of
//   the last row: a finite tanh, then filled with -inf like any score.  The tanh stands outside the staging lambdas (what they capture moves the
//   prologue's schedule); without CAP it is not there, and the kernels of the three other files are the parent's instruction for instruction
//   (profiles/fattn_softcap.txt).
#pragma once
#include "attn_token.h"      // k_slot, v_slot: the cache layouts k_rope_kv_prep writes
#include <stdlib.h>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float    f32x16 __attribute__((ext_vector_type(16)));

#define FA_VSTR 136                  // bytes per V^T row in LDS: 64 positions * 2 B + 8 B (conflict-free ds_read_b64 over 32 rows), independent of D
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
    float sc2;                                              // scale * log2(e); CAP: cap * log2(e)
    float cap_in;                                           // CAP: scale / cap, the factor of the raw score under the tanh (last: no other field moves)
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

// ---- what depends on the head size
// The K tile in LDS: 64 rows of CPR = D / 8 chunks of 16 bytes; chunk(tile, row, col) is where chunk col of row lies.  The fragment read is one
// ds_read_b128 per lane: lane (l31, hi) reads chunk 2 ks + hi of row 32 j + l31.  The LDS serves a b128 read in groups of consecutive lanes of one hi,
// each group covering all banks once (8 lanes x 16 B over 32 banks; 16 lanes over 64), and the lanes of a group differ in l31, the row, only.
//   64 / 128: rows of 2 D bytes, the chunks of a row XOR-swizzled with row & (CPR - 1): consecutive rows put one chunk column into different banks.
//   96 / 256: rows of 2 D + 16 bytes (CPR + 1 chunks: 13 at 96, 33 at 256), no swizzle.  The XOR permutes a row's chunks only for a power-of-two
//     CPR; CPR = 12 is none.  CPR + 1 is odd, so an odd multiple of consecutive rows gives 8 (16) different residues mod 8 (16): every lane of a
//     group in its own 16-byte bank group, no conflict.  The staging stores walk a row's chunks with consecutive lanes and skip one chunk at each
//     row end: at most two lanes of a group of eight meet (a 2-way conflict on one store group in CPR / 8).  Cost: 1 KB of padding.  256 keeps this
//     form although its CPR is a power of two (it was measured and bounded in it).
template <int D> struct fa_k_layout {
    static constexpr int CPR = D / 8;
    static constexpr bool swizzled = D == 64 || D == 128;
    static constexpr int row_bytes = swizzled ? 2 * D : 2 * D + 16;      // 112: 240 (15 chunks)
    static_assert(swizzled || (CPR + 1) % 2 == 1, "an odd K row stride in chunks");
    static __device__ __forceinline__ char * chunk(char * tile, int row, int col) { return tile + row * row_bytes + ((swizzled ? col ^ (row & (CPR - 1)) : col) << 4); }
};
// Feature rows of the V^T tile and of O^T: D rounded up to the 32 rows of an MFMA's A operand (80 -> 96, 112 -> 128); rows D .. fa_dp - 1 are never
// written and never stored (the header's D = 112 paragraph)
template <int D> constexpr int fa_dp() { return (D + 31) & ~31; }
// LDS of one workgroup: the K tile, then the V^T tile
template <int D> constexpr int fa_lds_bytes() { return 64 * fa_k_layout<D>::row_bytes + fa_dp<D>() * FA_VSTR; }
// Up to 128 the next tile's K / V rows are loaded into registers one tile ahead (the loads fly under the MFMA work of the current tile) and two
// workgroups share a CU.  At 256 those staging registers do not fit beside O, Q and S (the header's D = 256 paragraph): a tile's rows are loaded
// and stored between its two barriers, and one workgroup per CU gives each wave the full 512-register file.
template <int D> constexpr bool fa_tile_ahead() { return D <= 128; }
template <int D> constexpr int fa_min_blocks() { return D > 128 ? 1 : 2; }
// VL = 1, V^T rows (the runner's V cache: cllm_op_attn_prefill, launch_attn_long_flash), exists at 64 / 128 only
// (with it goes a.n_kv_dev, the position count read on the device: only launch_attn_long_flash sets it)
template <int D> constexpr bool fa_has_vt() { return D == 64 || D == 128; }
// Q fragments loaded, converted and rounded to fp16 as one group (the values do not depend on it: a Q8_0 block is two fragments).  Up to 128 all of
// them at once, every load issued before the first conversion; at 96 and 256 block by block, so a block's floats are dead before the next block's
// arrive (at 256 the whole row as floats would be 64 registers beside the 128 of O).  112 (80): KS is prime and the rows are F16, all at once.
template <int D> constexpr int fa_q_group() { return D == 64 || D == 128 || D % 32 ? D / 16 : 2; }
// The 64 CPR chunks of a K tile divide evenly over the 256 threads at 64 / 96 / 128 / 256, so no thread is without a chunk and a guard on the K
// staging (row 0 instead of a row past the tile, no store) never acts.  The compiler does not drop it, though: at 96 / 256 it costs a select per
// chunk, on the critical path at 256 where a tile's loads sit between its two barriers (decode D = 256 F16: 19.7 against 19.3 us), so those sizes
// have none.  64 / 128 keep theirs: without it each of their kernels comes out 6 .. 20 instructions different from the code the runner's prefill
// and long-context paths were measured with, for nothing that has been measured.  112 (896 chunks; 80: 640) needs it: there it acts.
template <int D> constexpr bool fa_k_guard() { return D == 64 || D == 128 || (64 * (D / 8)) % 256 != 0; }

// CAP: tanh(u) = 1 - 2 / (1 + e^(2u)) on the hardware's exp2 and rcp: no branch, one temporary, and no libm call frame (at D = 256 the kernel has
// 440 .. 509 registers).  e^(2u) overflows to inf for u > 44 (rcp -> 0, the result exactly 1) and underflows to 0 for u < -52 (rcp(1) = 1, exactly
// -1).  exp2 and rcp are good to 1 ulp each and the sum and the difference round once each: a few 1e-7 ABSOLUTE, also around u = 0 where the
// difference cancels.  The soft-max multiplies it by sc2 = cap log2(e) (72 at cap 50) in the exponent: about 1e-5 relative on a probability, two
// orders below the fp16 rounding of P (4.9e-4) that the tolerance tier is made of.
__device__ __forceinline__ float fa_tanh(float u) {
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(u * (2.0f * FA_LOG2E)));
}

template <int D, int KVT, int VL, int MASK, bool CAP = false>
__global__ void __launch_bounds__(256, fa_min_blocks<D>()) k_fattn(const fattn_args a) {
    using KL = fa_k_layout<D>;
    constexpr int NT = 256, BQ = 128, KS = D / 16, DP = fa_dp<D>(), NB = DP / 32, CPR = D / 8, QG = fa_q_group<D>();
    static_assert(D % 16 == 0 && KS % QG == 0, "whole S^T steps, whole Q groups");
    static_assert(KVT != CLLM_TYPE_Q8_0 || (D % 32 == 0 && QG % 2 == 0), "Q8_0 blocks per row, two fragments per block");
    static_assert(VL == 0 || (fa_has_vt<D>() && KVT == CLLM_TYPE_F16), "V^T rows: F16 at 64 / 128");
    extern __shared__ __attribute__((aligned(16))) char fa_smem[];
    char * Kl = fa_smem, * Vl = fa_smem + 64 * KL::row_bytes;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int rows = a.N * a.R, nqb = (rows + BQ - 1) / BQ;
    int qb = (int) blockIdx.x % nqb;
    const int split = (int) blockIdx.x / nqb;
    if (MASK == 1) qb = nqb - 1 - qb;                                  // the long (late) query blocks first
    const int y = blockIdx.y, b = blockIdx.z;
    const int hk = y * a.R / (a.H / a.Hkv);
    const bool wave_live = qb * BQ + wave * 32 < rows;
    const int rho = qb * BQ + wave * 32 + l31;
    const bool rvalid = rho < rows;
    const int rc = rvalid ? rho : rows - 1;
    const int n = rc / a.R, h = y * a.R + rc % a.R;

    // ---- Q: KS fragments of 8 halves (dk = 16 ks + 8 hi ..), converted as the CPU converts it for K's vec_dot
    half8 qf[KS];
    {
        const char * qp = a.q + (int64_t) n * a.q_nb1 + (int64_t) h * a.q_nb2 + (int64_t) b * a.q_nb3;
#pragma unroll
        for (int g = 0; g < KS / QG; g++) {
            float x[QG][8];
#pragma unroll
            for (int f = 0; f < QG; f++) {
                const int ks = QG * g + f;
                const f32x4 lo = *(const f32x4 *)(qp + (16 * ks + 8 * hi) * 4), up = *(const f32x4 *)(qp + (16 * ks + 8 * hi) * 4 + 16);
                x[f][0] = lo.x; x[f][1] = lo.y; x[f][2] = lo.z; x[f][3] = lo.w; x[f][4] = up.x; x[f][5] = up.y; x[f][6] = up.z; x[f][7] = up.w;
            }
            if (KVT == CLLM_TYPE_Q8_0) {                               // quantize_row_q8_0 (arch/x86/quants.c:290-345) then the dequantized value
#pragma unroll
                for (int blk = 0; blk < QG / 2; blk++) {               // one Q8_0 block = two fragments: the lane pair holds its 32 values
                    float amax = 0.0f;
#pragma unroll
                    for (int e = 0; e < 8; e++) amax = fmaxf(amax, fmaxf(fabsf(x[2 * blk][e]), fabsf(x[2 * blk + 1][e])));
                    amax = fa_pair_max(amax);
                    const float d = amax / 127.0f, id = amax != 0.0f ? 127.0f / amax : 0.0f, dq = h2f(f2h(d));
#pragma unroll
                    for (int e = 0; e < 8; e++) { x[2 * blk][e] = dq * rintf(x[2 * blk][e] * id); x[2 * blk + 1][e] = dq * rintf(x[2 * blk + 1][e] * id); }
                }
            }
#pragma unroll
            for (int f = 0; f < QG; f++)
#pragma unroll
                for (int e = 0; e < 8; e++) qf[QG * g + f][e] = (_Float16) x[f][e];
        }
    }

    const char * kb = a.k + (int64_t) hk * a.k_nb2 + (int64_t) b * a.k_nb3;
    const char * vb = a.v + (int64_t) hk * a.v_nb2 + (int64_t) b * a.v_nb3;
    const char * mrow = MASK == 2 ? a.mask + (int64_t) n * a.m_nb1 + (int64_t)(h % a.m_ne2) * a.m_nb2 + (int64_t)(b % a.m_ne3) * a.m_nb3 : nullptr;

    const int n_kv = fa_has_vt<D>() && a.n_kv_dev ? min(a.n_kv, a.n_kv_dev[0] + 1) : a.n_kv;
    const int kv_lo = split * a.chunk;
    int kv_hi = min(n_kv, kv_lo + a.chunk);
    if (MASK == 1) kv_hi = min(kv_hi, a.n_past + min(a.N - 1, (qb * BQ + BQ - 1) / a.R) + 1);
    const int lim = MASK == 1 ? a.n_past + n : 0;                      // causal: position kv is visible to row n iff kv <= n_past + n

    const float mask_mul = FA_LOG2E / a.sc2;                           // mask values are added to the RAW scores: (s + mask log2e / sc2) sc2 = s sc2 + mask log2e
    f32x16 o[NB];
#pragma unroll
    for (int i = 0; i < NB; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[i][r] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;

    // ---- K / V staging is split in two: global -> registers (fa_tile_ahead: issued one tile ahead) and registers -> LDS (conversion, K layout,
    //      transposition; between the two barriers of a tile).  Q8_0 rows keep their raw 16-bit pieces in the registers (34-byte blocks: 2-byte
    //      alignment) and are dequantized on the way into LDS.
    //      A thread count that does not divide the chunk count leaves the last threads a duplicate load (in bounds) and no store: the V units at 64 and 96
    //      (128 and 192 of them for 256 threads), and at 112 both the V units (224) and the K chunks (896: fa_k_guard).
    static_assert(((64 * CPR) % NT == 0 || fa_k_guard<D>()) && (VL == 0 || (D * 8) % NT == 0), "K chunks: every thread has one, or the guard; V^T chunks: every thread has one");
    constexpr bool Q8 = KVT == CLLM_TYPE_Q8_0;
    constexpr int NKC = (64 * CPR + NT - 1) / NT;                     // K chunks (8 elements) per thread: 2 | 3 | 4 | 8 (112: 4, the last one for half the threads)
    constexpr int NVU = VL == 1 ? (D * 8 + NT - 1) / NT : (16 * CPR + NT - 1) / NT;      // V^T chunks (VL 1) / 4-row x 8-element units (VL 0) per thread
    struct raw8 { uint32_t h[4]; uint32_t d; };                      // Q8_0: four 16-bit pieces of 8 quants + the block scale
    u32x4 kreg[Q8 ? 1 : NKC]; raw8 kraw[Q8 ? NKC : 1];
    u32x4 vreg[Q8 ? 1 : (VL == 1 ? NVU : 4 * NVU)]; raw8 vraw[Q8 ? 4 * NVU : 1];
    auto q8_load = [&](const char * row, int e0) {
        raw8 r; const char * p = row + (e0 >> 5) * 34;
        r.d = *(const uint16_t *) p;
        const uint16_t * qs = (const uint16_t *)(p + 2 + (e0 & 31));
#pragma unroll
        for (int i = 0; i < 4; i++) r.h[i] = qs[i];
        return r;
    };
    auto q8_cvt = [&](const raw8 & r) {
        const float d = h2f((uint16_t) r.d);
        u32x4 out;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const _Float16 lo = (_Float16)(d * (float)(int8_t)(r.h[i] & 0xff)), up = (_Float16)(d * (float)(int8_t)(r.h[i] >> 8));
            uint16_t x, y; __builtin_memcpy(&x, &lo, 2); __builtin_memcpy(&y, &up, 2);
            out[i] = (uint32_t) x | ((uint32_t) y << 16);
        }
        return out;
    };
    // The V^T form stands under `if constexpr (fa_has_vt<D>())`, not under `if constexpr (VL == 1)`: a discarded branch captures nothing, and what a
    // [&] closure captures (n_kv here) moves the compiler's schedule of the whole prologue.  So the sizes without the form do not capture for it, and
    // at 64 / 128 the VL 0 kernels capture as the VL 1 kernels do.
    auto load_tile = [&](int kv0) {                                    // every row index is clamped to kv_hi - 1: a ragged tile re-reads the last row
#pragma unroll
        for (int t = 0; t < NKC; t++) {
            const int c = tid + t * NT, row = c / CPR, col = c % CPR, kv = min(kv0 + (!fa_k_guard<D>() || c < 64 * CPR ? row : 0), kv_hi - 1);
            if (Q8) kraw[Q8 ? t : 0] = q8_load(kb + (int64_t) kv * a.k_nb1, col * 8);
            else    kreg[Q8 ? 0 : t] = *(const u32x4 *)(kb + (int64_t) kv * a.k_nb1 + col * 16);
        }
        if constexpr (fa_has_vt<D>()) if (VL == 1) {
#pragma unroll
            for (int t = 0; t < NVU; t++) {
                const int c = tid + t * NT, dv = (c >> 3) % D, kc = c & 7, kvs = kv0 + 8 * kc;
                const int kvl = min(kvs, (n_kv - 1) & ~7);
                vreg[Q8 ? 0 : t] = *(const u32x4 *)(vb + (int64_t) dv * a.v_nb1 + (int64_t) kvl * 2);
            }
            return;
        }
#pragma unroll
        for (int t = 0; t < NVU; t++) {
            const int u = (tid + t * NT) % (16 * CPR), kvg = u / CPR, dvg = u % CPR;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int kv = min(kv0 + 4 * kvg + i, kv_hi - 1);
                if (Q8) vraw[Q8 ? 4 * t + i : 0] = q8_load(vb + (int64_t) kv * a.v_nb1, dvg * 8);
                else    vreg[Q8 ? 0 : 4 * t + i] = *(const u32x4 *)(vb + (int64_t) kv * a.v_nb1 + dvg * 16);
            }
        }
    };
    auto store_tile = [&](int kv0) {
#pragma unroll
        for (int t = 0; t < NKC; t++) {
            const int c = tid + t * NT, row = c / CPR, col = c % CPR;
            if ((64 * CPR) % NT == 0 || c < 64 * CPR) *(u32x4 *) KL::chunk(Kl, row, col) = Q8 ? q8_cvt(kraw[Q8 ? t : 0]) : kreg[Q8 ? 0 : t];
        }
        if constexpr (fa_has_vt<D>()) if (VL == 1) {
#pragma unroll
            for (int t = 0; t < NVU; t++) {
                const int c = tid + t * NT, dv = c >> 3, kc = c & 7, kvs = kv0 + 8 * kc;
                u32x4 x = vreg[Q8 ? 0 : t];
                if (kv0 + 64 > n_kv) {                                 // (block-uniform: only the cache's last, partial tile)
                    const int left = n_kv - kvs;                       // elements of this chunk that exist (the rest of the cache row is not ours: may be anything)
#pragma unroll
                    for (int w = 0; w < 4; w++) {
                        const uint32_t keep = 2 * w + 1 < left ? 0xffffffffu : 2 * w < left ? 0xffffu : 0u;
                        x[w] &= keep;
                    }
                }
                if ((D * 8) % NT == 0 || c < D * 8) { char * p = Vl + dv * FA_VSTR + kc * 16; *(u32x2 *) p = u32x2{x.x, x.y}; *(u32x2 *)(p + 8) = u32x2{x.z, x.w}; }
            }
            return;
        }
#pragma unroll
        for (int t = 0; t < NVU; t++) {
            const int u = tid + t * NT, kvg = u / CPR, dvg = u % CPR;
            u32x4 x[4];
#pragma unroll
            for (int i = 0; i < 4; i++) x[i] = Q8 ? q8_cvt(vraw[Q8 ? 4 * t + i : 0]) : vreg[Q8 ? 0 : 4 * t + i];
            if ((16 * CPR) % NT == 0 || u < 16 * CPR) {
#pragma unroll
                for (int e = 0; e < 8; e++) {                      // 4 x 4 transposition in registers: V rows by position -> V^T rows by feature
                    const uint32_t sel = (e & 1) ? 0x07060302u : 0x05040100u;
                    const uint32_t lo = __builtin_amdgcn_perm(x[1][e >> 1], x[0][e >> 1], sel), up = __builtin_amdgcn_perm(x[3][e >> 1], x[2][e >> 1], sel);
                    *(u32x2 *)(Vl + (8 * dvg + e) * FA_VSTR + kvg * 8) = u32x2{lo, up};
                }
            }
        }
    };

    constexpr bool AHEAD = fa_tile_ahead<D>();
    if (AHEAD && kv_lo < kv_hi) load_tile(kv_lo);
    for (int kv0 = kv_lo; kv0 < kv_hi; kv0 += 64) {
        // ---- the mask of this tile (tensor form): the lane's 32 positions in 8 groups of 4
        float mv[2][16];
        bool skip = false;
        if (MASK == 2) {
            int any = 0;
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const int kvb = kv0 + 32 * j + 8 * g + 4 * hi;
                    uint16_t w[4];
                    if (a.m_al) {
                        u32x2 t = u32x2{0xfc00fc00u, 0xfc00fc00u};
                        if (kvb < kv_hi) t = *(const u32x2 *)(mrow + (int64_t) kvb * 2);
                        w[0] = (uint16_t) t.x; w[1] = (uint16_t)(t.x >> 16); w[2] = (uint16_t) t.y; w[3] = (uint16_t)(t.y >> 16);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; e++) w[e] = kvb + e < kv_hi ? *(const uint16_t *)(mrow + (int64_t)(kvb + e) * 2) : (uint16_t) 0xfc00;
                    }
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const float f = kvb + e < kv_hi ? h2f(w[e]) : -INFINITY;
                        mv[j][4 * g + e] = f * mask_mul;                   // in units of the raw score (the scale is applied later)
                        any |= (f != -INFINITY) && rvalid;
                    }
                }
            skip = !__syncthreads_or(any);                             // (also: the previous tile's fragments have been read) nothing of this tile visible: no staging, no math
        } else {
            __syncthreads();                                           // the previous tile's fragments have been read
        }
        if (!AHEAD && !skip) load_tile(kv0);
        if (!skip) store_tile(kv0);
        if (AHEAD && kv0 + 64 < kv_hi) load_tile(kv0 + 64);            // the next tile's loads fly under this tile's math
        if (skip) continue;
        __syncthreads();

        if (!wave_live) continue;                                      // (decode: the group's rows fit one wave; the others only help staging)
        // ---- S^T = K . Q^T: 2 KS MFMAs.  The K fragments are read FA_PD MFMAs ahead of their use (the compiler's own order is read -> wait -> MFMA,
        //      one LDS latency per MFMA); sched_barrier pins the order
        f32x16 s[2];
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) s[j][r] = 0.0f;
        {
            auto kfrag = [&](int idx) { return *(const half8 *) KL::chunk(Kl, 32 * (idx / KS) + l31, 2 * (idx % KS) + hi); };
            half8 kf[FA_PD];
#pragma unroll
            for (int p = 0; p < FA_PD; p++) kf[p] = kfrag(p);
#pragma unroll
            for (int idx = 0; idx < 2 * KS; idx++) {
                __builtin_amdgcn_sched_barrier(0);
                s[idx / KS] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[idx % FA_PD], qf[idx % KS], s[idx / KS], 0, 0, 0);
                if (idx + FA_PD < 2 * KS) kf[idx % FA_PD] = kfrag(idx + FA_PD);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- logit soft-cap: the raw score becomes tanh(s scale / cap), in (-1, 1); from here on sc2 = cap log2(e) is its scale (the header's CAP paragraph)
        if (CAP) {
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) s[j][r] = fa_tanh(s[j][r] * a.cap_in);
        }

        // ---- online soft-max (base 2) of the row held by this lane pair.  The exponent reference m_run follows the running maximum lazily:
        //      it moves (and O, l are rescaled) only when a tile's maximum exceeds it by more than FA_TAU, so p <= 2^FA_TAU (fp16 holds it with the
        //      same relative precision) and the rescale of the O registers leaves the steady state of the loop
        const bool full = MASK != 2 && kv0 + 64 <= kv_hi && (MASK == 0 || kv0 + 63 <= a.n_past + (qb * BQ + wave * 32) / a.R);      // nothing of this tile is masked for this wave
        float mx = -INFINITY;
        if (!full) {
#pragma unroll
            for (int j = 0; j < 2; j++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int kv = kv0 + 32 * j + fa_crow(r, hi);
                    float t = s[j][r];
                    if (MASK == 2) t += mv[j][r];                      // -inf beyond kv_hi
                    else if (MASK == 1) t = (kv <= lim && kv < kv_hi) ? t : -INFINITY;
                    else t = kv < kv_hi ? t : -INFINITY;
                    s[j][r] = t;
                }
        }
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) mx = fmaxf(mx, s[j][r]);
        mx = fa_pair_max(mx) * a.sc2;                                  // sc2 > 0: the maximum of the scaled scores
        const bool grow = mx > m_run + FA_TAU;                         // (m_run = -inf: any finite maximum)
        if (__any(grow)) {
            const float m_new = grow ? mx : m_run;
            const float alpha = grow ? __builtin_amdgcn_exp2f(m_run - m_new) : 1.0f;      // m_run = -inf -> 0
            l_run *= alpha;
#pragma unroll
            for (int i = 0; i < NB; i++)
#pragma unroll
                for (int r = 0; r < 16; r++) o[i][r] *= alpha;
            m_run = m_new;
        }
        const float msafe = m_run == -INFINITY ? 0.0f : m_run;         // a row with nothing visible yet: every p = exp2(-inf) = 0
        float psum = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) { const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[j][r], a.sc2, -msafe)); s[j][r] = p; psum += p; }
        l_run += psum;

        // ---- O^T += V^T . P^T: 4 NB MFMAs, V^T fragments read FA_PD ahead (112: the last block's rows D .. DP - 1 are whatever the LDS holds)
        {
            half8 pb[4];
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int e = 0; e < 8; e++) pb[q][e] = (_Float16) s[q >> 1][8 * (q & 1) + e];
            auto vfrag = [&](int idx) {                                // idx = 4-kv-group q (j, kk) major, dv block i minor
                const int q = idx / NB, i = idx % NB;
                const char * p = Vl + (32 * i + l31) * FA_VSTR + (32 * (q >> 1) + 16 * (q & 1) + 4 * hi) * 2;
                const half4 v0 = *(const half4 *) p, v1 = *(const half4 *)(p + 16);
                return half8{v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
            };
            half8 vf[FA_PD];
#pragma unroll
            for (int p = 0; p < FA_PD; p++) vf[p] = vfrag(p);
#pragma unroll
            for (int idx = 0; idx < 4 * NB; idx++) {
                __builtin_amdgcn_sched_barrier(0);
                o[idx % NB] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[idx % FA_PD], pb[idx / NB], o[idx % NB], 0, 0, 0);
                if (idx + FA_PD < 4 * NB) vf[idx % FA_PD] = vfrag(idx + FA_PD);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- epilogue: lane holds O^T[dv = 32 i + crow(r, hi), q = l31]: groups of 4 consecutive dv; the groups of the pad rows (dv >= D) are not stored
    const float l_tot = fa_pair_sum(l_run);
    if (!rvalid) return;
    if (a.splits == 1) {
        const float inv = l_tot == 0.0f ? 0.0f : 1.0f / l_tot;
        char * dp = a.dst + (int64_t) n * a.d_nbn + (int64_t) h * a.d_nbh + (int64_t) b * a.d_nbb;
#pragma unroll
        for (int i = 0; i < NB; i++)
#pragma unroll
            for (int g = 0; g < 4; g++)
                if (DP == D || 32 * i + 8 * g < D) *(f32x4 *)(dp + (32 * i + 8 * g + 4 * hi) * 4) = f32x4{o[i][4 * g] * inv, o[i][4 * g + 1] * inv, o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv};
    } else {
        float * pp = a.part + ((((int64_t) b * a.H + h) * a.N + n) * a.splits + split) * (D + 4);
#pragma unroll
        for (int i = 0; i < NB; i++)
#pragma unroll
            for (int g = 0; g < 4; g++)
                if (DP == D || 32 * i + 8 * g < D) *(f32x4 *)(pp + 32 * i + 8 * g + 4 * hi) = f32x4{o[i][4 * g], o[i][4 * g + 1], o[i][4 * g + 2], o[i][4 * g + 3]};
        if (hi == 0) { pp[D] = m_run; pp[D + 1] = l_tot; }
    }
}

// merge the split-KV partials of one (b, h, n) (ggml_flash_attn_ext_reduce_partials, ops.cpp:8642-8710): 1024 threads = D output elements x
// G = 1024 / D interleaved groups of splits, so that the loads of different splits are independent and coalesced.  D = 96: G = 10, and the last
// 64 threads (a partial eleventh group) take part in the two reductions over the splits only; likewise 112 (G = 9, 16 threads)
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

// ---- launch (a, decode: as launch_fattn planned them).  decode: one workgroup per (split, KV group, batch), four waves stage the tile (one load
//      latency), the wave that owns the packed rows computes, then the merge; prefill: 128 query rows per workgroup (R = 1)
template <int D, int KVT, int VL, int MASK, bool CAP = false>
static int fattn_go(hipStream_t st, const fattn_args & a, int B, bool decode) {
    constexpr int lds = fa_lds_bytes<D>();
    static_assert(lds <= 160 * 1024, "one CU's LDS");
    if (lds > 64 * 1024) { static uint64_t flag = 0; if (int rc = lds_opt_in(k_fattn<D, KVT, VL, MASK, CAP>, flag, lds)) return rc; }
    const dim3 grid(decode ? (unsigned) a.splits : (unsigned)((a.N + 127) / 128), (unsigned)(a.H / a.R), (unsigned) B);
    hipLaunchKernelGGL((k_fattn<D, KVT, VL, MASK, CAP>), grid, dim3(256), lds, st, a);
    LAUNCH_CHECK();
    if (a.splits > 1) { hipLaunchKernelGGL((k_fattn_merge<D>), dim3((unsigned) a.N, (unsigned) a.H, (unsigned) B), dim3(1024), 0, st, a); LAUNCH_CHECK(); }
    return CLLM_OK;
}
template <int D, int KVT, int VL>
static int fattn_go_mask(hipStream_t st, const fattn_args & a, int mmode, int B, bool decode) {
    if (mmode == 0) return fattn_go<D, KVT, VL, 0>(st, a, B, decode);
    if (mmode == 1) return fattn_go<D, KVT, VL, 1>(st, a, B, decode);
    return fattn_go<D, KVT, VL, 2>(st, a, B, decode);
}
// every instantiation of one head size: ktype F16 | Q8_0 (launch_fattn has checked it; Q8_0 where D % 32 == 0), vl 1 with F16 where fa_has_vt, mmode 0 none | 1 causal | 2 tensor
template <int D>
static int fattn_dispatch(hipStream_t st, const fattn_args & a, int ktype, int vl, int mmode, int B, bool decode) {
    if (vl == 1) {
        if constexpr (fa_has_vt<D>()) { if (ktype == CLLM_TYPE_F16) return fattn_go_mask<D, CLLM_TYPE_F16, 1>(st, a, mmode, B, decode); }
        return CLLM_E_UNSUPPORTED;
    }
    if (ktype == CLLM_TYPE_Q8_0) {                                     // a Q8_0 row is whole blocks of 32: not instantiated at 112
        if constexpr (D % 32 == 0) return fattn_go_mask<D, CLLM_TYPE_Q8_0, 0>(st, a, mmode, B, decode);
        return CLLM_E_UNSUPPORTED;
    }
    return fattn_go_mask<D, CLLM_TYPE_F16, 0>(st, a, mmode, B, decode);
}

// fattn_hs.hip: the head sizes 96 / 256; fattn_pad.hip: 112, F16 rows (V rows by position only); fattn_cap.hip: the logit soft-cap at 128 / 256
// (V rows by position, mmode 0 | 2)
int fattn_hs_launch(hipStream_t st, const fattn_args & a, int D, int ktype, int mmode, int B, bool decode);
int fattn_pad_launch(hipStream_t st, const fattn_args & a, int D, int ktype, int mmode, int B, bool decode);
int fattn_cap_launch(hipStream_t st, const fattn_args & a, int D, int ktype, int mmode, int B, bool decode);
