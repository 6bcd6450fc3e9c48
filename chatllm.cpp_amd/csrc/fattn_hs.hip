// fattn_hs.hip -- GGML_OP_FLASH_ATTN_EXT at the head sizes k_fattn (fattn.hip) cannot be instantiated at: D = 96 (Phi-3-mini class, vision / audio
// towers) and D = 256 (the Gemma line).  Same entry (launch_fattn plans, fattn_hs_launch launches), same numerics, same partial layout and merge.
//
// Numerics: exactly the computation fattn.hip's header describes and tests/fattn_model.py bounds -- v_mfma_f32_32x32x16_f16 in the swapped form
// (S^T = K . Q^T, O^T += V^T . P^T, a query row per lane pair), Q converted as the CPU converts it (fp16 | quantize_row_q8_0 then fp16), K / V at stored
// precision, fp32 online soft-max in base 2 with the lazy FA_TAU rescale, P rounded to fp16, fp32 l and O, exact zeros for a row that sees nothing.
// K / V are walked in tiles of 64 positions, as k_fattn walks them: one possible rescale per 64 positions, so term (c) of the model's bound
// ((2.5 n_in + 2 tiles_per_chunk + 5) u A) counts this kernel's roundings one for one, and launch_plan's chunk / splits describe it unchanged.
//
// What differs from k_fattn, and why:
//
// K tile in LDS: rows of KSTR = 2 D + 16 bytes, i.e. CPR + 1 chunks of 16 bytes with CPR = D / 8 (13 chunks at D = 96, 33 at D = 256), no swizzle.
//   k_fattn's XOR swizzle col ^ (row & (CPR - 1)) permutes a row's chunks only for a power-of-two CPR; CPR = 12 is none.  The fragment read is one
//   ds_read_b128 per lane: lane (l31, hi) reads chunk 2 ks + hi of row 32 j + l31, which lies at chunk (CPR + 1) (32 j + l31) + 2 ks + hi of the tile.
//   The LDS serves a b128 read in groups of consecutive lanes of one hi, each group covering all banks once (8 lanes x 16 B over 32 banks; 16 lanes
//   over 64): the lanes of a group differ in l31 only, CPR + 1 is odd, so an odd multiple of consecutive integers gives 8 (16) different residues
//   mod 8 (16): every lane of a group in its own 16-byte bank group, no conflict.  The staging stores walk a row's chunks with consecutive lanes and
//   skip one chunk at each row end: at most two lanes of a group of eight meet (a 2-way conflict on one store group in CPR / 8).  Cost: 1 KB of padding.
//   V^T keeps k_fattn's [dv][kv] rows of FA_VSTR bytes (independent of D).
//
// D = 96: KS = 6, NB = 3: 48 + 24 + 32 registers of O / Q / S, two workgroups per CU as k_fattn; LDS 64 * 208 + 96 * 136 = 26368 B.  K staging is three
//   chunks per thread exactly; the V^T staging has 16 * 12 = 192 units of 4 positions x 8 features for 256 threads: the last wave loads a duplicate
//   (in bounds) and stores nothing.  Q8_0 rows are 3 blocks of 34 bytes, 102 B: 2-byte aligned pieces as at every other size.
//
// D = 256: O^T alone is NB * 16 = 128 registers per lane, Q 64, S 32, FA_PD fragments 16, the tile-ahead staging 64 (F16; Q8_0 keeps 80 raw pieces):
//   over the 256 a wave has at two waves per SIMD (k_fattn's loop at 256: 148 .. 220 registers spilled).  Chosen here: ONE workgroup of four waves per
//   CU, one wave per SIMD with the full 512-register file (__launch_bounds__(256, 1)), and no tile-ahead prefetch: a tile's K / V rows are loaded and
//   stored between its two barriers (AHEAD = false), so no staging register lives over the MFMA loops.  440 .. 509 registers, no scratch.  LDS
//   64 * 528 + 256 * 136 = 68608 B (above 64 KB: opted in once per device).  Built and dropped without a run: the same at 512 registers WITH the
//   tile-ahead prefetch -- VALU operands must sit in the 256 architectural registers, the rest is reachable by MFMAs, loads and copies only, and the
//   Q8_0 and mask-tensor instantiations went to scratch (220 .. 308 bytes per lane).  The price of one wave per SIMD is known from k_fattn's own history
//   at D = 128 (0.74 ms per layer against 0.29 at two waves: a wave that waits at a tile barrier has nobody to give its SIMD to); measured here:
//   DESIGN.md section 6.  NOT built: Q fragments in LDS (a 128-row Q tile is 66 KB: with the K and V^T tiles one workgroup per CU again, and two LDS
//   reads per S MFMA); a 32-position KV tile (halves S and staging, not O, and the soft-max would rescale per 32 positions, which term (c) does not
//   count); O's dv blocks split over two waves sharing one score tile (fits 256 registers, needs P and the row statistics exchanged through LDS
//   every tile) -- the candidate for closing the gap.
//
// Not here: vl == 1 (the runner's V^T cache), cllm_op_attn_prefill, launch_attn_long_flash: those stay at 64 / 128.
#include "fattn.h"

template <int D, int KVT, int MASK>
__global__ void __launch_bounds__(256, D > 128 ? 1 : 2) k_fattn_hs(const fattn_args a) {
    constexpr int NT = 256, BQ = 128, KS = D / 16, NB = D / 32, CPR = D / 8, KSTR = D * 2 + 16;
    static_assert(D % 32 == 0 && (CPR + 1) % 2 == 1, "Q8_0 blocks per row; an odd K row stride in chunks");
    extern __shared__ __attribute__((aligned(16))) char fa_smem[];
    char * Kl = fa_smem, * Vl = fa_smem + 64 * KSTR;
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
        for (int blk = 0; blk < D / 32; blk++) {                       // one Q8_0 block = two fragments: the lane pair holds its 32 values
            float x[2][8];
#pragma unroll
            for (int f = 0; f < 2; f++) {
                const f32x4 lo = *(const f32x4 *)(qp + (32 * blk + 16 * f + 8 * hi) * 4), up = *(const f32x4 *)(qp + (32 * blk + 16 * f + 8 * hi) * 4 + 16);
                x[f][0] = lo.x; x[f][1] = lo.y; x[f][2] = lo.z; x[f][3] = lo.w; x[f][4] = up.x; x[f][5] = up.y; x[f][6] = up.z; x[f][7] = up.w;
            }
            if (KVT == CLLM_TYPE_Q8_0) {                               // quantize_row_q8_0 (arch/x86/quants.c:290-345) then the dequantized value
                float amax = 0.0f;
#pragma unroll
                for (int e = 0; e < 8; e++) amax = fmaxf(amax, fmaxf(fabsf(x[0][e]), fabsf(x[1][e])));
                amax = fa_pair_max(amax);
                const float d = amax / 127.0f, id = amax != 0.0f ? 127.0f / amax : 0.0f, dq = h2f(f2h(d));
#pragma unroll
                for (int e = 0; e < 8; e++) { x[0][e] = dq * rintf(x[0][e] * id); x[1][e] = dq * rintf(x[1][e] * id); }
            }
#pragma unroll
            for (int e = 0; e < 8; e++) { qf[2 * blk][e] = (_Float16) x[0][e]; qf[2 * blk + 1][e] = (_Float16) x[1][e]; }
        }
    }

    const char * kb = a.k + (int64_t) hk * a.k_nb2 + (int64_t) b * a.k_nb3;
    const char * vb = a.v + (int64_t) hk * a.v_nb2 + (int64_t) b * a.v_nb3;
    const char * mrow = MASK == 2 ? a.mask + (int64_t) n * a.m_nb1 + (int64_t)(h % a.m_ne2) * a.m_nb2 + (int64_t)(b % a.m_ne3) * a.m_nb3 : nullptr;

    const int n_kv = a.n_kv;
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

    // ---- K / V staging in two steps, as k_fattn: global -> registers (D = 96: one tile ahead, the loads fly under the MFMA work of the current tile), registers ->
    //      LDS between the two barriers of a tile (Q8_0: dequantized on the way; V: 4 x 4 transposition in registers into V^T rows)
    constexpr bool Q8 = KVT == CLLM_TYPE_Q8_0;
    constexpr int NKC = 64 * CPR / NT;                                // K chunks (8 elements) per thread: 3 | 8
    constexpr int NVU = (16 * CPR + NT - 1) / NT;                     // V units (4 positions x 8 features) per thread: 1 (192 units) | 2
    static_assert((64 * CPR) % NT == 0, "K staging covers the tile exactly");
    struct raw8 { uint32_t h[4]; uint32_t d; };                      // Q8_0: four 16-bit pieces of 8 quants + the block scale
    u32x4 kreg[Q8 ? 1 : NKC]; raw8 kraw[Q8 ? NKC : 1];
    u32x4 vreg[Q8 ? 1 : 4 * NVU]; raw8 vraw[Q8 ? 4 * NVU : 1];
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
    auto load_tile = [&](int kv0) {                                    // every row index is clamped to kv_hi - 1: a ragged tile re-reads the last row
#pragma unroll
        for (int t = 0; t < NKC; t++) {
            const int c = tid + t * NT, row = c / CPR, col = c % CPR, kv = min(kv0 + row, kv_hi - 1);
            if (Q8) kraw[Q8 ? t : 0] = q8_load(kb + (int64_t) kv * a.k_nb1, col * 8);
            else    kreg[Q8 ? 0 : t] = *(const u32x4 *)(kb + (int64_t) kv * a.k_nb1 + col * 16);
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
    auto store_tile = [&]() {
#pragma unroll
        for (int t = 0; t < NKC; t++) {
            const int c = tid + t * NT, row = c / CPR, col = c % CPR;
            *(u32x4 *)(Kl + row * KSTR + col * 16) = Q8 ? q8_cvt(kraw[Q8 ? t : 0]) : kreg[Q8 ? 0 : t];
        }
#pragma unroll
        for (int t = 0; t < NVU; t++) {
            const int u = tid + t * NT, kvg = u / CPR, dvg = u % CPR;
            u32x4 x[4];
#pragma unroll
            for (int i = 0; i < 4; i++) x[i] = Q8 ? q8_cvt(vraw[Q8 ? 4 * t + i : 0]) : vreg[Q8 ? 0 : 4 * t + i];
            if ((16 * CPR) % NT == 0 || u < 16 * CPR) {
#pragma unroll
                for (int e = 0; e < 8; e++) {                          // 4 x 4 transposition in registers: V rows by position -> V^T rows by feature
                    const uint32_t sel = (e & 1) ? 0x07060302u : 0x05040100u;
                    const uint32_t lo = __builtin_amdgcn_perm(x[1][e >> 1], x[0][e >> 1], sel), up = __builtin_amdgcn_perm(x[3][e >> 1], x[2][e >> 1], sel);
                    *(u32x2 *)(Vl + (8 * dvg + e) * FA_VSTR + kvg * 8) = u32x2{lo, up};
                }
            }
        }
    };

    constexpr bool AHEAD = D <= 128;                                   // D = 256: a tile's rows are loaded and stored between its two barriers (no registers held over the math)
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
        if (!skip) store_tile();
        if (AHEAD && kv0 + 64 < kv_hi) load_tile(kv0 + 64);            // the next tile's loads fly under this tile's math
        if (skip) continue;
        __syncthreads();

        if (!wave_live) continue;                                      // (decode: the group's rows fit one wave; the others only help staging)
        // ---- S^T = K . Q^T: 2 KS MFMAs, K fragments read FA_PD ahead of their use; sched_barrier pins the order
        f32x16 s[2];
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) s[j][r] = 0.0f;
        {
            auto kfrag = [&](int idx) { return *(const half8 *)(Kl + (32 * (idx / KS) + l31) * KSTR + (2 * (idx % KS) + hi) * 16); };
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

        // ---- online soft-max (base 2) of the row held by this lane pair; m_run follows the running maximum lazily (FA_TAU), as in k_fattn
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

        // ---- O^T += V^T . P^T: 4 NB MFMAs, V^T fragments read FA_PD ahead
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

    // ---- epilogue: lane holds O^T[dv = 32 i + crow(r, hi), q = l31]: groups of 4 consecutive dv
    const float l_tot = fa_pair_sum(l_run);
    if (!rvalid) return;
    if (a.splits == 1) {
        const float inv = l_tot == 0.0f ? 0.0f : 1.0f / l_tot;
        char * dp = a.dst + (int64_t) n * a.d_nbn + (int64_t) h * a.d_nbh + (int64_t) b * a.d_nbb;
#pragma unroll
        for (int i = 0; i < NB; i++)
#pragma unroll
            for (int g = 0; g < 4; g++)
                *(f32x4 *)(dp + (32 * i + 8 * g + 4 * hi) * 4) = f32x4{o[i][4 * g] * inv, o[i][4 * g + 1] * inv, o[i][4 * g + 2] * inv, o[i][4 * g + 3] * inv};
    } else {
        float * pp = a.part + ((((int64_t) b * a.H + h) * a.N + n) * a.splits + split) * (D + 4);
#pragma unroll
        for (int i = 0; i < NB; i++)
#pragma unroll
            for (int g = 0; g < 4; g++)
                *(f32x4 *)(pp + 32 * i + 8 * g + 4 * hi) = f32x4{o[i][4 * g], o[i][4 * g + 1], o[i][4 * g + 2], o[i][4 * g + 3]};
        if (hi == 0) { pp[D] = m_run; pp[D + 1] = l_tot; }
    }
}

template <int D, int KVT, int MASK>
static int fattn_hs_go(hipStream_t st, const fattn_args & a, int B, bool decode) {
    constexpr int lds = 64 * (D * 2 + 16) + D * FA_VSTR;
    static_assert(lds <= 160 * 1024, "one CU's LDS");
    if (lds > 64 * 1024) { static uint64_t flag = 0; if (int rc = lds_opt_in(k_fattn_hs<D, KVT, MASK>, flag, lds)) return rc; }
    // decode: one workgroup per (split, KV group, batch), four waves stage, the wave that owns the packed rows computes; prefill: 128 query rows per workgroup
    const dim3 grid(decode ? (unsigned) a.splits : (unsigned)((a.N + 127) / 128), (unsigned)(a.H / a.R), (unsigned) B);
    hipLaunchKernelGGL((k_fattn_hs<D, KVT, MASK>), grid, dim3(256), lds, st, a);
    LAUNCH_CHECK();
    if (a.splits > 1) { hipLaunchKernelGGL((k_fattn_merge<D>), dim3((unsigned) a.N, (unsigned) a.H, (unsigned) B), dim3(1024), 0, st, a); LAUNCH_CHECK(); }
    return CLLM_OK;
}

int fattn_hs_launch(hipStream_t st, const fattn_args & a, int D, int ktype, int mmode, int B, bool decode) {
#define FA_HS_MASKS(D_, KVT_) do { if (mmode == 0) return fattn_hs_go<D_, KVT_, 0>(st, a, B, decode); if (mmode == 1) return fattn_hs_go<D_, KVT_, 1>(st, a, B, decode); \
                                   return fattn_hs_go<D_, KVT_, 2>(st, a, B, decode); } while (0)
    if (D == 96) { if (ktype == CLLM_TYPE_Q8_0) FA_HS_MASKS(96, CLLM_TYPE_Q8_0); FA_HS_MASKS(96, CLLM_TYPE_F16); }
    if (D == 256) { if (ktype == CLLM_TYPE_Q8_0) FA_HS_MASKS(256, CLLM_TYPE_Q8_0); FA_HS_MASKS(256, CLLM_TYPE_F16); }
#undef FA_HS_MASKS
    return CLLM_E_UNSUPPORTED;
}
