// gemv_rows32.hip -- the decode step's mat-vec for the 32-weight block formats (Q4_0 / Q4_1 / Q8_0): a wave streams RPW rows side by side.
//
// Same contract as k_gemv_dec (gemv_decode_kernel.h): activation produced in the kernel (prologue 1..4), dst = W . act (+ bias) (+ resid) or the SiLU(gate) * up
// epilogue, every row accumulated in the ORDER of the reference's AVX2 ggml_vec_dot_q4_0_q8_0 / q4_1_q8_1 / q8_0_q8_0 (arch/x86/quants.c:543-577, 701-760, 1012-1040):
// per block b in row order and AVX lane A, acc[A] = fma(d_w d_x, (float) sumi[A], acc[A]) -- bit-identical to libggml-cpu.so.
//
// Why a second form: these formats fold the scale in every 32 weights (Q4_K: every 256), i.e. EIGHT serial fp32 chain steps per 18 / 20 / 34 bytes.  k_gemv_dec gives a
// row to a whole wave: one lane per block makes the eight integer sums and writes chain records to LDS, then lanes 0..7 walk the 64 blocks of records serially: 64 fma +
// 32 LDS reads with 8 of 64 lanes at work -- more instructions than the integer part itself, and the launch is instruction-issue bound (0.28 of the HBM roofline on
// Q4_0 gate/up).  Here a step is RPW rows x LPR = 64 / RPW blocks: lane (r, t) owns block t of row r in a step (same loads, same integer work), the records are
// [row][slot of A][t], and EVERY lane runs a chain: lane (r, j) walks the LPR blocks of row r for slot j -- LPR fma per step instead of 64 (RPW 8: 8).
// RPW is picked by the launcher so that there are at least ~8 units per CU (gate/up, lm_head: 8; the hidden-sized outputs: 2 or 4).
#include "gemv_act.h"
#include "q4k.h"
#include "q32.h"
#include "gemv_rows_launch.h"

#ifndef R32_P
#define R32_P 4
#endif

typedef int r32_i4 __attribute__((ext_vector_type(4)));
#define R32_REC_BYTES (64 * 9 * 4 + 2 * 256)          // per wave: RPW rows x 9 sub-rows (8 slots + d_w d_x) x LPR floats, then Q4_1's m_w[64], s_a[64]

template <int FMT, int PRO, int EPI, int NPRE, int RPW>
__global__ void __launch_bounds__(1024) k_gemv_rows32(const float * __restrict__ px, const float * __restrict__ pw, const char * __restrict__ W, int nblk, int nunits, float eps,
                                                      float * __restrict__ dst, const float * __restrict__ bias, const float * resid) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr bool IS_Q8 = FMT == CLLM_TYPE_Q8_0, IS_41 = FMT == CLLM_TYPE_Q4_1;
    constexpr int BS = q32_fmt<FMT>::BS, P = R32_P, LPR = 64 / RPW;
    const int tid = threadIdx.x, lane = tid & 63;
    const int K = nblk * 32;
    const unsigned nb01 = (unsigned) nblk * (unsigned) BS;
#ifndef R32_C0_PLANE
#define R32_C0_PLANE 0                                 // 1: Q4_0's (-8, -8, -8, -8) . a per (block, AVX lane) from a plane the prologue leaves in LDS; 0: taken on the fly (the LDS pipe is the busy unit)
#endif
    constexpr bool IS_40 = !IS_Q8 && !IS_41, NEED_C0 = IS_40 && R32_C0_PLANE;
    const unsigned arb = (unsigned) act_row_bytes(K, IS_41 ? ACT_Q8_1 : ACT_Q8_0);      // the activation row; Q4_0: then K bytes of c0[block][AVX lane] (int32)

    // ---- (1) this thread's activation groups: loads issued before anything else (gemv_act.h) ----
    const int e0 = tid * 4;
    f32x4 vv[NPRE], gg[NPRE];
    gemv_act_load<PRO, NPRE>(vv, gg, px, pw, K, e0);

    // ---- (2) this wave's units (RPW consecutive rows): (k * 16 + wave) * grid + block; the first P steps fly during the prologue.
    //          A block's bytes are loaded as the 4-byte aligned window around it (q32.h); rows are whole dwords, so a block starts in the upper half of its
    //          first dword exactly when its index is odd: the lane's byte selectors are constants ----
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = (nblk + LPR - 1) / LPR;                              // steps per unit
    const int ustride = 16 * gridDim.x, u0 = wave * gridDim.x + blockIdx.x;
    const int nmine = u0 < nunits ? (nunits - u0 + ustride - 1) / ustride : 0;
    const int r = lane / LPR, t = lane % LPR;
    const bool odd = !IS_41 && (t & 1);
    const uint32_t psel = odd ? 0x07060504u : 0x05040302u;             // v_perm_b32 selector: bytes 2..5 / 4..7 of a dword pair
    const unsigned lane_off = (unsigned) r * nb01 + (unsigned) t * BS - (odd ? 2u : 0u);
    u32x4 qa[P], qb[IS_Q8 ? P : 1];
    uint32_t qt[P];
    int iu = 0, is = 0;
    auto issue = [&](int p) {                                          // unconditional: out-of-range lanes re-read the unit's first block and are masked
        const bool ok = iu < nmine && LPR * is + t < nblk;
#ifdef R32_FAKE_COALESCED        /* timing experiment only (wrong results): every lane 16 contiguous, aligned bytes of the step's region */
        const char * bp = W + (size_t)(unsigned)(ok ? u0 + iu * ustride : u0 < nunits ? u0 : 0) * (size_t)(RPW * nb01) + (ok ? (unsigned)(is * 1152 + lane * 16) : 0u);
#else
        const char * bp = W + (size_t)(unsigned)(ok ? u0 + iu * ustride : u0 < nunits ? u0 : 0) * (size_t)(RPW * nb01) + (ok ? lane_off + (unsigned)(LPR * is) * BS : 0u);
#endif
        if (IS_41) { qt[p] = *(const uint32_t *) bp; qa[p] = *(const u32x4 *)(bp + 4); }
        else {
            qa[p] = *(const u32x4 *) bp;
            if (IS_Q8) { qb[IS_Q8 ? p : 0] = *(const u32x4 *)(bp + 16); qt[p] = *(const uint32_t *)(bp + 32); }
            else qt[p] = *(const uint32_t *)(bp + 16);
        }
        if (++is == S) { is = 0; iu++; }
    };
#pragma unroll
    for (int p = 0; p < P; p++) issue(p);

    // ---- (3) the activation row: [RMS_NORM * weight | SiLU * up |] quantize -> LDS, Q4_0's c0 plane behind it (gemv_act.h) ----
    __shared__ double part[16];
    gemv_act_store<32, IS_41, NEED_C0, PRO, NPRE>(lds, vv, gg, px, K, eps, e0, lane, part);
    __syncthreads();
    if (nmine == 0) return;

    // ---- (4) stream the units ----
    const int j = lane & 7;                                            // the chain this lane runs: slot j of row r
    const char * act = lds;
    const float * actd = (const float *)(lds + act_off_d(K));
    const float * acts = (const float *)(lds + act_off_s(K, IS_41 ? ACT_Q8_1 : ACT_Q8_0));
    float * rec = (float *)(lds + arb + (NEED_C0 ? K : 0) + wave * R32_REC_BYTES);
    float * X = rec + r * (9 * LPR) + t;                               // this lane's record column: X[slot * LPR], X[8 * LPR] = d_w d_x
    float * M = rec + 64 * 9;                                          // Q4_1: m_w[lane], s_a[64 + lane]
    const float * xr = rec + r * (9 * LPR) + j * LPR, * dr = rec + r * (9 * LPR) + 8 * LPR, * mr = M + r * LPR;
    float acc = 0.0f, accs = 0.0f;
    int cu = 0, cs = 0;
    while (cu < nmine) {
#pragma unroll
        for (int p = 0; p < P; p++) {
            const int b = LPR * cs + t;
            const bool ok = cu < nmine && b < nblk;
            const int bb = ok ? b : 0;
            // -- the block in place: h = fp16 d (Q4_1: | m << 16), q0 (q1) = the quant bytes
            uint32_t h; u32x4 q0, q1 = {0, 0, 0, 0};
            if (IS_41) { h = qt[p]; q0 = qa[p]; }
            else {
                const u32x4 a = qa[p];
                h = a.x >> (odd ? 16 : 0);
                auto pm = [&](uint32_t hi, uint32_t lo) { return __builtin_amdgcn_perm(hi, lo, psel); };
                if (IS_Q8) {
                    const u32x4 c = qb[IS_Q8 ? p : 0];
                    q0 = u32x4{pm(a.y, a.x), pm(a.z, a.y), pm(a.w, a.z), pm(c.x, a.w)};
                    q1 = u32x4{pm(c.y, c.x), pm(c.z, c.y), pm(c.w, c.z), pm(qt[p], c.w)};
                } else q0 = u32x4{pm(a.y, a.x), pm(a.z, a.y), pm(a.w, a.z), pm(qt[p], a.w)};
            }
            issue(p);
            // -- eight exact integer sums (q32_emit's arithmetic), records
            const u32x4 a0 = *(const u32x4 *)(act + bb * 32), a1 = *(const u32x4 *)(act + bb * 32 + 16);
            const float yd = actd[bb];
            int s[8];
            if (IS_Q8) {
                s[0] = dot4(q0.x, a0.x, 0); s[1] = dot4(q0.y, a0.y, 0); s[2] = dot4(q0.z, a0.z, 0); s[3] = dot4(q0.w, a0.w, 0);
                s[4] = dot4(q1.x, a1.x, 0); s[5] = dot4(q1.y, a1.y, 0); s[6] = dot4(q1.z, a1.z, 0); s[7] = dot4(q1.w, a1.w, 0);
            } else {
                r32_i4 c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};           // Q4_0: the prologue's c0 plane
                if (NEED_C0) { c0 = *(const r32_i4 *)(act + arb + bb * 32); c1 = *(const r32_i4 *)(act + arb + bb * 32 + 16); }
                else if (IS_40) {
                    c0 = r32_i4{dot4(0xf8f8f8f8u, a0.x, 0), dot4(0xf8f8f8f8u, a0.y, 0), dot4(0xf8f8f8f8u, a0.z, 0), dot4(0xf8f8f8f8u, a0.w, 0)};
                    c1 = r32_i4{dot4(0xf8f8f8f8u, a1.x, 0), dot4(0xf8f8f8f8u, a1.y, 0), dot4(0xf8f8f8f8u, a1.z, 0), dot4(0xf8f8f8f8u, a1.w, 0)};
                }
                s[0] = dot4(q0.x & 0x0f0f0f0fu, a0.x, c0.x); s[1] = dot4(q0.y & 0x0f0f0f0fu, a0.y, c0.y);
                s[2] = dot4(q0.z & 0x0f0f0f0fu, a0.z, c0.z); s[3] = dot4(q0.w & 0x0f0f0f0fu, a0.w, c0.w);
                s[4] = dot4((q0.x >> 4) & 0x0f0f0f0fu, a1.x, c1.x); s[5] = dot4((q0.y >> 4) & 0x0f0f0f0fu, a1.y, c1.y);
                s[6] = dot4((q0.z >> 4) & 0x0f0f0f0fu, a1.z, c1.z); s[7] = dot4((q0.w >> 4) & 0x0f0f0f0fu, a1.w, c1.w);
            }
            // slot of AVX lane A = 4(A&1) + (A&2) + (A>>2): [A0 A4 A2 A6 | A1 A5 A3 A7] (the hsum below)
#ifdef R32_FAKE_NOREC
            acc += __int_as_float((s[0] ^ s[1] ^ s[2] ^ s[3] ^ s[4] ^ s[5] ^ s[6] ^ s[7]) & 1) * yd + (ok ? h2f((uint16_t) h) : 0.0f);
#else
            X[0 * LPR] = (float) s[0]; X[1 * LPR] = (float) s[4]; X[2 * LPR] = (float) s[2]; X[3 * LPR] = (float) s[6];
            X[4 * LPR] = (float) s[1]; X[5 * LPR] = (float) s[5]; X[6 * LPR] = (float) s[3]; X[7 * LPR] = (float) s[7];
            X[8 * LPR] = ok ? h2f((uint16_t) h) * yd : 0.0f;          // a masked block: fma(0, finite, acc) = acc
            if (IS_41) { M[lane] = ok ? h2f((uint16_t)(h >> 16)) : 0.0f; M[64 + lane] = acts[bb]; }
#endif
            wave_lds_fence();
            // -- the chains: LPR blocks in row order
#ifndef R32_FAKE_NOCHAIN       /* timing experiments only (wrong results): R32_FAKE_NOCHAIN, R32_FAKE_NOREC, R32_FAKE_COALESCED */
#pragma unroll
            for (int i = 0; i < LPR; i += 4) {
                const f32x4 xv = *(const f32x4 *)(xr + i), dv = *(const f32x4 *)(dr + i);
                acc = __builtin_fmaf(dv.x, xv.x, acc); acc = __builtin_fmaf(dv.y, xv.y, acc); acc = __builtin_fmaf(dv.z, xv.z, acc); acc = __builtin_fmaf(dv.w, xv.w, acc);
                if (IS_41) {                                          // summs = fma(m_w, s_a, summs) (arch/x86/quants.c:726): the same chain in every lane of the row
                    const f32x4 mv = *(const f32x4 *)(mr + i), sv = *(const f32x4 *)(mr + 64 + i);
                    accs = __builtin_fmaf(mv.x, sv.x, accs); accs = __builtin_fmaf(mv.y, sv.y, accs); accs = __builtin_fmaf(mv.z, sv.z, accs); accs = __builtin_fmaf(mv.w, sv.w, accs);
                }
            }
#endif
            wave_lds_fence();
            if (++cs == S) {                                          // RPW rows complete: hsum_float_8 over the 8 slots (neighbour exchanges), epilogue, store
                const float hsum = gemv_hsum8(acc);
                float v = IS_41 ? hsum + accs : hsum;
                if (cu < nmine) {
                    const int unit = u0 + cu * ustride;
                    if (EPI == 1) {                                   // rows alternate gate_u, up_u: the up row is the next lane group
                        const float up = __int_as_float(__builtin_amdgcn_ds_bpermute(((lane + LPR) & 63) * 4, __float_as_int(v)));
                        if (t == 0 && !(r & 1)) dst[unit * (RPW / 2) + (r >> 1)] = silu_poly(v) * up;
                    } else {
                        if (bias || resid) v = gemv_bias_resid<RPW>(v, bias, resid, (size_t) unit * RPW, r);
                        if (t == 0) dst[(size_t) unit * RPW + r] = v;
                    }
                }
                acc = 0.0f; accs = 0.0f; cs = 0; cu++;
            }
        }
    }
}

static int g_rows32_mode = -1;
extern "C" __attribute__((visibility("default"))) void cllm_debug_set_gemv_rows32(int mode) { g_rows32_mode = mode; }      // tests / tools: 0 = k_gemv_dec, 1 = pick, 2 / 4 / 8 = force

// K % 32 == 0, rows whole dwords (Q4_0 / Q8_0: K % 64 == 0), nrows % RPW == 0; CLLM_E_UNSUPPORTED: k_gemv_dec takes the launch
int launch_gemv_rows32(hipStream_t st, int wtype, const void * W, int64_t K, int64_t nrows, int pro, const float * px, const float * pw, float eps, int epi, float * dst,
                       const float * bias, const float * resid) {
    if (g_rows32_mode < 0) g_rows32_mode = opt_int(OPT_CLLM_GEMV_ROWS32);      // 0: off, 2 / 4 / 8: that many rows per wave where the shape allows
    const int mode = g_rows32_mode;
    if (!mode || wtype == CLLM_TYPE_Q4_K || ((uintptr_t) W & 3) || !gemv_row_shape_ok(wtype, K, nrows, pro, epi, bias, resid)) return CLLM_E_UNSUPPORTED;
    if (epi == 1 && nrows % 2) return CLLM_E_UNSUPPORTED;
    const int nblk = (int)(K / 32), cus = device_cu_count();
    // rows per wave: 8 where that leaves >= 8 units per CU (gate/up, lm_head: 17.5 vs 29 us, 63 vs 120 us on Llama-3-8B Q4_0); the hidden-sized outputs have too few
    // rows for that -- one row per wave (k_gemv_dec) keeps 16 waves per CU busy and measured faster than 2 or 4 rows side by side (o: 7.3 vs 10.4 us, down: 21 vs 33 us).
    // 2 / 4 are kept for the tests and tools (cllm_debug_set_gemv_rows32 / CLLM_GEMV_ROWS32).
    int rpw = 0;
    if (mode == 1) { if (pro == 1 && nrows % 8 == 0 && nrows / 8 >= 8 * (int64_t) cus) rpw = 8; }
    else if ((mode == 2 || mode == 4 || mode == 8) && nrows % mode == 0 && (mode != 8 || pro == 1)) rpw = mode;
    if (!rpw) return CLLM_E_UNSUPPORTED;
    const int nunits = (int)(nrows / rpw);
    const int grid = (nunits + 15) / 16 < cus ? (nunits + 15) / 16 : cus;
    const size_t lds = gemv_row_lds(wtype, K, wtype == CLLM_TYPE_Q4_0 && R32_C0_PLANE, 16 * (size_t) R32_REC_BYTES);
    if (lds > K_GEMV_ROWS32_MAX_DYN_LDS) return CLLM_E_UNSUPPORTED;
    auto go = [&](auto fmt, auto epi_c) {
        return gemv_row_by_pro_npre(pro, gemv_npre(K), [&](auto pro_c, auto npre_c) {
            constexpr int FMT = decltype(fmt)::value, PRO = decltype(pro_c)::value, EPI = decltype(epi_c)::value, NPRE = decltype(npre_c)::value;
            auto run = [&](auto rpw_c) {
                return gemv_row_launch<k_gemv_rows32<FMT, PRO, EPI, NPRE, decltype(rpw_c)::value>, K_GEMV_ROWS32_MAX_DYN_LDS>(st, grid, lds, px, pw, (const char *) W, nblk, nunits, eps, dst, bias, resid);
            };
            if constexpr (PRO == 1) return rpw == 8 ? run(gemv_c<8>()) : rpw == 2 ? run(gemv_c<2>()) : run(gemv_c<4>());
            else if constexpr (EPI == 0) return rpw == 2 ? run(gemv_c<2>()) : run(gemv_c<4>());
            else return (int) CLLM_E_UNSUPPORTED;                      // (refused above: EPI 1 and 8 rows per wave exist behind the norm prologue only)
        });
    };
    return gemv_row_by_type32(wtype, [&](auto fmt) { return pro == 1 && epi == 1 ? go(fmt, gemv_c<1>()) : go(fmt, gemv_c<0>()); });
}
