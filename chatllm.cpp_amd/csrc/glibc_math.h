// glibc_math.h -- expf / sinf / cosf with the RESULTS of glibc 2.35's libm (the reference's CPU path calls them: the n mod 8 tail of
// ggml_vec_soft_max_f32 / ggml_vec_silu_f32, vec.cpp:396-431, 547-; the RoPE cache, ops.cpp:5589-5628), so that the device agrees with
// the host to the last bit where the device's own math library is only ~1 ulp close.  Restatement of the published algorithms of
// sysdeps/ieee754/flt-32/{e_expf.c, s_sinf.c, s_cosf.c, sincosf.h} (ARM optimized routines): everything is evaluated in double and
// rounded once to float, so only the operations' order matters, not the instruction selection.  Compiles for the host too:
// oracle/glibc_math_check.c compares it with the libm of this image over the float range (tests/test_oracle_vs_reference.py).
// Further down: tanhf / expm1f (float arithmetic, see there), the sigmoid expression, the fp32 <-> fp16 conversions and the two GELU tables
// of the element-wise activations (tests/test_unary_model.py compares them with the reference's CPU backend).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define GM_FN __host__ __device__ static inline
#define GM_TAB static __device__ const
#define GM_TAB_HOST static const
#else
#define GM_FN static inline
#define GM_TAB static const
#endif

GM_FN uint32_t gm_asuint(float f)    { uint32_t u; memcpy(&u, &f, 4); return u; }
GM_FN float    gm_asfloat(uint32_t u){ float f; memcpy(&f, &u, 4); return f; }
GM_FN uint64_t gm_asuint64(double f) { uint64_t u; memcpy(&u, &f, 8); return u; }
GM_FN double   gm_asdouble(uint64_t u){ double f; memcpy(&f, &u, 8); return f; }

// ---- expf (e_expf.c, exp2f_data.c: N = 32) -----------------------------------------------------------------------------------------
// T[i] = asuint64(2^(i/32)) - (i << 47); a table in constant memory on the device (a 32-way switch compiles to a branch tree that costs the
// one lane running a soft_max tail ~100 cycles per element)
#if defined(__HIPCC__)
__device__ __constant__ static const uint64_t gm_exp2f_T_dev[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull
};
#endif
static const uint64_t gm_exp2f_T_host[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull
};
GM_FN uint64_t gm_exp2f_tab(int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return gm_exp2f_T_dev[i & 31];
#else
    return gm_exp2f_T_host[i & 31];
#endif
}
// in two steps so that a device caller can fetch the table entry T[ki & 31] its own way between them (from LDS: decode_fused.hip) -- the arithmetic and its order are
// those of the one-piece function
GM_FN uint64_t gm_expf_ki(float x) {
    // z = InvLn2N * xd feeds two additions only: gcc fuses both (kd = z + SHIFT, r = z - kd) and z itself is never rounded
    return gm_asuint64(__builtin_fma(0x1.71547652b82fep+0 * 32, (double) x, 0x1.8p+52));
}
GM_FN float gm_expf_fin(float x, uint64_t ki, uint64_t t /* T[ki & 31] */) {
    const double xd = (double) x;
    const uint32_t abstop = (gm_asuint(x) >> 20) & 0x7ff;
    if (abstop >= 0x42b) {                                  // |x| >= 88 or nan
        if (gm_asuint(x) == 0xff800000u) return 0.0f;
        if (abstop >= 0x7f8) return x + x;
        if (x > 0x1.62e42ep6f) return gm_asfloat(0x7f800000u);                  // overflow
        if (x < -0x1.9fe368p6f) return 0.0f;                                    // underflow
        if (x < -0x1.9d1d9ep6f) return gm_asfloat(1u);                          // may-underflow: 0x1.4p-75f squared = the smallest subnormal
    }
    const double kd = gm_asdouble(ki) - 0x1.8p+52;
    const double r = __builtin_fma(0x1.71547652b82fep+0 * 32, xd, -kd);
    double z;
    t += ki << 47;
    const double s = gm_asdouble(t);
    // (the libm of this image runs its FMA build -- ifunc on x86-64-v3 hosts: the three multiply-adds are single roundings)
    z = __builtin_fma(0x1.c6af84b912394p-5 / 32 / 32 / 32, r, 0x1.ebfce50fac4f3p-3 / 32 / 32);
    const double r2 = r * r;
    double y = __builtin_fma(0x1.62e42ff0c52d6p-1 / 32, r, 1.0);
    y = __builtin_fma(z, r2, y);
    y = y * s;
    return (float) y;
}
GM_FN float gm_expf(float x) { const uint64_t ki = gm_expf_ki(x); return gm_expf_fin(x, ki, gm_exp2f_tab((int)(ki & 31))); }

// ---- sinf / cosf (s_sinf.c, s_cosf.c, sincosf.h, sincosf_data.c) -----------------------------------------------------------------------
GM_FN uint32_t gm_inv_pio4(int i) {        // the bits of 4/pi, 8 hex digits from every second digit on
    switch (i) {
        case 0: return 0xa2u; case 1: return 0xa2f9u; case 2: return 0xa2f983u; case 3: return 0xa2f9836eu; case 4: return 0xf9836e4eu; case 5: return 0x836e4e44u;
        case 6: return 0x6e4e4415u; case 7: return 0x4e441529u; case 8: return 0x441529fcu; case 9: return 0x1529fc27u; case 10: return 0x29fc2757u; case 11: return 0xfc2757d1u;
        case 12: return 0x2757d1f5u; case 13: return 0x57d1f534u; case 14: return 0xd1f534ddu; case 15: return 0xf534ddc0u; case 16: return 0x34ddc0dbu; case 17: return 0xddc0db62u;
        case 18: return 0xc0db6295u; case 19: return 0xdb629599u; case 20: return 0x6295993cu; case 21: return 0x95993c43u; case 22: return 0x993c4390u; default: return 0x3c439041u;
    }
}
// polynomial on [-pi/4, pi/4]; neg: the second table (c coefficients negated); odd n: cosine polynomial
GM_FN float gm_sincos_poly(double x, double x2, int neg, int n) {
    const double sg = neg ? -1.0 : 1.0;
    if ((n & 1) == 0) {
        const double s1c = -0x1.555545995a603p-3, s2c = 0x1.1107605230bc4p-7, s3c = -0x1.994eb3774cf24p-13;
        const double x3 = x * x2;
        const double s1 = s2c + x2 * s3c;
        const double x7 = x3 * x2;
        const double s = x + x3 * s1c;
        return (float)(s + x7 * s1);
    } else {
        const double c0 = sg * 0x1p0, c1c = sg * -0x1.ffffffd0c621cp-2, c2c = sg * 0x1.55553e1068f19p-5, c3c = sg * -0x1.6c087e89a359dp-10, c4c = sg * 0x1.99343027bf8c3p-16;
        const double x4 = x2 * x2;
        const double c2 = c3c + x2 * c4c;
        const double c1 = c0 + x2 * c1c;
        const double x6 = x4 * x2;
        const double c = c1 + x4 * c2c;
        return (float)(c + x6 * c2);
    }
}
GM_FN double gm_reduce_fast(double x, int * np) {
    const double r = x * 0x1.45F306DC9C883p+23;
    const int n = ((int32_t) r + 0x800000) >> 24;
    *np = n;
    return __builtin_fma(-(double) n, 0x1.921FB54442D18p0, x);      // the libm of this image runs its FMA build (ifunc): x - n * hpi is one rounding
}
GM_FN double gm_reduce_large(uint32_t xi, int * np) {
    const int a = (int)((xi >> 26) & 15);
    const int shift = (int)((xi >> 23) & 7);
    uint64_t n, res0, res1, res2;
    xi = (xi & 0xffffff) | 0x800000;
    xi <<= shift;
    res0 = (uint32_t)(xi * gm_inv_pio4(a));
    res1 = (uint64_t) xi * gm_inv_pio4(a + 4);
    res2 = (uint64_t) xi * gm_inv_pio4(a + 8);
    res0 = (res2 >> 32) | (res0 << 32);
    res0 += res1;
    n = (res0 + (1ull << 61)) >> 62;
    res0 -= n << 62;
    const double x = (double)(int64_t) res0;
    *np = (int) n;
    return x * 0x1.921FB54442D18p-62;
}
GM_FN double gm_sign(int n) { return ((n & 3) == 1 || (n & 3) == 2) ? -1.0 : 1.0; }     // sign[4] = { 1, -1, -1, 1 }
// which: 0 = sinf, 1 = cosf
GM_FN float gm_sincosf(float y, int which) {
    double x = (double) y;
    const uint32_t at = (gm_asuint(y) >> 20) & 0x7ff;
    int n;
    if (at < 0x3f4) {                                       // |y| < pi/4   (abstop12(0x1.921FB6p-1f) = 0x3f4)
        if (at < 0x398) return which ? 1.0f : y;            // |y| < 2^-12
        return gm_sincos_poly(x, x * x, 0, which);
    } else if (at < 0x42f) {                                // |y| < 120    (abstop12(120.0f) = 0x42f)
        x = gm_reduce_fast(x, &n);
        const double s = gm_sign(n);
        return gm_sincos_poly(x * s, x * x, (n & 2) != 0, n ^ which);
    } else if (at < 0x7f8) {
        const uint32_t xi = gm_asuint(y);
        const int sign = (int)(xi >> 31);
        x = gm_reduce_large(xi, &n);
        const double s = gm_sign(n + sign);
        return gm_sincos_poly(x * s, x * x, ((n + sign) & 2) != 0, n ^ which);
    }
    return y - y;                                           // inf / nan -> nan
}
GM_FN float gm_sinf(float y) { return gm_sincosf(y, 0); }
GM_FN float gm_cosf(float y) { return gm_sincosf(y, 1); }

// ---- tanhf (s_tanhf.c) over expm1f (s_expm1f.c): the fdlibm float routines glibc 2.35 still ships -------------------------------------
// Unlike expf above these are evaluated in FLOAT, every operation rounded on its own: the unit must be compiled without contraction
// (-ffp-contract=off), as glibc itself is, and the divisions are IEEE.  UNARY(TANH) (unary-ops.cpp:19-21) and the tanhf inside
// ggml_gelu_f32 (vec.h:976-978) call it.
#if defined(__HIP_DEVICE_COMPILE__)
#define GM_DIV(a, b) __fdiv_rn((a), (b))
#else
#define GM_DIV(a, b) ((a) / (b))
#endif
GM_FN float gm_expm1f(float x) {
    const float one = 1.0f, huge = 1.0e+30f, tiny = 1.0e-30f;
    const float o_threshold = 8.8721679688e+01f, ln2_hi = 6.9313812256e-01f, ln2_lo = 9.0580006145e-06f, invln2 = 1.4426950216e+00f;
    const float Q1 = -3.3333335072e-02f, Q2 = 1.5873016091e-03f, Q3 = -7.9365076090e-05f, Q4 = 4.0082177293e-06f, Q5 = -2.0109921195e-07f;
    float y, hi, lo, c = 0.0f, t, e, hxs, hfx, r1;
    int32_t k;
    uint32_t hx = gm_asuint(x);
    const uint32_t xsb = hx & 0x80000000u;                  // sign bit of x
    hx &= 0x7fffffffu;
    if (hx >= 0x4195b844u) {                                // |x| >= 27 ln2
        if (hx >= 0x42b17218u) {                            // |x| >= 88.721...
            if (hx > 0x7f800000u) return x + x;             // nan
            if (hx == 0x7f800000u) return xsb == 0 ? x : -1.0f;
            if (x > o_threshold) return gm_asfloat(0x7f800000u);                // huge * huge
        }
        if (xsb != 0) return tiny - one;                    // x < -27 ln2: -1
    }
    if (hx > 0x3eb17218u) {                                 // |x| > 0.5 ln2
        if (hx < 0x3F851592u) {                             // and |x| < 1.5 ln2
            if (xsb == 0) { hi = x - ln2_hi; lo =  ln2_lo; k =  1; }
            else          { hi = x + ln2_hi; lo = -ln2_lo; k = -1; }
        } else {
            k = (int32_t)(invln2 * x + (xsb == 0 ? 0.5f : -0.5f));
            t = (float) k;
            hi = x - t * ln2_hi;                            // t * ln2_hi is exact here
            lo = t * ln2_lo;
        }
        x = hi - lo;
        c = (hi - x) - lo;
    } else if (hx < 0x33000000u) {                          // |x| < 2^-25: x
        t = huge + x;
        return x - (t - (huge + x));
    } else k = 0;
    hfx = 0.5f * x;
    hxs = x * hfx;
    r1 = one + hxs * (Q1 + hxs * (Q2 + hxs * (Q3 + hxs * (Q4 + hxs * Q5))));
    t = 3.0f - r1 * hfx;
    e = hxs * GM_DIV(r1 - t, 6.0f - x * t);
    if (k == 0) return x - (x * e - hxs);                   // c is 0
    e = (x * (e - c) - c);
    e -= hxs;
    if (k == -1) return 0.5f * (x - e) - 0.5f;
    if (k == 1) {
        if (x < -0.25f) return -2.0f * (e - (x + 0.5f));
        return one + 2.0f * (x - e);
    }
    if (k <= -2 || k > 56) {                                // suffice to return exp(x) - 1
        y = one - (e - x);
        y = gm_asfloat(gm_asuint(y) + ((uint32_t) k << 23));                    // add k to y's exponent
        return y - one;
    }
    if (k < 23) {
        t = gm_asfloat(0x3f800000u - (0x1000000u >> k));    // 1 - 2^-k
        y = t - (e - x);
        y = gm_asfloat(gm_asuint(y) + ((uint32_t) k << 23));
    } else {
        t = gm_asfloat((uint32_t)(0x7f - k) << 23);         // 2^-k
        y = x - (e + t);
        y += one;
        y = gm_asfloat(gm_asuint(y) + ((uint32_t) k << 23));
    }
    return y;
}
GM_FN float gm_tanhf(float x) {
    const float one = 1.0f, two = 2.0f, tiny = 1.0e-30f;
    float t, z;
    const uint32_t jx = gm_asuint(x), ix = jx & 0x7fffffffu;
    if (ix >= 0x7f800000u) {
        if (ix > 0x7f800000u) return gm_asfloat(jx | 0x00400000u);             // one / x +- one on a nan: the nan itself, quiet (its sign and payload kept)
        return (jx >> 31) ? -one : one;                     // one / x +- one on +-inf
    }
    if (ix < 0x41b00000u) {                                 // |x| < 22
        if (ix == 0) return x;                              // +-0
        if (ix < 0x24000000u) return x * (one + x);         // |x| < 2^-55
        if (ix >= 0x3f800000u) {                            // |x| >= 1
            t = gm_expm1f(two * __builtin_fabsf(x));
            z = one - GM_DIV(two, t + two);
        } else {
            t = gm_expm1f(-two * __builtin_fabsf(x));
            z = GM_DIV(-t, t + two);
        }
    } else z = one - tiny;                                  // |x| >= 22: +-1
    return (jx >> 31) ? -z : z;
}

// ---- UNARY(SIGMOID): op_sigmoid, unary-ops.cpp:31-33: 1.f / (1.f + expf(-x)), libm expf per element, IEEE division ---------------------
GM_FN float gm_sigmoidf(float x) {
    if (x != x) return gm_asfloat((gm_asuint(x) ^ 0x80000000u) | 0x00400000u);  // the nan of -x, made quiet by expf's x + x, through + and / unchanged
    return GM_DIV(1.0f, 1.0f + gm_expf(-x));
}

// ---- fp32 <-> fp16 as the reference's x86-64-v3 build converts single values: GGML_CPU_FP32_TO_FP16 is NOT F16C there but the portable
// ggml_compute_fp32_to_fp16 (simd-mappings.h:143-145 -> ggml-impl.h:401-425: round to nearest even, every nan -> sign | 0x7e00), and
// GGML_CPU_FP16_TO_FP32 a lookup in ggml_table_f32_f16, filled by ggml_compute_fp16_to_fp32 (ggml-impl.h:378-399: exact; its float
// multiply turns a signalling nan quiet).  In integers here, so that host and device cannot differ.
GM_FN uint16_t gm_fp32_to_fp16(float f) {
    const uint32_t u = gm_asuint(f), a = u & 0x7fffffffu;
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                    // >= 65520 (the tie above the largest half goes to the even side: inf), inf
    uint32_t r, rem, half;
    if (a < 0x38800000u) {                                  // below the smallest normal half (2^-14): r = RNE(|f| * 2^24)
        if (a < 0x33000000u) return sign;                   // < 2^-25
        const uint32_t shift = 126u - (a >> 23), m = (a & 0x7fffffu) | 0x800000u;                  // 14 .. 24
        r = m >> shift; rem = m & ((1u << shift) - 1u); half = 1u << (shift - 1u);
    } else {
        r = (a - 0x38000000u) >> 13; rem = a & 0x1fffu; half = 0x1000u;                            // (a carry out of the mantissa steps the exponent)
    }
    if (rem > half || (rem == half && (r & 1u))) r++;
    return (uint16_t)(sign | r);
}
GM_FN float gm_fp16_to_fp32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    if (e == 0x1fu) return gm_asfloat(sign | 0x7f800000u | (m << 13) | (m ? 0x00400000u : 0u));
    if (e == 0u) return gm_asfloat(sign | gm_asuint((float)(int32_t) m * 0x1p-24f));               // zero and the subnormal halves: m * 2^-24, exact
    return gm_asfloat(sign | ((e + 112u) << 23) | (m << 13));
}

// ---- UNARY(GELU) / UNARY(GELU_QUICK) with GGML_GELU_FP16 / GGML_GELU_QUICK_FP16 (vec.h:17-18, the default build): a 65 536-entry fp16 table
// indexed by the fp16 rounding of x (ggml_vec_gelu_f32, vec.h:996-1009; ggml_vec_gelu_quick_f32, vec.h:1037-1044), filled by ggml_cpu_init
// (ggml-cpu.c:3694-3703) from ggml_gelu_f32 (vec.h:976-978) and ggml_gelu_quick_f32 (vec.h:1025-1027) with the host's tanhf / expf -- here
// with their restatements above, in float and uncontracted as that C11 unit is compiled.  Host side only: the device loads the tables.
GM_FN float gm_gelu_lookup(const uint16_t * tab /* gelu */, float x) {
    return x <= -10.0f ? 0.0f : x >= 10.0f ? x : gm_fp16_to_fp32(tab[gm_fp32_to_fp16(x)]);          // (a nan fails both tests: the table's nan entries)
}
GM_FN float gm_gelu_quick_lookup(const uint16_t * tab /* gelu_quick */, float x) { return gm_fp16_to_fp32(tab[gm_fp32_to_fp16(x)]); }      // no clamp: +-inf entries included
static inline float gm_gelu_f32(float x) {
    const float GELU_COEF_A = 0.044715f, SQRT_2_OVER_PI = 0.79788456080286535587989211986876f;
    return 0.5f * x * (1.0f + gm_tanhf(SQRT_2_OVER_PI * x * (1.0f + GELU_COEF_A * x * x)));
}
static inline float gm_gelu_quick_f32(float x) {
    const float GELU_QUICK_COEF = -1.702f;
    return x * (1.0f / (1.0f + gm_expf(GELU_QUICK_COEF * x)));
}
static inline void gm_build_gelu_tables(uint16_t * gelu /* [65536] */, uint16_t * gelu_quick /* [65536] */) {
    for (uint32_t i = 0; i < 65536u; i++) {
        const float f = gm_fp16_to_fp32((uint16_t) i);
        gelu[i]       = gm_fp32_to_fp16(gm_gelu_f32(f));
        gelu_quick[i] = gm_fp32_to_fp16(gm_gelu_quick_f32(f));
    }
}
