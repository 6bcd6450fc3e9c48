// norm_order.h -- the ordering rules of GGML_OP_NORM, written ONCE for the device (k_norm, ops.hip, through common.h) and for plain C (tests/norm_host.c, which
// tests/test_norm_model.py compiles alone with gcc and compares with the reference's CPU backend).  Nothing of HIP is needed to include it.  Not a public header.
//
// ggml_compute_forward_norm_f32 (ggml-cpu/ops.cpp:3643-3688) as the reference's x86-64-v3 build runs it (the AVX2 + FMA branch of ggml_vec_cvar_f32), per row of n floats:
//   S        = sum of (double) x[i], serially, i ascending                                  ggml_vec_sum_f32, vec.h:1510-1520
//   mean     = (float) S / (float) n                                                        ops.cpp:3669-3670: one float division
//   v_i      = x[i] - mean                                                                  ggml_vec_cvar_f32, vec.cpp:471-545
//   h_g      = ((q_0 + q_4) + (q_2 + q_6)) + ((q_1 + q_5) + (q_3 + q_7)), q_j = v_j * v_j   per whole group of 8, all in float, no fma (vec.cpp:484-494)
//   V        = sum of (double) h_g, groups ascending, then (double)(v_i * v_i) of the n % 8 leftovers one by one
//   variance = (float)(V / n)                                                               a double division (vec.cpp:544), then the conversion (ops.cpp:3680)
//   scale    = 1.0f / sqrtf(variance + eps)                                                 ops.cpp:3683
//   y[i]     = (x[i] - mean) * scale                                                        two roundings (the stored v_i, then ggml_vec_scale_f32), never an fma
// Compile uncontracted (-ffp-contract=off, as csrc/Makefile does): q_k + q_(k+4) must not become fma(v_k, v_k, q_(k+4)).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NM_FN __host__ __device__ static inline
#else
#define NM_FN static inline
#endif

// ---- the float steps (IEEE division and square root on either side: hipcc rounds both correctly by default, as rms_scale relies on) ----
// (S + 0.0: the serial chain starts from +0.0, so its total is never -0; a tree over a row of -0 alone can give -0, and the sign would reach every output)
NM_FN float nm_mean(double S, int64_t n)             { return (float)(S + 0.0) / (float) n; }
NM_FN float nm_variance(double V, int64_t n)         { return (float)(V / (double) n); }
NM_FN float nm_scale(float variance, float eps)      { return 1.0f / sqrtf(variance + eps); }
NM_FN float nm_out(float x, float mean, float scale) { const float v = x - mean; return v * scale; }
// one group of 8 centred values: _mm256_mul_ps, extractf128 + add, movehl + add, movehdup + add_ss (vec.cpp:488-493)
NM_FN float nm_group_h(float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7) {
    const float t0 = v0 * v0 + v4 * v4, t1 = v1 * v1 + v5 * v5, t2 = v2 * v2 + v6 * v6, t3 = v3 * v3 + v7 * v7;
    return (t0 + t2) + (t1 + t3);
}
NM_FN float nm_group_h_at(const float * x, float mean) {
    return nm_group_h(x[0] - mean, x[1] - mean, x[2] - mean, x[3] - mean, x[4] - mean, x[5] - mean, x[6] - mean, x[7] - mean);
}
NM_FN int64_t nm_var_terms(int64_t n) { return (n >> 3) + (n & 7); }       // what V adds: the group sums and the leftovers' squares

// ---- the serial chains: the reference's own order.  (The device runs these very additions with the terms fetched 64 at a time: norm_serial_sum and
// norm_serial_var_sum, common.h, which form each term with nm_group_h as here; tests/test_gpu_norm.py holds them to the reference on the rows that need them.) ----
NM_FN double nm_serial_sum(const float * x, int64_t n) {
    double S = 0.0;
    for (int64_t i = 0; i < n; i++) S += (double) x[i];
    return S;
}
NM_FN double nm_serial_var_sum(const float * x, int64_t n, float mean) {
    double V = 0.0;
    int64_t i = 0;
    for (; i + 7 < n; i += 8) V += (double) nm_group_h_at(x + i, mean);
    for (; i < n; i++) { const float v = x[i] - mean; V += (double)(v * v); }
    return V;
}

// ---- ORDER.  Whoever adds S or V in another order than the chains above (the workgroup of k_norm adds both as trees) asks these two tests, per row, whether the
// order can matter; where it can, the serial chain is run instead.
//
// S is a sum of SIGNED terms, so RMS_NORM's test (rms_scale, common.h: an interval relative to the sum itself) does not carry over: with cancellation S can be
// arbitrarily small against what the additions round.  The terms (double) x[i] are exact; a double sum of n terms in ANY order lies within gamma_(n-1) * sum|x_i| of the
// exact sum, gamma_k = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability, 4.2) -- so two orders differ by at most 2 gamma_(n-1) * sum|x_i|.  A = sum|x_i| comes
// through the same tree (itself within gamma_(n-1) of its exact value), and d = (2 n + 16) u A covers 2 gamma_(n-1) times the exact sum|x_i| plus the roundings of A, d,
// S - d and S + d for every n below 2^40.  All the op sees of S is (float) S, a monotonic conversion: when (float)(S - d) and (float)(S + d) are the same float, the
// serial S, which lies between them, converts to it too.  NaN (a NaN in the row; +inf and -inf; a lone inf, where d = inf and S - d = NaN) compares unequal: the serial
// chain runs and gives the same NaN / inf.  A finite S beyond the float range converts to inf at both ends: inf == inf, safe.
NM_FN int nm_sum_order_safe(double S, double A, int64_t n) {
    const double d = A * ((double)(2 * n + 16) * 0x1p-53);
    return (float)(S - d) == (float)(S + d);
}
// V is a sum of m NON-NEGATIVE terms, each an exact float that every order shares (h_g is a fixed float tree; a leftover's square one float product): the structure of the
// soft-max total (soft_total_order_safe, common.h) and of RMS_NORM's sum.  Two orders differ by at most 2 gamma_(m-1) of the value; all the op sees is
// (float)(V / n), monotonic in V.  The ends are formed by multiplication, so that V = inf (a float square overflowed: every order shares it) gives inf == inf: safe, no
// serial pass; V = NaN compares unequal and the serial chain gives NaN again.
NM_FN int nm_var_order_safe(double V, int64_t n) {
    const double r = (double)(2 * nm_var_terms(n) + 16) * 0x1p-53;
    return nm_variance(V * (1.0 - r), n) == nm_variance(V * (1.0 + r), n);
}

// ======== L2_NORM and GROUP_NORM: the other two normalisation nodes, under the same contract (k_l2_norm, k_l2_norm_wave, k_group_norm of ops.hip; tests/l2_group_norm_host.c,
// which tests/test_l2_group_norm_model.py compiles alone with gcc and compares with the reference's CPU backend) ========
//
// ggml_compute_forward_l2_norm_f32 (ggml-cpu/ops.cpp:4051-4092), per row of n floats:
//   sum      = sum of (double)(x[i] * x[i]), serially, i ascending, from +0.0                a float product, then widened (ops.cpp:4077-4080)
//   scale    = 1.0f / fmaxf(sqrtf((float) sum), eps)                                          ops.cpp:4086 (sqrtf takes a float: the double is converted first)
//   y[i]     = x[i] * scale                                                                   ggml_vec_scale_f32: one float multiply
// fmaxf returns its non-NaN operand: a row that holds a NaN has scale = 1 / eps (inf with eps = 0), so only the NaN elements and any 0 * inf are NaN; a row that holds an
// inf has scale = 0; a row of zeros has scale = 1 / eps.
//
// ggml_compute_forward_group_norm_f32 (ops.cpp:3956-4029), per (group, i03); the group's rows are (i02 in [start, end), i01 in [0, ne01)), N = ne00 * ne01 * (end - start):
//   S        = sum over the rows, (i02, i01) ascending, of sumr;  sumr = sum of (double) x[i00], serially from 0.0 per row      ops.cpp:3988-3999
//   mean     = (float)(S / (double) N)                                                        ops.cpp:4000: a double division, then the conversion (NORM divides floats)
//   v        = x - mean
//   V        = sum over the rows of sumr2;  sumr2 = sum of (double)(v * v), serially from 0.0 per row                          ops.cpp:4002-4017: a scalar loop, no groups of 8
//   variance = (float)(V / (double) N)                                                        ops.cpp:4018
//   scale    = 1.0f / sqrtf(variance + eps)                                                   ops.cpp:4019 (nm_scale)
//   y        = v * scale                                                                      two roundings, never an fma (nm_out)
NM_FN int nm_same_float(float a, float b) {                 // equal AND the same zero: -0 == +0 compares equal, but a mean of -0 and one of +0 give a -0 element different signs
    uint32_t p, q; __builtin_memcpy(&p, &a, 4); __builtin_memcpy(&q, &b, 4);
    return a == b && p == q;
}

// ---- the float steps ----
NM_FN float nm_l2_scale(double sum, float eps)      { return 1.0f / fmaxf(sqrtf((float) sum), eps); }
NM_FN float nm_l2_out(float x, float scale)         { return x * scale; }
NM_FN float nm_gn_mean(double S, int64_t N)         { return (float)((S + 0.0) / (double) N); }     // (S + 0.0: as in nm_mean, the chains start from +0.0 and never total -0)
NM_FN float nm_gn_variance(double V, int64_t N)     { return (float)(V / (double) N); }
NM_FN int64_t nm_gn_channels_per_group(int64_t C, int64_t n_groups) { return (C + n_groups - 1) / n_groups; }

// ---- the serial chains: the reference's own order.  GROUP_NORM's has two levels: a chain from 0.0 per row, the rows' totals added in (i02, i01) order.  `x` is the group's
// first row (channel `start` of batch i03); nb1, nb2 in bytes, as the tensor has them. ----
NM_FN double nm_l2_serial_sumsq(const float * x, int64_t n) {
    double sum = 0.0;
    for (int64_t i = 0; i < n; i++) sum += (double)(x[i] * x[i]);
    return sum;
}
NM_FN double nm_gn_serial_row_sq(const float * x, int64_t n, float mean) {
    double s = 0.0;
    for (int64_t i = 0; i < n; i++) { const float v = x[i] - mean; s += (double)(v * v); }
    return s;
}
NM_FN const float * nm_gn_row(const char * x, int64_t row, int64_t ne1, int64_t nb1, int64_t nb2) {      // row = (i02 - start) * ne1 + i01
    return (const float *)(x + (row % ne1) * nb1 + (row / ne1) * nb2);
}
NM_FN double nm_gn_serial_sum(const char * x, int64_t ne0, int64_t ne1, int64_t step, int64_t nb1, int64_t nb2) {
    double S = 0.0;
    for (int64_t row = 0; row < ne1 * step; row++) S += nm_serial_sum(nm_gn_row(x, row, ne1, nb1, nb2), ne0);
    return S;
}
NM_FN double nm_gn_serial_var_sum(const char * x, int64_t ne0, int64_t ne1, int64_t step, int64_t nb1, int64_t nb2, float mean) {
    double V = 0.0;
    for (int64_t row = 0; row < ne1 * step; row++) V += nm_gn_serial_row_sq(nm_gn_row(x, row, ne1, nb1, nb2), ne0, mean);
    return V;
}

// ---- ORDER: the three interval tests of these two nodes.  The reference's nested order (a chain per row, then a chain over the rows' totals; its additions to 0.0 are exact)
// is ONE particular summation tree of the N terms, and so is whatever a wave or a workgroup does instead.  The bound the tests rest on (Higham 4.2, as above: any double sum
// of m terms lies within gamma_(m-1) * sum|t_i| of the exact sum) holds for EVERY such tree, so two of them differ by at most 2 gamma_(m-1) * sum|t_i|.
//
// L2's sum: n non-negative terms, each an exact float product that every order shares -- RMS_NORM's structure.  All the op sees is (float) sum, monotonic.  The ends are
// formed by multiplication: sum = inf (a square overflowed, or an inf in the row: every order shares it) gives inf == inf, safe; sum = NaN compares unequal and the serial
// chain gives NaN again.
NM_FN int nm_l2_order_safe(double sum, int64_t n) {
    const double r = (double)(2 * n + 16) * 0x1p-53;
    return (float)(sum * (1.0 - r)) == (float)(sum * (1.0 + r));
}
// GROUP_NORM's S: N signed terms, so A = sum|x| through the same tree is needed, as for nm_sum_order_safe, and the comparison is of what THIS op sees, (float)(S / N):
// division by a positive N and the conversion are monotonic.  The two ends must also be the same zero (nm_same_float): a serial S of -1e-60 and a tree's +1e-60 both give a
// mean that compares equal to 0, with different signs.  NaN / inf: as nm_sum_order_safe.
NM_FN int nm_gn_sum_order_safe(double S, double A, int64_t N) {
    const double d = A * ((double)(2 * N + 16) * 0x1p-53);
    return nm_same_float(nm_gn_mean(S - d, N), nm_gn_mean(S + d, N));
}
// GROUP_NORM's V: N non-negative terms (one float square per element: N of them, not nm_var_terms), on (float)(V / N).  inf and NaN: as nm_var_order_safe.
NM_FN int nm_gn_var_order_safe(double V, int64_t N) {
    const double r = (double)(2 * N + 16) * 0x1p-53;
    return nm_gn_variance(V * (1.0 - r), N) == nm_gn_variance(V * (1.0 + r), N);
}
