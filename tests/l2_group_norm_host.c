/* tests/l2_group_norm_host.c -- TEST INFRASTRUCTURE.  The L2_NORM and GROUP_NORM part of chatllm.cpp_amd/csrc/norm_order.h -- the text k_l2_norm, k_l2_norm_wave and
 * k_group_norm (csrc/ops.hip) are built from -- behind a plain C interface: each node in the reference's order, and in a deliberately DIFFERENT order (pairwise sums)
 * guarded by the same interval tests and serial fallbacks as the device.  Plain C, no HIP: tests/test_l2_group_norm_model.py builds it alone with gcc
 * (-ffp-contract=off, as the kernels are compiled) and compares both with the reference's CPU backend.  Tensors are dense. */
#include <stdlib.h>

#include "../chatllm.cpp_amd/csrc/norm_order.h"

/* halves, recursively: no two of its additions but the very first are the serial chain's */
static double pair_sum(const double * t, long m) {
    if (m <= 0) return 0.0;
    if (m == 1) return t[0];
    return pair_sum(t, m / 2) + pair_sum(t + m / 2, m - m / 2);
}

/* ---- L2_NORM ---- */
void lg_l2_serial(long rows, long n, const float * x, float * y, float eps) {
    for (long r = 0; r < rows; r++, x += n, y += n) {
        const float scale = nm_l2_scale(nm_l2_serial_sumsq(x, n), eps);
        for (long i = 0; i < n; i++) y[i] = nm_l2_out(x[i], scale);
    }
}
/* guarded != 0: nm_l2_order_safe decides per row whether the pairwise total stands; guarded == 0: the pairwise totals as they are.  *fallbacks counts the rows that
 * redid the sum.  Returns 0, or -1 without memory. */
int lg_l2_pairwise(long rows, long n, const float * x, float * y, float eps, int guarded, long * fallbacks) {
    double * t = (double *) malloc(sizeof(double) * (size_t)(n + 1));
    if (!t) return -1;
    *fallbacks = 0;
    for (long r = 0; r < rows; r++, x += n, y += n) {
        for (long i = 0; i < n; i++) t[i] = (double)(x[i] * x[i]);
        double sum = pair_sum(t, n);
        if (guarded && !nm_l2_order_safe(sum, n)) { sum = nm_l2_serial_sumsq(x, n); (*fallbacks)++; }
        const float scale = nm_l2_scale(sum, eps);
        for (long i = 0; i < n; i++) y[i] = nm_l2_out(x[i], scale);
    }
    free(t);
    return 0;
}

/* ---- GROUP_NORM over a dense [ne0, ne1, C, ne3] ---- */
static void gn_finish(long N, const float * x, float * y, float mean, double V, float eps) {
    const float scale = nm_scale(nm_gn_variance(V, N), eps);
    for (long i = 0; i < N; i++) y[i] = nm_out(x[i], mean, scale);
}
/* mode 0: the reference's order (both two-level chains); 1: pairwise totals behind the interval tests; 2: pairwise totals as they are.  fallbacks[0] / [1] count the
 * groups that redid S / V.  A group without channels touches nothing.  Returns 0, or -1 without memory. */
int lg_group_norm(long ne0, long ne1, long C, long ne3, int n_groups, const float * x, float * y, float eps, int mode, long * fallbacks) {
    const long cpg = (long) nm_gn_channels_per_group(C, n_groups);
    const long nb1 = 4 * ne0, nb2 = nb1 * ne1, nb3 = nb2 * C;
    double * t = (double *) malloc(sizeof(double) * (size_t)(ne0 * ne1 * cpg + 1));
    if (!t) return -1;
    fallbacks[0] = fallbacks[1] = 0;
    for (long g = 0; g < n_groups; g++) {
        const long start = g * cpg, end = start + cpg < C ? start + cpg : C, step = end - start;
        if (step <= 0) continue;
        const long N = ne0 * ne1 * step;
        for (long i3 = 0; i3 < ne3; i3++) {
            const char * xb = (const char *) x + start * nb2 + i3 * nb3;
            const float * xg = (const float *) xb;                      /* dense: the group's N elements lie end to end, in the chains' order */
            float * yg = (float *)((char *) y + start * nb2 + i3 * nb3);
            double S, V;
            if (mode == 0) S = nm_gn_serial_sum(xb, ne0, ne1, step, nb1, nb2);
            else {
                double A;
                for (long i = 0; i < N; i++) t[i] = (double) xg[i];
                S = pair_sum(t, N);
                for (long i = 0; i < N; i++) t[i] = (double) fabsf(xg[i]);
                A = pair_sum(t, N);
                if (mode == 1 && !nm_gn_sum_order_safe(S, A, N)) { S = nm_gn_serial_sum(xb, ne0, ne1, step, nb1, nb2); fallbacks[0]++; }
            }
            const float mean = nm_gn_mean(S, N);
            if (mode == 0) V = nm_gn_serial_var_sum(xb, ne0, ne1, step, nb1, nb2, mean);
            else {
                for (long i = 0; i < N; i++) { const float v = xg[i] - mean; t[i] = (double)(v * v); }
                V = pair_sum(t, N);
                if (mode == 1 && !nm_gn_var_order_safe(V, N)) { V = nm_gn_serial_var_sum(xb, ne0, ne1, step, nb1, nb2, mean); fallbacks[1]++; }
            }
            gn_finish(N, xg, yg, mean, V, eps);
        }
    }
    free(t);
    return 0;
}
