/* tests/norm_host.c -- TEST INFRASTRUCTURE.  chatllm.cpp_amd/csrc/norm_order.h -- the text k_norm (csrc/ops.hip) is built from -- behind a plain C interface:
 * a row of GGML_OP_NORM in the reference's order, and in a deliberately DIFFERENT order (pairwise sums) guarded by the same interval tests and serial fallbacks as
 * the device.  Plain C, no HIP: tests/test_norm_model.py builds it alone with gcc (-ffp-contract=off, as the kernels are compiled) and compares both with the
 * reference's CPU backend. */
#include <stdlib.h>

#include "../chatllm.cpp_amd/csrc/norm_order.h"

static void finish(long n, const float * x, float * y, float mean, double V, float eps) {
    const float scale = nm_scale(nm_variance(V, n), eps);
    for (long i = 0; i < n; i++) y[i] = nm_out(x[i], mean, scale);
}

/* the reference's order: both serial chains */
void nh_rows_serial(long rows, long n, const float * x, float * y, float eps) {
    for (long r = 0; r < rows; r++, x += n, y += n) {
        const float mean = nm_mean(nm_serial_sum(x, n), n);
        finish(n, x, y, mean, nm_serial_var_sum(x, n, mean), eps);
    }
}

/* halves, recursively: no two of its additions but the very first are the serial chain's */
static void pair_sum_abs(const float * x, long n, double * s, double * a) {
    if (n <= 0) { *s = 0.0; *a = 0.0; return; }
    if (n == 1) { *s = (double) x[0]; *a = (double) fabsf(x[0]); return; }
    double s0, a0, s1, a1;
    pair_sum_abs(x, n / 2, &s0, &a0);
    pair_sum_abs(x + n / 2, n - n / 2, &s1, &a1);
    *s = s0 + s1; *a = a0 + a1;
}
static double pair_sum(const double * t, long m) {
    if (m <= 0) return 0.0;
    if (m == 1) return t[0];
    return pair_sum(t, m / 2) + pair_sum(t + m / 2, m - m / 2);
}

/* the other order.  guarded != 0: the interval tests of norm_order.h decide per row whether a pairwise total stands or the serial chain is run (what k_norm does with
 * its workgroup trees); guarded == 0: the pairwise totals as they are.  fallbacks[0] / [1] count the rows that redid S / V.  Returns 0, or -1 without memory. */
int nh_rows_pairwise(long rows, long n, const float * x, float * y, float eps, int guarded, long * fallbacks) {
    double * t = (double *) malloc(sizeof(double) * (size_t)(nm_var_terms(n) + 1));
    if (!t) return -1;
    fallbacks[0] = fallbacks[1] = 0;
    for (long r = 0; r < rows; r++, x += n, y += n) {
        double S, A;
        pair_sum_abs(x, n, &S, &A);
        if (guarded && !nm_sum_order_safe(S, A, n)) { S = nm_serial_sum(x, n); fallbacks[0]++; }
        const float mean = nm_mean(S, n);
        long m = 0, i = 0;
        for (; i + 7 < n; i += 8) t[m++] = (double) nm_group_h_at(x + i, mean);
        for (; i < n; i++) { const float v = x[i] - mean; t[m++] = (double)(v * v); }
        double V = pair_sum(t, m);
        if (guarded && !nm_var_order_safe(V, n)) { V = nm_serial_var_sum(x, n, mean); fallbacks[1]++; }
        finish(n, x, y, mean, V, eps);
    }
    free(t);
    return 0;
}
