/* tests/unary_host.c -- TEST INFRASTRUCTURE.  The host side of chatllm.cpp_amd/csrc/glibc_math.h behind a plain C interface: what the
 * element-wise kernels of csrc/ops.hip evaluate per element (gm_tanhf, gm_sigmoidf, the two table lookups) and the table builder the
 * library runs before its first GELU.  Plain C, no HIP: tests/test_unary_model.py builds it alone with gcc (-ffp-contract=off, as the
 * kernels are compiled) and compares it with the reference's CPU backend. */
#include "../chatllm.cpp_amd/csrc/glibc_math.h"

static uint16_t tab_gelu[1 << 16], tab_gelu_quick[1 << 16];
static int tab_ready = 0;
static void tables(void) { if (!tab_ready) { gm_build_gelu_tables(tab_gelu, tab_gelu_quick); tab_ready = 1; } }

void uh_build_tables(uint16_t * gelu, uint16_t * gelu_quick) { gm_build_gelu_tables(gelu, gelu_quick); }
void uh_fp32_to_fp16(long n, const float * x, uint16_t * y) { for (long i = 0; i < n; i++) y[i] = gm_fp32_to_fp16(x[i]); }
void uh_fp16_to_fp32(long n, const uint16_t * x, float * y) { for (long i = 0; i < n; i++) y[i] = gm_fp16_to_fp32(x[i]); }
/* op: the codes of cllm_unary (== ggml_unary_op); -1: SQR */
int uh_unary(int op, long n, const float * x, float * y) {
    tables();
    for (long i = 0; i < n; i++) {
        const float v = x[i];
        switch (op) {
            case 4:  y[i] = gm_tanhf(v); break;
            case 6:  y[i] = (v > 0.0f) ? v : 0.0f; break;
            case 7:  y[i] = gm_sigmoidf(v); break;
            case 8:  y[i] = gm_gelu_lookup(tab_gelu, v); break;
            case 9:  y[i] = gm_gelu_quick_lookup(tab_gelu_quick, v); break;
            case -1: y[i] = v * v; break;
            default: return -1;
        }
    }
    return 0;
}
