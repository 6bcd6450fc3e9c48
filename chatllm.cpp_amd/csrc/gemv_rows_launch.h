#pragma once
// gemv_rows_launch.h -- the host side the three row-streaming decode mat-vecs share (k_gemv_rows, k_gemv_rows32, k_gemv_team32: the launches they take are k_gemv_dec's
// otherwise; that kernel's own host layer is gemv_decode_launch.h):
//   gemv_row_shape_ok()        the refusals of "a quantized matrix times one activation row quantized in the kernel"
//   gemv_row_lds()             the LDS sum: the activation row, Q4_0's c0 plane where the kernel keeps one, what the waves stage
//   K_GEMV_*_MAX_DYN_LDS       each kernel's dynamic-LDS cap: what its launcher refuses against AND what the attribute asks for
//   gemv_row_launch<>()        the attribute (once per device and instantiation) + the launch
//   gemv_row_by_type32(), gemv_row_by_pro_npre()     the ladders over the weight type and over (pro, npre)
// Host code only: which instantiations a translation unit holds, and in which order, is decided by the leaves its launcher names.
#include <type_traits>
#include "common.h"

#define K_GEMV_ROWS_MAX_DYN_LDS   (159 * 1024)      // (+ the prologue's static 128 bytes)
#define K_GEMV_ROWS32_MAX_DYN_LDS (159 * 1024)
// not k_gemv_dec's 160 KB - 256: Q4_0 needs about 2.25 K + 90112 bytes, so that cap would launch K 31857 .. 32653, which this one refuses and nothing has ever run
#define K_GEMV_TEAM32_MAX_DYN_LDS (158 * 1024)      // (+ the static 80 + 128 bytes)

// false: CLLM_E_UNSUPPORTED.  What is a kernel's own stays with its launcher: rows per wave or team, nblk %, grid caps, W's alignment, k_gemv_team32's K >= 256
static inline bool gemv_row_shape_ok(int wtype, int64_t K, int64_t nrows, int pro, int epi, const float * bias, const float * resid) {
    if (!is_quant_type(wtype) || K % wtype_blck(wtype) || pro < 1 || pro > 4 || nrows <= 0 || K > gemv_k_max(pro)) return false;
    const uint64_t row_bytes = cllm_row_size(wtype, K);
    if (row_bytes % 4 || (uint64_t) nrows * row_bytes >= (1ull << 32)) return false;      // rows are whole dwords; byte offsets into the matrix are 32-bit
    if (epi == 1 && (pro != 1 || bias || resid)) return false;                            // SiLU(gate) * up: behind the norm prologue only, nothing added
    return true;
}

static inline size_t gemv_row_lds(int wtype, int64_t K, bool c0_plane, size_t staged) {
    return act_row_bytes(K, act_kind_of(wtype)) + (c0_plane ? (size_t) K : 0) + staged;
}

template <auto KERNEL, int MAX_DYN_LDS, class... Args>
static int gemv_row_launch(hipStream_t st, int grid, size_t lds, Args... args) {
    static uint64_t attr = 0;
    if (const int rc = lds_opt_in(KERNEL, attr, MAX_DYN_LDS)) return rc;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned) grid), dim3(1024), lds, st, args...);
    LAUNCH_CHECK();
    return CLLM_OK;
}

template <int N> using gemv_c = std::integral_constant<int, N>;

// leaf(gemv_c<FMT>) for the three tuned 32-weight block formats (the launcher has refused every other type)
template <class Leaf>
static int gemv_row_by_type32(int wtype, Leaf && leaf) {
    return with_tuned_type(wtype, [&](auto t) -> int { if constexpr (wtype_blck(decltype(t)::value) == 32) return leaf(t); else return CLLM_E_UNSUPPORTED; });
}

// leaf(gemv_c<PRO>, gemv_c<NPRE>) for the pairs the prologue has (NPRE 8: the plain-quantize forms only, common.h gemv_k_max); the leaf names its kernel's instantiations
template <class Leaf>
static int gemv_row_by_pro_npre(int pro, int npre, Leaf && leaf) {
    if (pro == 1) return npre == 1 ? leaf(gemv_c<1>(), gemv_c<1>()) : leaf(gemv_c<1>(), gemv_c<4>());
    if (pro == 2) return npre == 1 ? leaf(gemv_c<2>(), gemv_c<1>()) : npre == 4 ? leaf(gemv_c<2>(), gemv_c<4>()) : leaf(gemv_c<2>(), gemv_c<8>());
    if (pro == 4) return npre == 1 ? leaf(gemv_c<4>(), gemv_c<1>()) : npre == 4 ? leaf(gemv_c<4>(), gemv_c<4>()) : leaf(gemv_c<4>(), gemv_c<8>());
    return               npre == 1 ? leaf(gemv_c<3>(), gemv_c<1>()) : leaf(gemv_c<3>(), gemv_c<4>());
}
