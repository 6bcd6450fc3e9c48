// types.h -- what a tensor type IS, generated from types.def (the only list): traits, predicates and the dispatch ladders over the weight type.
// Plain C++17, nothing of HIP: g++ compiles it alone (tests/test_types.py does), host/ggml-hip.cpp includes it by relative path.
#pragma once

#include <stddef.h>
#include <type_traits>

#include "../../include/chatllm_hip.h"

#ifdef __HIPCC__
#define CLLM_HD __host__ __device__
#else
#define CLLM_HD
#endif

// the activation format's "kind" is its quantization block size (32 / 256); ACT_Q8_1 names the third flavour and maps to block size 32 (common.h: the act row layout)
enum { ACT_NONE = 0, ACT_Q8_0 = 32, ACT_Q8_K = 256, ACT_Q8_1 = 33 };

namespace wt {       // the words of types.def's columns
enum family { unknown = -1, plain, tuned, kq256, kq32 };
enum act    { none = ACT_NONE, q8_0 = ACT_Q8_0, q8_1 = ACT_Q8_1, q8_k = ACT_Q8_K };
enum flag   { no_flags = 0, iq_grid = 1, get_rows = 2 };
struct row { int id, bytes, elems, act, family, align, flags; };
CLLM_HD constexpr row of(int t) {
    switch (t) {
#define CLLM_WTYPE(name, id, bytes, elems, act, family, align, flags) case id: return row{ id, bytes, elems, act, family, align, flags };
#include "types.def"
#undef CLLM_WTYPE
    }
    return row{ -1, 0, 0, none, unknown, 0, no_flags };
}
#define CLLM_WTYPE(name, id, bytes, elems, act, family, align, flags) static_assert(CLLM_TYPE_##name == id, "types.def and include/chatllm_hip.h disagree on " #name);
#include "types.def"
#undef CLLM_WTYPE
}

CLLM_HD constexpr size_t wtype_size(int t)         { return (size_t) wt::of(t).bytes; }       // 0: not a type of the table
CLLM_HD constexpr int    wtype_blck(int t)         { return wt::of(t).elems; }
CLLM_HD constexpr int    wtype_row_align(int t)    { return wt::of(t).align; }
CLLM_HD constexpr int    act_kind_of(int t)        { return wt::of(t).act; }
CLLM_HD constexpr bool   is_quant_type(int t)      { return wt::of(t).family == wt::tuned; }
CLLM_HD constexpr bool   is_kq_type(int t)         { return wt::of(t).family == wt::kq256 || wt::of(t).family == wt::kq32; }
CLLM_HD constexpr bool   is_k256_type(int t)       { return wt::of(t).elems == 256; }
CLLM_HD constexpr bool   is_iq_grid_type(int t)    { return (wt::of(t).flags & wt::iq_grid) != 0; }
CLLM_HD constexpr bool   wtype_has_get_rows(int t) { return (wt::of(t).flags & wt::get_rows) != 0; }

// leaf(std::integral_constant<int, T>()) for the row of `wtype` among the FAMILIES named, in the table's order; CLLM_E_UNSUPPORTED (nothing called) for every other type.
// Host code only: which kernel instantiations a translation unit holds is decided by what its leaf names.
template <int F0, int F1, class Leaf>
static inline int with_type_of_family(int wtype, Leaf && leaf) {
#define CLLM_WTYPE(name, id, bytes, elems, act, family, align, flags) \
    if constexpr (wt::family == F0 || wt::family == F1) { if (wtype == id) return leaf(std::integral_constant<int, id>()); }
#include "types.def"
#undef CLLM_WTYPE
    return CLLM_E_UNSUPPORTED;
}
template <class Leaf> static inline int with_tuned_type(int wtype, Leaf && leaf) { return with_type_of_family<wt::tuned, wt::tuned>(wtype, leaf); }
template <class Leaf> static inline int with_kq_type(int wtype, Leaf && leaf)    { return with_type_of_family<wt::kq256, wt::kq32>(wtype, leaf); }
