// prints the type table as csrc/types.h generates it, one row per line (tests/test_types.py builds this with g++ alone: the header needs nothing of HIP):
//   name id size blck act_kind row_align quant kq k256 iq_grid get_rows
#include <stdio.h>
#include "../chatllm.cpp_amd/csrc/types.h"

int main() {
#define CLLM_WTYPE(name, id, bytes, elems, act, family, align, flags) \
    printf("%s %d %zu %d %d %d %d %d %d %d %d\n", #name, id, wtype_size(id), wtype_blck(id), act_kind_of(id), wtype_row_align(id), (int) is_quant_type(id), (int) is_kq_type(id), \
           (int) is_k256_type(id), (int) is_iq_grid_type(id), (int) wtype_has_get_rows(id));
#include "../chatllm.cpp_amd/csrc/types.def"
#undef CLLM_WTYPE
    static_assert(wtype_size(-1) == 0 && wtype_blck(63) == 0 && !is_quant_type(9) && !is_kq_type(9), "a type outside the table is nothing");
    int seen = 0;       // the ladders: each calls its leaf for its own family's rows and for nothing else
    for (int t = -1; t < 64; t++) {
        const int a = with_tuned_type(t, [&](auto c) { return 1000 + decltype(c)::value; }), b = with_kq_type(t, [&](auto c) { return 1000 + decltype(c)::value; });
        if ((a == 1000 + t) != is_quant_type(t) || (b == 1000 + t) != is_kq_type(t) || (a != 1000 + t && a != CLLM_E_UNSUPPORTED) || (b != 1000 + t && b != CLLM_E_UNSUPPORTED)) return 1;
        seen += (a == 1000 + t) + (b == 1000 + t);
    }
    return seen == 22 ? 0 : 2;
}
