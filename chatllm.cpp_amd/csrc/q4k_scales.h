// q4k_scales.h -- the 6-bit scale / min unpack of a Q4_K / Q5_K super-block header, stated ONCE.  Plain C++ over uint32_t, nothing of HIP
// (tests/q4k_scales_main.cpp builds it with g++ alone and compares it with the byte-wise definition).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define Q4K_SCALES_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define Q4K_SCALES_FN static inline
#endif

// get_scale_min_k4 (ggml-quants.c:703-711) for the eight sub-blocks at once.  hy, hz, hw = bytes 0..3, 4..7, 8..11 of scales[12] as little-endian words (the words
// y, z, w of the 16-byte header {d, dmin, scales}).  Byte j of u0 = sc[j], of u1 = sc[4 + j], of u2 = m[j], of u3 = m[4 + j].
struct q4k_scales_t { uint32_t u0, u1, u2, u3; };
Q4K_SCALES_FN q4k_scales_t q4k_scales(uint32_t hy, uint32_t hz, uint32_t hw) {
    q4k_scales_t s;
    s.u0 = hy & 0x3f3f3f3fu;
    s.u2 = hz & 0x3f3f3f3fu;
    s.u1 = (hw & 0x0f0f0f0fu) | (((hy >> 6) & 0x03030303u) << 4);
    s.u3 = ((hw >> 4) & 0x0f0f0f0fu) | (((hz >> 6) & 0x03030303u) << 4);
    return s;
}
#undef Q4K_SCALES_FN
