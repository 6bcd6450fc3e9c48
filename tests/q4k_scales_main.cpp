// csrc/q4k_scales.h against get_scale_min_k4 written byte by byte from its definition (tests/test_q4k_scales.py builds this with g++ alone: the header needs
// nothing of HIP).  Headers: all zero, all 0xff, each of the 96 single-bit ones, 10 000 random ones from a fixed seed; all eight (sc, m) pairs, exact equality.
#include <stdio.h>
#include <string.h>
#include "../chatllm.cpp_amd/csrc/q4k_scales.h"

// the definition: sub-block j of the 12 scale bytes q -> 6-bit scale d and 6-bit min m
static void get_scale_min_k4(int j, const uint8_t * q, uint8_t * d, uint8_t * m) {
    if (j < 4) {
        *d = q[j] & 63;
        *m = q[j + 4] & 63;
    } else {
        *d = (uint8_t)((q[j + 4] & 0xF) | ((q[j - 4] >> 6) << 4));
        *m = (uint8_t)((q[j + 4] >> 4) | ((q[j] >> 6) << 4));
    }
}

static int check(const uint8_t * q) {
    uint32_t h[3];
    memcpy(h, q, 12);                       // the words y, z, w of the 16-byte block header as a little-endian device loads them
    const q4k_scales_t s = q4k_scales(h[0], h[1], h[2]);
    const uint32_t sc[2] = { s.u0, s.u1 }, mn[2] = { s.u2, s.u3 };
    for (int j = 0; j < 8; j++) {
        uint8_t d, m;
        get_scale_min_k4(j, q, &d, &m);
        if (((sc[j >> 2] >> (8 * (j & 3))) & 0xff) != d || ((mn[j >> 2] >> (8 * (j & 3))) & 0xff) != m) {
            fprintf(stderr, "sub-block %d of header", j);
            for (int i = 0; i < 12; i++) fprintf(stderr, " %02x", q[i]);
            fprintf(stderr, ": want (%u, %u), got (%u, %u)\n", d, m, (sc[j >> 2] >> (8 * (j & 3))) & 0xff, (mn[j >> 2] >> (8 * (j & 3))) & 0xff);
            return 1;
        }
    }
    return 0;
}

int main() {
    const uint16_t probe = 1;
    if (*(const uint8_t *) &probe != 1) { fprintf(stderr, "a little-endian host is needed\n"); return 2; }
    uint8_t q[12];
    int bad = 0, n = 0;
    memset(q, 0, 12);    bad += check(q); n++;
    memset(q, 0xff, 12); bad += check(q); n++;
    for (int b = 0; b < 96; b++) { memset(q, 0, 12); q[b >> 3] = (uint8_t)(1u << (b & 7)); bad += check(q); n++; }
    uint64_t x = 0x9e3779b97f4a7c15ull;     // xorshift64*, fixed seed
    for (int r = 0; r < 10000; r++) {
        for (int i = 0; i < 12; i++) { x ^= x >> 12; x ^= x << 25; x ^= x >> 27; q[i] = (uint8_t)((x * 0x2545f4914f6cdd1dull) >> 56); }
        bad += check(q); n++;
    }
    printf("%d headers, %d mismatches\n", n, bad);
    return bad ? 1 : 0;
}
