// philox.h -- the counter-based randomness the feeder (feed.hip) and the discriminator augmentation (augment.hip) share:
// Philox4x32-10 (Salmon et al., SC'11) and Box-Muller on word pairs.  Pure functions of their arguments; the counter
// layouts are in include/pdgn_hip.h, the host mirrors in tests/feed_mirror.py and tests/augment_mirror.py.
#pragma once
#include "common.h"

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned w[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// two normals from two words: u1 in (0, 1], u2 in [0, 1), both exact in fp32; the accurate logf / sincosf (the tests bound the
// deviation from an fp64 evaluation by a multiple of an fp32 host evaluation's own)
__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, float sigma, float &n0, float &n1) {
    float u1 = (float)((wa >> 8) + 1u) * 5.9604644775390625e-8f;
    float u2 = (float)(wb >> 8) * 5.9604644775390625e-8f;
    float rad = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.2831855f * u2, &s, &c);
    n0 = sigma * (rad * c);
    n1 = sigma * (rad * s);
}
