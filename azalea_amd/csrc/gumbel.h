// gumbel.h -- the noise of the Gumbel root search (azx_set_gumbel), shared by the tree kernels and the host
// (azx_gumbel_variate, azx_selftest_gumbel).  NOT the reference's behaviour: off by default, outside every parity claim.
//
// One Gumbel(0, 1) variate per (engine seed, game uid, ply from the empty board, root child index j): word j & 3 of
//     Philox4x32-10(key of seed + uid).gen(0x47554D42, ply, j >> 2, 0x4E4F4953)
// -- the game's key (game_rng) on a counter of its own, so nothing is shared with the move draw (0xC0FFEE, ..) -- then
//     u = ((word >> 8) + 1/2) / 2^24,  g = -ln(-ln u).
// The host computes g in double precision.  The device returns a float32: for the upper half of the 24-bit values u is
// not a float32 (2^24 - 1/2 rounds to 2^24), so -ln u is taken there as -log1pf(-y) of the complement
// y = ((word >> 8 ^ 0xffffff) + 1/2) / 2^24, which is one; both logarithms are the accurate library functions, not the
// fast intrinsics.  g lies in [-2.86, 17.33].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#define AZX_GUMBEL_C0 0x47554D42u
#define AZX_GUMBEL_C3 0x4E4F4953u

__host__ __device__ inline void azx_philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2,
                                                  uint32_t c3, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the raw word of child j (host and device agree exactly)
__host__ __device__ inline uint32_t azx_gumbel_word(uint64_t seed, int64_t uid, int ply, int child) {
    const uint64_t s = seed + (uint64_t)uid;
    uint32_t r[4];
    azx_philox4x32_10((uint32_t)s, (uint32_t)(s >> 32) ^ 0x5bd1e995u, AZX_GUMBEL_C0, (uint32_t)ply,
                      (uint32_t)(child >> 2), AZX_GUMBEL_C3, r);
    return r[child & 3];
}

// host: the definition, in double precision
inline double azx_gumbel_of_word_host(uint32_t word) {
    const double u = ((double)(word >> 8) + 0.5) / 16777216.0;
    return -log(-log(u));
}

// device: float32, accurate logarithms
__device__ inline float azx_gumbel_of_word(uint32_t word) {
    const uint32_t x = word >> 8;
    float t;                                                   // -ln u
    if (x & 0x800000u) t = -log1pf(-(((float)(x ^ 0xffffffu) + 0.5f) * (1.0f / 16777216.0f)));
    else t = -logf(((float)x + 0.5f) * (1.0f / 16777216.0f));
    return -logf(t);
}
