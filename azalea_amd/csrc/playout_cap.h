// playout_cap.h -- the per-ply draw of playout cap randomisation (azx_set_playout_cap), shared by the tree kernels and
// the host (azx_playout_cap_is_full).  NOT the reference's behaviour: off by default, outside every parity claim.
//
// One 32-bit word per (engine seed, game uid, ply from the empty board), from the game's key (game_rng: the two key
// words of seed + uid) on a stream of its own: both key words are salted before they meet the ply, so the word shares
// no intermediate value with the Dirichlet words (noise_base + select * golden), the reflection bits (noise_base ^ tag)
// or the Philox move draw.  Nothing else enters: not the slot, the pool size, the half-pool or the launch.
// The ply is a FULL search iff word <= thr_m1, with thr_m1 = ceil(full_prob * 2^32) - 1 clamped to [0, 2^32 - 1], an
// integer the host computes once: device and host agree exactly, full_prob == 1 makes every ply full, and the smallest
// full_prob still leaves the one word 0 full (probability 2^-32 per ply).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

__host__ __device__ inline uint32_t azx_cap_mix32(uint32_t x) {   // the tree kernels' mix32
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__host__ __device__ inline uint32_t azx_cap_word(uint64_t seed, int64_t uid, int ply) {
    const uint64_t s = seed + (uint64_t)uid;
    const uint32_t k0 = (uint32_t)s, k1 = (uint32_t)(s >> 32) ^ 0x5bd1e995u;   // the game's key (game_rng)
    return azx_cap_mix32((k0 ^ 0x50434150u) + azx_cap_mix32((k1 ^ 0x43415021u) + (uint32_t)ply * 0x2c1b3c6du));
}

__host__ __device__ inline bool azx_cap_is_full(uint64_t seed, int64_t uid, int ply, uint32_t thr_m1) {
    return azx_cap_word(seed, uid, ply) <= thr_m1;
}

// host only: the threshold of full_prob in (0, 1]
inline uint32_t azx_cap_threshold_m1(double full_prob) {
    const double t = ceil(ldexp(full_prob, 32));            // in [1, 2^32] for full_prob in (0, 1]
    if (t >= 4294967296.0) return 0xFFFFFFFFu;
    if (t <= 1.0) return 0u;
    return (uint32_t)((uint64_t)t - 1ull);
}
