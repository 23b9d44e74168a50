// selfplay_openings.h -- the per-game draw of the self-play opening book (azx_set_selfplay_openings), shared by the
// tree kernels and the host (azx_selfplay_opening_word, azx_selfplay_openings_bounds).  NOT the reference's behaviour
// (its games start from game.reset()): off by default, outside every parity claim.
//
// One 32-bit word per (engine seed, game uid), from the game's key (game_rng: the two key words of seed + uid) on a
// stream of its own: both key words are salted, with salts no other stream uses, before they are mixed, so the word
// shares no intermediate value with the Dirichlet words (noise_base + select * golden), the reflection bits
// (noise_base ^ tag), the playout-cap word (playout_cap.h), the resign-exemption word (resign.h), the Gumbel variates
// (gumbel.h: Philox on counters of their own) or the Philox move draw.  Nothing else enters: not the slot, the pool
// size, the half-pool, the launch or the ply.
// The bounds table of a book of n openings with weights W[o] >= 0 (all equal when none are given):
//   ub[o] = (uint64) floor(ldexp(cum[o] / cum[n-1], 32)),  cum the float64 running sum taken left to right,
//   ub[n-1] forced to 2^32,
// integers the host computes once.  Game u starts from the least o with word < ub[o]: device and host agree exactly, a
// zero-weight opening (ub[o] == ub[o-1], or ub[0] == 0) is never drawn, and the last opening with a positive weight
// takes every word the rounding of the quotients leaves over.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

__host__ __device__ inline uint32_t azx_book_mix32(uint32_t x) {   // the tree kernels' mix32
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__host__ __device__ inline uint32_t azx_book_word(uint64_t seed, int64_t uid) {
    const uint64_t s = seed + (uint64_t)uid;
    const uint32_t k0 = (uint32_t)s, k1 = (uint32_t)(s >> 32) ^ 0x5bd1e995u;   // the game's key (game_rng)
    return azx_book_mix32((k0 ^ 0x4f50454eu) + azx_book_mix32((k1 ^ 0x424f4f4bu) * 0x85ebca6bu + 0x73656174u));
}

// the least o in [0, n) with word < ub[o]; ub is non-decreasing and ub[n-1] == 2^32, so there is one.  A binary search:
// at most ceil(log2 n) <= 20 dependent loads (azx_openings_check holds n to 2^20).
__host__ __device__ inline int azx_book_index(uint32_t word, const uint64_t *ub, int n) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint64_t)word < ub[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// host only: the bounds of n weights (null: uniform).  Returns null, or what is wrong with the weights and in *bad the
// index of the offending one (-1: their sum).
inline const char *azx_book_bounds(int n, const double *weights, uint64_t *ub, int *bad) {
    double total = 0.0;
    *bad = -1;
    for (int o = 0; o < n; ++o) {
        const double w = weights ? weights[o] : 1.0;
        if (!isfinite(w)) { *bad = o; return "is not finite"; }
        if (w < 0.0) { *bad = o; return "is negative"; }
        total += w;                                             // (left to right: total is cum[n-1])
    }
    if (!isfinite(total)) return "sum is not finite";
    if (!(total > 0.0)) return "are all zero";
    double cum = 0.0;
    for (int o = 0; o < n; ++o) {
        cum += weights ? weights[o] : 1.0;
        const double t = floor(ldexp(cum / total, 32));         // in [0, 2^32]
        ub[o] = t >= 4294967296.0 ? (1ull << 32) : (uint64_t)t;
    }
    ub[n - 1] = 1ull << 32;
    return nullptr;
}
