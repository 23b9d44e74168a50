// resign.h -- the per-game exemption draw of resignation (azx_set_resign), shared by the tree kernels and the host
// (azx_resign_is_exempt).  NOT the reference's behaviour: off by default, outside every parity claim.
//
// One 32-bit word per (engine seed, game uid), from the game's key (game_rng: the two key words of seed + uid) on a
// stream of its own: both key words are salted, with salts no other stream uses, before they are mixed, so the word
// shares no intermediate value with the Dirichlet words (noise_base + select * golden), the reflection bits
// (noise_base ^ tag), the playout-cap word (playout_cap.h salts the same key words differently and folds the ply in)
// or the Philox move draw.  Nothing else enters: not the slot, the pool size, the half-pool or the launch.
// The game is EXEMPT from resigning (a no-resign calibration game) iff keep_prob > 0 and word <= thr_m1, with
// thr_m1 = ceil(keep_prob * 2^32) - 1, an integer the host computes once: device and host agree exactly,
// keep_prob == 1 exempts every game and keep_prob == 0 none (the host passes that case as a mode of its own:
// AZX_RESIGN_NONE_EXEMPT, since -1 is no threshold).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

// DevEngine::resign_mode
#define AZX_RESIGN_OFF 0
#define AZX_RESIGN_NONE_EXEMPT 1     // keep_prob == 0
#define AZX_RESIGN_DRAW_EXEMPT 2     // keep_prob in (0, 1]: exempt iff azx_resign_word(seed, uid) <= thr_m1

__host__ __device__ inline uint32_t azx_resign_mix32(uint32_t x) {   // the tree kernels' mix32
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__host__ __device__ inline uint32_t azx_resign_word(uint64_t seed, int64_t uid) {
    const uint64_t s = seed + (uint64_t)uid;
    const uint32_t k0 = (uint32_t)s, k1 = (uint32_t)(s >> 32) ^ 0x5bd1e995u;   // the game's key (game_rng)
    return azx_resign_mix32((k0 ^ 0x52534e31u) + azx_resign_mix32((k1 ^ 0x4b454550u) * 0x9e3779b1u + 0x6e6f7273u));
}

__host__ __device__ inline bool azx_resign_exempt(uint64_t seed, int64_t uid, int mode, uint32_t thr_m1) {
    return mode == AZX_RESIGN_DRAW_EXEMPT && azx_resign_word(seed, uid) <= thr_m1;
}

// host only: the threshold of keep_prob in (0, 1]
inline uint32_t azx_resign_threshold_m1(double keep_prob) {
    const double t = ceil(ldexp(keep_prob, 32));            // in [1, 2^32] for keep_prob in (0, 1]
    if (t >= 4294967296.0) return 0xFFFFFFFFu;
    if (t <= 1.0) return 0u;
    return (uint32_t)((uint64_t)t - 1ull);
}
