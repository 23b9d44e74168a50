// rollout_kernels.h -- the rollout evaluator (include/azx.h, "Rollout evaluator"): the mixers and the position key the
// host definition and the kernel share, the host definition itself, and the launchers of rollout_kernels.hip.
//
// NOT the reference's behaviour: its only network-free agent is RandomPolicy.  A Hex board that is full has exactly one
// winner and further stones never undo a win, so a uniformly random playout to the end is a uniformly random fill of
// the empty cells plus one connectivity test.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AZX_ROLLOUT_MAX 4096          // rollouts per position
#define AZX_ROLLOUT_FILLS 64          // filled boards azx_selftest_rollout returns per row (the first pass's lanes)

__host__ __device__ inline uint64_t azx_ro_sm(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__host__ __device__ inline uint32_t azx_ro_lb(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// key of rollout r of the position with key H
__host__ __device__ inline uint32_t azx_ro_key(uint64_t H, uint32_t r) {
    return azx_ro_lb((uint32_t)H ^ azx_ro_lb((uint32_t)(H >> 32) + r));
}

// the draw of empty cell c in the rollout with key k
__host__ __device__ inline uint32_t azx_ro_word(uint32_t k, uint32_t c) { return azx_ro_lb(k + c * 0x9E3779B9u); }

// The definition on the host, cell by cell with a stack flood fill (the kernel works on bit boards instead).  board:
// N*N values in {0, 1, 2}, already checked.  Returns the number of the R rollouts colour 1 wins.
inline int azx_rollout_host(uint64_t seed, int N, const int32_t *board, int R) {
    const int cells = N * N;
    uint64_t H = azx_ro_sm(seed);
    int e = 0;
    for (int c = 0; c < cells; ++c) {
        if (board[c]) H ^= azx_ro_sm(seed + 4ull * (uint64_t)c + (uint64_t)board[c]);
        else e += 1;
    }
    static const int di[6] = {-1, -1, 0, 0, 1, 1}, dj[6] = {0, 1, -1, 1, -1, 0};      // hex.py:192-197
    int wins = 0;
    uint8_t full[169], seen[169];
    int stack[169];
    for (int r = 0; r < R; ++r) {
        const uint32_t k = azx_ro_key(H, (uint32_t)r);
        uint32_t need = (uint32_t)(e + 1) >> 1, rem = (uint32_t)e;
        for (int c = 0; c < cells; ++c) {
            full[c] = (uint8_t)board[c];
            seen[c] = 0;
            if (board[c]) continue;
            if ((uint32_t)(((uint64_t)azx_ro_word(k, (uint32_t)c) * rem) >> 32) < need) { full[c] = 1; need -= 1; }
            else full[c] = 2;
            rem -= 1;
        }
        int top = 0;
        for (int j = 0; j < N; ++j)
            if (full[j] == 1) { seen[j] = 1; stack[top++] = j; }
        bool won = false;
        while (top > 0 && !won) {
            const int c = stack[--top], i = c / N, j = c - i * N;
            if (i == N - 1) { won = true; break; }
            for (int t = 0; t < 6; ++t) {
                const int a = i + di[t], b = j + dj[t];
                if (a < 0 || a >= N || b < 0 || b >= N) continue;
                const int d = a * N + b;
                if (full[d] == 1 && !seen[d]) { seen[d] = 1; stack[top++] = d; }
            }
        }
        wins += won ? 1 : 0;
    }
    return wins;
}

// R rollouts of each of the n int32 [cells] boards at board_dev (first player's view: the mover is colour 1):
// value_dev[r] = (2 wins - R) / R, prior_dev[r][j] = 1 / e for j < e and 0 up to the row's `cells` entries, wins_dev[r]
// = wins (may be null).  One wavefront per row, one lane per rollout.
void azx_launch_rollout(const int32_t *board_dev, int n, int N, int R, uint64_t seed, float *value_dev,
                        float *prior_dev, int32_t *wins_dev, hipStream_t stream);
// the same launch with its two optional extras: fills_dev uint8 [n][min(R, 64)][cells], the filled boards of the
// first rollouts (the self-test), and won_total_dev, one counter the rows' wins are added to (azx_rollout_stats)
void azx_launch_rollout_ex(const int32_t *board_dev, int n, int N, int R, uint64_t seed, float *value_dev,
                           float *prior_dev, int32_t *wins_dev, uint8_t *fills_dev, unsigned long long *won_total_dev,
                           hipStream_t stream);
