// replay_kernels.h -- launchers of the device replay ring kernels (replay_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/azx.h"

struct ReplayRows {          // struct of arrays over replay rows (harvest queue or ring)
    uint8_t *board;          // [rows][AZX_CELL_STRIDE]
    float *prob;             // [rows][AZX_CELL_STRIDE]
    int32_t *color, *k;      // [rows]
    float *reward;           // [rows]
};

// splitmix64's finalizer: the host mixes (seed, collate count) into a collate's key with it (azx_replay_set_reflect),
// k_replay_collate the key and the output row into that row's bit
__host__ __device__ inline unsigned long long azx_mix64(unsigned long long x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

void azx_launch_replay_put(const ReplayRows &src, const ReplayRows &ring, long long n, long long cap,
                           long long write_idx, hipStream_t st);
void azx_launch_replay_collate(const ReplayRows &ring, const long long *idx, int B, int ncells,
                               long long *color, int32_t *legal, long long *result, int32_t *board,
                               float *prob, float *reward, int32_t *max_k, int mover_n, int reflect,
                               unsigned long long reflect_key, hipStream_t st);
void azx_launch_rows_export(const uint8_t *qb, const float *qp, long long n, int ncells, int32_t *board,
                            float *prob, hipStream_t st);
void azx_launch_rows_pack(const ReplayRows &src, const long long *uid, long long first, long long n, int ncells,
                          uint8_t *rec, hipStream_t st);
void azx_launch_records_put(const uint8_t *rec, const ReplayRows &ring, long long n, long long cap,
                            long long write_idx, int ncells, hipStream_t st);
