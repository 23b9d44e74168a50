// policy_temp.h -- policy temperature of the search's priors (azx_set_policy_temp), shared by the tree kernels and the
// host (azx_policy_temp_row).  NOT the reference's behaviour: off by default, outside every parity claim.
// include/azx.h has the definition.
//
// temper(P[0..k), m), m in 1..8 eighths (temperature 8 / m), m == 8 the identity:
//     s1 = sqrtf(P_j), s2 = sqrtf(s1), s3 = sqrtf(s2)
//     q_j = the left-to-right product of those s whose bit of m is set (bit 2: s1, bit 1: s2, bit 0: s3) = P_j^(m/8)
//     Z   = the sum over j of (uint32_t)(q_j * 2^24)             Zf = (float)Z * 2^-24
//     result_j = q_j / Zf
// and the row comes back AS DELIVERED when a P_j is not finite, below 0 or above 1, or when Z == 0.
// Every operation is one float32 operation (no contraction; the divide and the square roots are IEEE's); Z is an integer
// sum, so neither the lanes' order nor the shape of a reduction can change a bit of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/azx.h"

// the guard on one element: true where the row must be left as delivered (a NaN fails both comparisons)
__host__ __device__ inline bool azx_pt_bad(float p) { return !(p >= 0.0f && p <= 1.0f); }

// q_j = P_j^(m/8) for m in 1..7, as a product of square roots
__host__ __device__ inline float azx_pt_q(float p, int m) {
#pragma clang fp contract(off)
    const float s1 = sqrtf(p);
    const float s2 = sqrtf(s1);
    const float s3 = sqrtf(s2);
    float q = 1.0f;                     // (1.0f * s is s: the product starts at the first selected root)
    if (m & 4) q = q * s1;
    if (m & 2) q = q * s2;
    if (m & 1) q = q * s3;
    return q;
}

// one element's share of Z
__host__ __device__ inline uint32_t azx_pt_word(float q) { return (uint32_t)(q * 16777216.0f); }

// Zf of a row's Z (Z != 0)
__host__ __device__ inline float azx_pt_zf(uint32_t Z) { return (float)Z * (1.0f / 16777216.0f); }
