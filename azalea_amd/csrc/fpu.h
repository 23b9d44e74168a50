// fpu.h -- first-play urgency (azx_set_fpu), shared by the tree kernels and the host (azx_fpu_score).  NOT the
// reference's behaviour: off by default, outside every parity claim.  include/azx.h has the definition.
//
// Where PUCT scores a node's children, a child with num_visits == 0 takes Q = fpu in place of -total_value / 1:
//     ABSOLUTE    fpu = value
//     REDUCTION   fpu = Qp - (r * sqrtf(mass)),   Qp = tv_p / max(nv_p, 1),   mass = (float)M / 2^24,
//                 M = the sum, over the node's children with num_visits > 0, of (uint32_t)(prior * 2^24)
// Every operation is one float32 operation (no contraction; the divide and the square root are IEEE's); M is an integer
// sum, so neither the lanes' order nor the shape of a reduction can change a bit of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/azx.h"

// one child's share of M (the caller adds it only where the child's num_visits > 0)
__host__ __device__ inline uint32_t azx_fpu_mass_word(float prior) { return (uint32_t)(prior * 16777216.0f); }

// Q of the unvisited children of a node with (nv_p, tv_p), for mode ABSOLUTE or REDUCTION; r is the reduction that
// holds at this node (root_reduction at the search's root, reduction below it)
__host__ __device__ inline float azx_fpu_q(int mode, float value, float r, float nv_p, float tv_p, uint32_t M) {
#pragma clang fp contract(off)
    if (mode == AZX_FPU_ABSOLUTE) return value;
    const float qp = tv_p / fmaxf(nv_p, 1.0f);
    const float mass = (float)M * (1.0f / 16777216.0f);
    const float red = r * sqrtf(mass);
    return qp - red;
}
