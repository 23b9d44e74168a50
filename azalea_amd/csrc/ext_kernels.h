// ext_kernels.h -- launchers of the external-evaluator hand-over kernels (ext_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "azx_dev.h"

#define AZX_EXT_NO_ERROR 0x7fffffff   // info[2] while every imported row passed its checks

// device buffers of the hand-over between the tree kernels and a caller-supplied evaluator (azx_eval_fn)
struct ExtBufs {
    int32_t *src2ev;   // [G*bs] evaluation index of leaf slot g*bs+u, -1: no request (terminal / not selected)
    int32_t *row_ev;   // [G*bs] evaluation index of row r, rows in (slot, leaf) order
    int32_t *info;     // [4] rows n, kmax, first bad row << 3 | what failed (AZX_EXT_NO_ERROR: none), 0
    int32_t *board;    // [G*bs][ncells] int32 first player's view
    int32_t *legal;    // [G*bs][ncells] tile + 1 in the flipped frame, original order, 0-padded
    float *value;      // [G*bs]         evaluator output
    float *prior;      // [G*bs][ncells] evaluator output: entry j = legal move j
};

// row order of the pending requests (map ev_src -> rows, exclusive scan over the leaf slots): info[0] = n, info[1] = kmax
void azx_launch_ext_order(const DevEngine &E, const ExtBufs &x, hipStream_t st);
// ev_board / ev_flip / leaf_mask -> x.board / x.legal for rows [0, n)
void azx_launch_ext_export(const DevEngine &E, const ExtBufs &x, int n, hipStream_t st);
// x.value / x.prior -> ev_value / ev_prior (by original cell) with the checks of mcts.py:211-213 -> info[2]
void azx_launch_ext_import(const DevEngine &E, const ExtBufs &x, int n, hipStream_t st);
