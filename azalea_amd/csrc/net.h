// net.h -- HexNetwork inference forward on gfx950 (net_kernels.hip): interface used by azx_capi.cpp
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "azx_dev.h"

struct AzxNet;

// tower_f16 != 0 (AZX_FLAG_TOWER_F16): the plain-f16 tower (k_tower_f16_s16, or k_stem_wide_f16 + k_conv_wide_f16_s16 per
// layer) instead of the split-f16 one; AZX_EINVAL when the shape has none or AZX_TOWER=fp32 is set (net_priv.h: TowerChoice)
int azx_net_create(AzxNet **out, int N, int blocks, int chans, int max_evals, int tower_f16, hipStream_t st);
// host only, no device call: what azx_net_kernel_info would report for the network azx_net_create would make of these
// arguments now, written to buf (truncated to cap - 1 bytes); its full length, or azx_net_create's refusal (< 0)
int azx_net_describe(int N, int blocks, int chans, int tower_f16, char *buf, int cap);
void azx_net_destroy(AzxNet *net);
// the engine re-made its stream (azx_reserve_cus): use `st` from now on and make the wide tower's side streams on the
// same CU mask (`mask` words, 0 words = all CUs); the old side streams are drained and dropped
void azx_net_set_stream(AzxNet *net, hipStream_t st, const uint32_t *mask, int words);
const char *azx_net_error();
int azx_net_set_weights(AzxNet *net, int n, const char *const *names, const void *const *ptrs,
                        const int64_t *counts, int on_device);
bool azx_net_ready(const AzxNet *net);
// AZX_ERANGE when a split-f16 or plain-f16 tower launch since the last check saw an activation beyond the f16 range (blocks on st)
int azx_net_check_range(AzxNet *net, hipStream_t st);
// packed buffer number `which` (name, bytes, contents); *nbytes = -1 past the last one
int azx_net_debug_weights(AzxNet *net, int which, void *out, int64_t cap, int64_t *nbytes, char *name, int name_cap);
const char *azx_net_kernel_info(const AzxNet *net);   // which tower / heads kernels this net launches
// evaluate the packed requests ev_board[0 .. *d.n_eval) -> ev_value, ev_prior (by original cell)
void azx_net_eval(AzxNet *net, const DevEngine &d, hipStream_t st);
// the same for a view of part of the pool (d's ev_* and n_eval point at that part's queue, of at most max_n requests),
// on scratch rows [row0, row0 + max_n): calls on disjoint row ranges may overlap on different streams -- when
// azx_net_rows_splittable (every tower but the wide one, whose layer launches run on side streams of their own)
bool azx_net_rows_splittable(const AzxNet *net);
void azx_net_eval_rows(AzxNet *net, const DevEngine &d, int row0, int max_n, hipStream_t st);
// the requests at and behind row `first` of that view (first < max_n), as a launch of its own after
// azx_net_eval_rows(net, d, row0, first, st) on the same stream: the two together evaluate what one call over max_n
// rows evaluates.  The kernels are the same ones on offset pointers; their count max(0, *d.n_eval - first) is written
// to ctr[0] by a one-thread kernel first (ctr: 4 ints of device scratch; [1..3] are azx_debug_stagger's), so the launch
// does nothing when fewer than `first` requests are queued.
// `first` must be a multiple of this: whole blocks of every tower and heads kernel (asserted in net_kernels.hip)
constexpr int AZX_NET_ROW_ALIGN = 16;
void azx_net_eval_rows_behind(AzxNet *net, const DevEngine &d, int row0, int first, int max_n, int32_t *ctr, hipStream_t st);
// Network.run on host arrays (network.py:87-105): value[B], moves_logprob[B][K]
int azx_net_forward_host(AzxNet *net, int B, int K, const int32_t *boards,
                         const int32_t *legal_moves, float *value, float *logprob, hipStream_t st);

// One 3x3 convolution of a wide tower (C a multiple of 128, boards up to 13x13) for the TRAINING step (train_wide.hip):
// k_conv_wide_f16x3_s16's staging and k-loop on a split-f16 image `in` [boards][cells][C hi | C lo] and one layer's
// fragments `w16` in the wide pack; writes the raw fp32 product times `*unscale` (a device word: the scales are made on
// the device) to out32 [boards][cells][C] and, when `stat` is given, per-board per-channel (sum, sum of squares) pairs
// [boards][C].
int azx_net_wide_train_conv(int N, int C, const unsigned short *w16, const unsigned short *in, float *out32, int n_boards,
                            const float *unscale, float2 *stat, hipStream_t st);
// The backward-data convolution of the same step with the next elementwise pass fused into its epilogue: writes
// g_{l-1} = (conv^T product [+ skip]) masked by act_{l-1} > 0 (`mask`: one bit per element, [boards][cells][C / 8] bytes, k_tw_bnact's), this board's (sum g, sum g xhat_{l-1}) pairs to pgsum
// [boards][C] (xhat from raw_{l-1} and BN_{l-1}'s batch sums `sums` [C][4 doubles], invN = 1 / (boards x cells)) and
// max |g| into *gmax (atomicMax on the float's bits).
int azx_net_wide_train_conv_bwd(int N, int C, const unsigned short *w16, const unsigned short *in, float *g_out, int n_boards,
                                const float *unscale, float2 *pgsum, const unsigned char *mask, const float *raw, const float *skip,
                                const double *sums, float invN, unsigned int *gmax, hipStream_t st);
