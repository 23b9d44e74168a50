// ext_kernels.hip -- the hand-over between the tree kernels and a caller-supplied evaluator (gfx950).
//
// The reference evaluates a search's leaf batch with net.run on (board, legal_moves) rows built on the host
// (mcts.py:170-215).  With an azx_eval_fn registered the engine hands a whole pool's leaf batch to the caller in
// DEVICE buffers instead: the search kernel queues requests in atomicAdd order (ev_*, azx_dev.h), k_ext_order puts
// them in (slot, leaf) order -- the order azx_get_leaves uses, so results do not depend on how the GPU scheduled the
// games -- k_ext_export widens them to the int32 rows the reference's network takes, and after the callback
// k_ext_import checks the results the way mcts.py:211-213 asserts and scatters the priors back by original cell.
// Export and import move about 9 B per cell and row each way: one wavefront per row, 4 B per lane.
#include "ext_kernels.h"

// hex.py:107-111 (r, c) -> (N-1-c, N-1-r)
__device__ __forceinline__ int ext_flip_cell(int cell, int N) {
    const int r = cell / N, c = cell - r * N;
    return (N - 1 - c) * N + (N - 1 - r);
}

// empties mask word s of a leaf, cut to the board's cells
__device__ __forceinline__ uint64_t ext_mask(const DevEngine &E, int src, int s) {
    const int nv = E.ncells - 64 * s;
    const uint64_t valid = nv >= 64 ? ~0ull : (nv <= 0 ? 0ull : ((1ull << nv) - 1ull));
    return E.leaf_mask[(size_t)src * 4 + s] & valid;
}

// evaluation index -> leaf slot: src2ev[ev_src[e]] = e for the n_eval pending requests
__global__ __launch_bounds__(256) void k_ext_map(DevEngine E, ExtBufs x) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = *E.n_eval, total = E.G * E.bs;
    if (e >= n || e >= total) return;
    const int src = E.ev_src[e];
    if (src >= 0 && src < total) x.src2ev[src] = e;
}

// exclusive scan of "has a request" over the leaf slots in (slot, leaf) order, 1024 slots per step (ballot prefix
// within each wave, wave totals through LDS); also the batch's largest legal-move count
__global__ __launch_bounds__(1024) void k_ext_scan(DevEngine E, ExtBufs x) {
    __shared__ int wave_tot[16];
    __shared__ int carry_s, kmax_s;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int total = E.G * E.bs;
    if (t == 0) { carry_s = 0; kmax_s = 0; }
    __syncthreads();
    int kmax = 0;
    for (int base = 0; base < total; base += 1024) {
        const int i = base + t;
        const int ev = i < total ? x.src2ev[i] : -1;
        const bool has = ev >= 0;
        const uint64_t b = __ballot(has);
        const int below = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[w] = __popcll(b);
        __syncthreads();
        int off = carry_s;
        for (int v = 0; v < w; ++v) off += wave_tot[v];
        if (has) {
            x.row_ev[off + below] = ev;
            int k = 0;
            for (int s = 0; s < 4; ++s) k += __popcll(ext_mask(E, i, s));
            kmax = k > kmax ? k : kmax;
        }
        __syncthreads();
        if (t == 0) {
            int sum = 0;
            for (int v = 0; v < 16; ++v) sum += wave_tot[v];
            carry_s += sum;
        }
        __syncthreads();
    }
    atomicMax(&kmax_s, kmax);
    __syncthreads();
    if (t == 0) {
        x.info[0] = carry_s;
        x.info[1] = kmax_s;
    }
}

// one wavefront per row: the int32 board and the legal list (ascending original cells, mapped through the flip
// when the mover is O and through the 180-degree turn when ev_flip bit 1 is set, + 1), zero-padded to the row width
// -- what azx_get_leaves builds on the host
__global__ __launch_bounds__(256) void k_ext_export(DevEngine E, ExtBufs x, int n) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int nc = E.ncells;
    const int e = x.row_ev[r];
    const int src = E.ev_src[e], flip = E.ev_flip[e];
    const uint8_t *b = E.ev_board + (size_t)e * AZX_CELL_STRIDE;
    int32_t *ob = x.board + (size_t)r * nc;
    int32_t *ol = x.legal + (size_t)r * nc;
    for (int c = lane; c < nc; c += 64) ob[c] = b[c];
    int pre = 0;
    for (int s = 0; s < 3; ++s) {
        const uint64_t m = ext_mask(E, src, s);
        const int c = s * 64 + lane;
        if ((m >> lane) & 1ull) {
            const int pos = pre + __popcll(m & ((1ull << lane) - 1ull));
            const int t = (flip & 1) ? ext_flip_cell(c, E.N) : c;
            ol[pos] = ((flip & 2) ? nc - 1 - t : t) + 1;            // bit 1: the board was turned by 180 degrees
        }
        pre += __popcll(m);
    }
    for (int p = pre + lane; p < nc; p += 64) ol[p] = 0;
}

// one wavefront per row: value -> ev_value, prior j -> ev_prior[cell of legal move j] (original frame, as
// azx_put_evals).  A row that fails mcts.py:211-213 (a prior < 0 or NaN, |sum of the k priors - 1| >= 1e-4) or has
// a value that is not finite is reported in info[2] (the smallest such row wins) and enters the tree as value 0 with
// uniform priors, so that the tree kernels never read what the checks rejected.
__global__ __launch_bounds__(256) void k_ext_import(DevEngine E, ExtBufs x, int n) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int nc = E.ncells;
    const int e = x.row_ev[r];
    const int src = E.ev_src[e];
    const float *pr = x.prior + (size_t)r * nc;
    uint64_t m[3];
    int pos[3];
    float p[3];
    int pre = 0;
    bool neg = false;
    float part = 0.0f;
    for (int s = 0; s < 3; ++s) {
        m[s] = ext_mask(E, src, s);
        pos[s] = -1;
        p[s] = 0.0f;
        if ((m[s] >> lane) & 1ull) {
            pos[s] = pre + __popcll(m[s] & ((1ull << lane) - 1ull));
            p[s] = pr[pos[s]];
            neg = neg || !(p[s] >= 0.0f);
            part += p[s];
        }
        pre += __popcll(m[s]);
    }
    const int k = pre;
    const float v = x.value[r];
    const float sum = wave_sum(part);
    const int bad = (isfinite(v) ? 0 : 1) | (__ballot(neg) ? 2 : 0) | (fabsf(sum - 1.0f) < 1e-4f ? 0 : 4);
    float *op = E.ev_prior + (size_t)e * AZX_CELL_STRIDE;
    const float uni = k > 0 ? 1.0f / (float)k : 0.0f;
    for (int s = 0; s < 3; ++s)
        if (pos[s] >= 0) op[s * 64 + lane] = bad ? uni : p[s];
    if (lane == 0) {
        E.ev_value[e] = bad ? 0.0f : v;
        if (bad) atomicMin(x.info + 2, (r << 3) | bad);
    }
}

void azx_launch_ext_order(const DevEngine &E, const ExtBufs &x, hipStream_t st) {
    const int total = E.G * E.bs;
    (void)hipMemsetAsync(x.src2ev, 0xff, sizeof(int32_t) * (size_t)total, st);
    hipLaunchKernelGGL(k_ext_map, dim3((total + 255) / 256), dim3(256), 0, st, E, x);
    hipLaunchKernelGGL(k_ext_scan, dim3(1), dim3(1024), 0, st, E, x);
}

void azx_launch_ext_export(const DevEngine &E, const ExtBufs &x, int n, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ext_export, dim3((n + 3) / 4), dim3(256), 0, st, E, x, n);
}

void azx_launch_ext_import(const DevEngine &E, const ExtBufs &x, int n, hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ext_import, dim3((n + 3) / 4), dim3(256), 0, st, E, x, n);
}
