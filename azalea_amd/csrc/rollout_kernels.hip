// rollout_kernels.hip -- the rollout evaluator's kernel (gfx950): value of a Hex position from uniformly random fills.
//
// include/azx.h ("Rollout evaluator") has the definition this kernel is held to bit for bit; rollout_kernels.h has the
// same definition on the host.  NOT the reference's behaviour (its only network-free agent is RandomPolicy).
//
// Layout: one wavefront per row (position), one lane per rollout, ceil(R / 64) passes.  The position is three
// wave-uniform bit boards of W 64-bit words (W = 1 up to 8x8, 2 up to 11x11, 3 up to 13x13): the lanes read the row's
// cells once and ballot them into empties and colour-1 stones, and XOR-reduce the position key.  Each lane then walks
// the empties in ascending order (a wave-uniform loop over the set bits), draws its own selection-sampling decisions
// and keeps its filled colour-1 board in W registers.  The connectivity test is a flood fill from the lane's colour-1
// cells of row 0: the six neighbour steps are word shifts by 1, N - 1 and N with the column-wrap bits cleared first.
// Every loop is bounded at launch: the fill by the empties' count (<= cells), the flood by `cells` steps (each step
// that changes anything adds a cell), the passes by R.  No atomics but one add per row to the statistics counter.
#include "rollout_kernels.h"

template <int W>
struct Bits {
    uint64_t w[W];
};

template <int W>
__device__ __forceinline__ Bits<W> bits_shl(const Bits<W> &a, int k) {   // 0 < k < 64
    Bits<W> o;
#pragma unroll
    for (int s = 0; s < W; ++s) o.w[s] = (a.w[s] << k) | (s > 0 ? a.w[s > 0 ? s - 1 : 0] >> (64 - k) : 0ull);
    return o;
}

template <int W>
__device__ __forceinline__ Bits<W> bits_shr(const Bits<W> &a, int k) {   // 0 < k < 64
    Bits<W> o;
#pragma unroll
    for (int s = 0; s < W; ++s) o.w[s] = (a.w[s] >> k) | (s < W - 1 ? a.w[s < W - 1 ? s + 1 : s] << (64 - k) : 0ull);
    return o;
}

__device__ __forceinline__ uint64_t wave_xor64(uint64_t v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo ^= (uint32_t)__shfl_xor((int)lo, off, 64);
        hi ^= (uint32_t)__shfl_xor((int)hi, off, 64);
    }
    return ((uint64_t)hi << 32) | lo;
}

template <int W>
__global__ __launch_bounds__(256) void k_rollout(const int32_t *__restrict__ board, int n, int N, int R, uint64_t seed,
                                                 float *__restrict__ value, float *__restrict__ prior,
                                                 int32_t *__restrict__ wins_out, uint8_t *__restrict__ fills,
                                                 unsigned long long *__restrict__ won_total) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                                   // (whole wavefronts leave: no barrier below)
    const int cells = N * N;
    const int32_t *b = board + (size_t)row * cells;

    // the position as wave-uniform bit boards, the geometry masks and the position key
    Bits<W> emp, stone1, notfirst, notlast, lastrow;
    uint64_t part = 0;
#pragma unroll
    for (int s = 0; s < W; ++s) {
        const int c = s * 64 + lane;
        const bool in = c < cells;
        const int v = in ? b[c] : 3;
        const int col = c % N;
        emp.w[s] = __ballot(v == 0);
        stone1.w[s] = __ballot(v == 1);
        notfirst.w[s] = __ballot(in && col != 0);
        notlast.w[s] = __ballot(in && col != N - 1);
        lastrow.w[s] = __ballot(in && c >= cells - N);
        if (in && v != 0) part ^= azx_ro_sm(seed + 4ull * (uint64_t)c + (uint64_t)v);
    }
    const uint64_t H = azx_ro_sm(seed) ^ wave_xor64(part);
    const uint64_t row0 = N >= 64 ? ~0ull : ((1ull << N) - 1ull);
    int e = 0;
#pragma unroll
    for (int s = 0; s < W; ++s) e += __popcll(emp.w[s]);

    int wins = 0;
    const int passes = (R + 63) >> 6;
    for (int p = 0; p < passes; ++p) {
        const int r = p * 64 + lane;
        const uint32_t k = azx_ro_key(H, (uint32_t)r);
        // selection sampling over the empties in ascending cell order: exactly (e + 1) >> 1 become colour 1
        Bits<W> one = stone1;
        uint32_t need = (uint32_t)(e + 1) >> 1, rem = (uint32_t)e;
#pragma unroll
        for (int s = 0; s < W; ++s) {
            uint64_t m = emp.w[s];
            for (int it = 0; it < 64 && m; ++it) {
                const int bit = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const uint32_t w = azx_ro_word(k, (uint32_t)(s * 64 + bit));
                if (__umulhi(w, rem) < need) {
                    one.w[s] |= 1ull << bit;
                    need -= 1;
                }
                rem -= 1;
            }
        }
        if (fills && p == 0 && r < R) {
            uint8_t *f = fills + ((size_t)row * (R < AZX_ROLLOUT_FILLS ? R : AZX_ROLLOUT_FILLS) + lane) * cells;
#pragma unroll
            for (int s = 0; s < W; ++s)
                for (int bit = 0; bit < 64 && s * 64 + bit < cells; ++bit)
                    f[s * 64 + bit] = ((one.w[s] >> bit) & 1ull) ? 1 : 2;
        }
        // flood fill from the colour-1 cells of row 0 (hex.py:192-197's six neighbours as shifts)
        Bits<W> reach;
#pragma unroll
        for (int s = 0; s < W; ++s) reach.w[s] = s == 0 ? (one.w[0] & row0) : 0ull;
        bool won = false;
        for (int it = 0; it < cells; ++it) {
            Bits<W> nf, nl;
#pragma unroll
            for (int s = 0; s < W; ++s) {
                nf.w[s] = reach.w[s] & notfirst.w[s];
                nl.w[s] = reach.w[s] & notlast.w[s];
            }
            const Bits<W> up = bits_shr<W>(reach, N), down = bits_shl<W>(reach, N);
            const Bits<W> left = bits_shr<W>(nf, 1), right = bits_shl<W>(nl, 1);
            const Bits<W> upright = bits_shr<W>(nl, N - 1), downleft = bits_shl<W>(nf, N - 1);
            uint64_t grown = 0, last = 0;
#pragma unroll
            for (int s = 0; s < W; ++s) {
                const uint64_t nb = up.w[s] | down.w[s] | left.w[s] | right.w[s] | upright.w[s] | downleft.w[s];
                const uint64_t nw = nb & one.w[s] & ~reach.w[s];
                reach.w[s] |= nw;
                grown |= nw;
                last |= reach.w[s] & lastrow.w[s];
            }
            won = last != 0;
            if (!__any(grown != 0 && !won)) break;
        }
        wins += __popcll(__ballot(won && r < R));
    }

    if (lane == 0) {
        value[row] = (float)(2 * wins - R) / (float)R;
        if (wins_out) wins_out[row] = wins;
        if (won_total) atomicAdd(won_total, (unsigned long long)wins);
    }
    const float uni = e > 0 ? 1.0f / (float)e : 0.0f;
    float *pr = prior + (size_t)row * cells;
    for (int j = lane; j < cells; j += 64) pr[j] = j < e ? uni : 0.0f;
}

void azx_launch_rollout_ex(const int32_t *board_dev, int n, int N, int R, uint64_t seed, float *value_dev,
                           float *prior_dev, int32_t *wins_dev, uint8_t *fills_dev, unsigned long long *won_total_dev,
                           hipStream_t stream) {
    if (n <= 0 || N < 2 || N > 13 || R < 1 || R > AZX_ROLLOUT_MAX) return;
    const dim3 grid((n + 3) / 4), block(256);
    if (N * N <= 64)
        hipLaunchKernelGGL(k_rollout<1>, grid, block, 0, stream, board_dev, n, N, R, seed, value_dev, prior_dev, wins_dev,
                           fills_dev, won_total_dev);
    else if (N * N <= 128)
        hipLaunchKernelGGL(k_rollout<2>, grid, block, 0, stream, board_dev, n, N, R, seed, value_dev, prior_dev, wins_dev,
                           fills_dev, won_total_dev);
    else
        hipLaunchKernelGGL(k_rollout<3>, grid, block, 0, stream, board_dev, n, N, R, seed, value_dev, prior_dev, wins_dev,
                           fills_dev, won_total_dev);
}

void azx_launch_rollout(const int32_t *board_dev, int n, int N, int R, uint64_t seed, float *value_dev,
                        float *prior_dev, int32_t *wins_dev, hipStream_t stream) {
    azx_launch_rollout_ex(board_dev, n, N, R, seed, value_dev, prior_dev, wins_dev, nullptr, nullptr, stream);
}
