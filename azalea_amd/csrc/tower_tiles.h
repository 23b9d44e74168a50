// tower_tiles.h -- which cell sits in which row of which 16-row position tile of k_tower_f16x3_s16 (host only: no HIP
// dependency, so it also builds stand-alone).
//
// A block of the fused tower holds two boards as 256 LDS rows, row 128 * board + cell (cells >= N * N are dead rows).
// Its four waves own four position tiles ("slots") of 16 rows each.  A lane forms its LDS address from its own cell and
// an output element's sum does not depend on where it sits in a tile, so the membership is free:
//   rows   slot m of wave w holds the rows 64 w + 16 m .. + 15 (the identity: 16 consecutive cells of one board);
//   edge   slot AZX_TOWER_LIGHT_SLOT of waves 0..3 (the wave's "light" tile) holds 16 cells of the top row / the
//          bottom row / the left column / the right column (columns without the corners) of BOTH boards, topped up
//          with dead rows where a class has fewer than 16; all other rows fill the other 12 tiles in ascending order.
//          For three of the nine taps of a 3x3 convolution every row of such a tile reads padding: the kernel skips
//          those taps' MFMAs for the tile (skip[w], bit = tap, built from the tile's contents).
// Where a class cannot reach 16 rows even with dead rows the map is `rows`.
#pragma once
#include <stdint.h>

#define AZX_TOWER_LIGHT_SLOT 3   // the lagging last tile of the k-loop: no weight load sits in its MFMAs' shadow

struct AzxTowerTiles {
    uint8_t row[256];    // [wave 4][slot 4][tile row 16] -> LDS row
    uint32_t skip[4];    // per wave: taps (bit 3 (dy + 1) + dx + 1) that are padding for all 16 rows of the light tile
    int edge;            // 1: the edge map, 0: rows
};

// tap of LDS row L reads padding: a dead row, or a neighbour off the board
static inline bool azx_tile_tap_is_padding(int N, int L, int tap) {
    const int cell = L & 127;
    if (cell >= N * N) return true;
    const int y = cell / N + tap / 3 - 1, x = cell % N + tap % 3 - 1;
    return y < 0 || y >= N || x < 0 || x >= N;
}

static inline void azx_tower_tiles_rows(AzxTowerTiles *t) {
    for (int i = 0; i < 256; ++i) t->row[i] = (uint8_t)i;
    for (int w = 0; w < 4; ++w) t->skip[w] = 0u;
    t->edge = 0;
}

// ds_read_b128 serves a wave in groups of 16 lanes that mix the tile rows {4-7, 12-15} of one k-group with the rows
// {0-3, 8-11} of the next, which sits 8 slots of 16 B further in the LDS row (net_kernels.hip, lrow / lchunk); an LDS
// row starts on slot (row mod 16).  The two slot keys of a tile row in the two kinds of group:
static inline void azx_tile_slot_keys(int L, int tile_row, int *k1, int *k2) {
    const bool a = (tile_row & 4) == 0;                  // rows {0-3, 8-11}
    *k1 = (L + (a ? 8 : 0)) & 15;
    *k2 = (L + (a ? 0 : 8)) & 15;
}

static inline void azx_tower_tiles_build(int N, int edge, AzxTowerTiles *t) {
    azx_tower_tiles_rows(t);
    if (!edge || N < 2 || N * N > 121) return;
    const int ncells = N * N;
    // class of every LDS row: 0 top, 1 bottom, 2 left, 3 right, 4 interior, 5 dead
    int cls[256];
    for (int L = 0; L < 256; ++L) {
        const int cell = L & 127, y = cell / N, x = cell % N;
        cls[L] = cell >= ncells ? 5 : y == 0 ? 0 : y == N - 1 ? 1 : x == 0 ? 2 : x == N - 1 ? 3 : 4;
    }
    bool used[256] = {false};
    int light[4][16];
    for (int c = 0; c < 4; ++c) {
        // 16 rows of the class (dead rows once it is exhausted), each time the free row whose residue mod 16 is the
        // rarest in the tile so far: rows on one residue share their LDS banks
        int nres[16] = {0}, chosen[16];
        for (int k = 0; k < 16; ++k) {
            int best = -1;
            for (int pass = 0; pass < 2 && best < 0; ++pass)
                for (int L = 0; L < 256; ++L)
                    if (!used[L] && cls[L] == (pass ? 5 : c) && (best < 0 || nres[L & 15] < nres[best & 15])) best = L;
            if (best < 0) { azx_tower_tiles_rows(t); return; }     // not even with dead rows: the identity
            used[best] = true;
            ++nres[best & 15];
            chosen[k] = best;
        }
        // their order in the tile: each into the free tile row where it meets the fewest rows on its two slot keys
        int n1[16] = {0}, n2[16] = {0};
        bool taken[16] = {false};
        for (int k = 0; k < 16; ++k) {
            int best = -1, best_cost = 0;
            for (int r = 0; r < 16; ++r) {
                if (taken[r]) continue;
                int k1, k2;
                azx_tile_slot_keys(chosen[k], r, &k1, &k2);
                const int cost = n1[k1] + n2[k2];
                if (best < 0 || cost < best_cost) { best = r; best_cost = cost; }
            }
            int k1, k2;
            azx_tile_slot_keys(chosen[k], best, &k1, &k2);
            ++n1[k1];
            ++n2[k2];
            taken[best] = true;
            light[c][best] = chosen[k];
        }
    }
    int next = 0;                                        // every other row, ascending, into the other 12 tiles
    for (int w = 0; w < 4; ++w)
        for (int m = 0; m < 4; ++m)
            for (int r = 0; r < 16; ++r) {
                if (m == AZX_TOWER_LIGHT_SLOT) { t->row[64 * w + 16 * m + r] = (uint8_t)light[w][r]; continue; }
                while (used[next]) ++next;
                t->row[64 * w + 16 * m + r] = (uint8_t)next++;
            }
    for (int w = 0; w < 4; ++w) {
        uint32_t mask = 0u;
        for (int tap = 0; tap < 9; ++tap) {
            bool all = true;
            for (int r = 0; r < 16; ++r) all = all && azx_tile_tap_is_padding(N, t->row[64 * w + 16 * AZX_TOWER_LIGHT_SLOT + r], tap);
            if (all) mask |= 1u << tap;
        }
        t->skip[w] = mask;
    }
    t->edge = 1;
}
