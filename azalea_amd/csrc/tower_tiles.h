// tower_tiles.h -- which cell sits in which row of which 16-row position tile of k_tower_f16x3_s16 (host only: no HIP
// dependency, so it also builds stand-alone).
//
// A block of the fused tower holds two boards as 256 rows, row L = 128 * board + cell (cells >= N * N are dead rows; in
// the LDS image board 1 starts AZX_TOWER_BOARD_GAP rows later: azx_tile_lds_row).
// Its four waves own four position tiles ("slots") of 16 rows each.  A lane forms its LDS address from its own cell and
// an output element's sum does not depend on where it sits in a tile, so the membership is free:
//   rows   slot m of wave w holds the rows 64 w + 16 m .. + 15 (the identity: 16 consecutive cells of one board);
//   edge   slot AZX_TOWER_LIGHT_SLOT of waves 0..3 (the wave's "light" tile) holds 16 cells of the top row / the
//          bottom row / the left column / the right column (columns without the corners) of BOTH boards, topped up
//          with dead rows where a class has fewer than 16; all other rows fill the other 12 tiles.  Every tile takes
//          rows of 16 different residues mod 16 in the LDS image wherever its rows reach that many, each in the tile
//          row of its residue, so that its reads are as free of bank conflicts as those of 16 consecutive rows.
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

// The block's LDS image keeps board 1 eight rows behind board 0's 128: with the boards 128 rows apart a cell had the
// same residue mod 16 on either board and 16 cells of one edge of the two boards could not have 16 different ones.
// The 8 rows between the boards are never read (a tap that would reach them is padding).
#define AZX_TOWER_BOARD_GAP 8
#define AZX_TOWER_LDS_ROWS (256 + AZX_TOWER_BOARD_GAP)
static inline int azx_tile_lds_row(int L) { return L + AZX_TOWER_BOARD_GAP * (L >> 7); }

// ds_read_b128 serves a wave in groups of 16 lanes that mix the tile rows {4-7, 12-15} of one k-group with the rows
// {0-3, 8-11} of the next, which sits 8 slots of 16 B further in the LDS row (net_kernels.hip, lrow / lchunk); an LDS
// row starts on slot (row mod 16).  The two slot keys of a tile row that holds LDS row R, in the two kinds of group
// (two rows of a tile on one key share their banks: one more LDS cycle for the read):
static inline void azx_tile_slot_keys(int R, int tile_row, int *k1, int *k2) {
    const bool a = (tile_row & 4) == 0;                  // rows {0-3, 8-11}
    *k1 = (R + (a ? 8 : 0)) & 15;
    *k2 = (R + (a ? 0 : 8)) & 15;
}

// The order of 16 chosen rows in their tile.  16 consecutive LDS rows (the `rows` map) have 16 different keys of either
// kind, and only the residue mod 16 enters a key: the first row of every residue rho goes to tile row rho, so a tile
// of 16 different residues is as free of conflicts as `rows`.  A row whose residue the tile already holds goes to the
// free tile row where it meets the fewest rows on its two keys.
static inline void azx_tile_place(const int *chosen, int *out) {
    int n1[16] = {0}, n2[16] = {0}, later[16], nlater = 0;
    bool taken[16] = {false};
    for (int k = 0; k < 16; ++k) {
        const int R = azx_tile_lds_row(chosen[k]), r = R & 15;
        if (taken[r]) { later[nlater++] = chosen[k]; continue; }
        int k1, k2;
        azx_tile_slot_keys(R, r, &k1, &k2);
        ++n1[k1];
        ++n2[k2];
        taken[r] = true;
        out[r] = chosen[k];
    }
    for (int k = 0; k < nlater; ++k) {
        const int R = azx_tile_lds_row(later[k]);
        int best = -1, best_cost = 0, k1, k2;
        for (int r = 0; r < 16; ++r) {
            if (taken[r]) continue;
            azx_tile_slot_keys(R, r, &k1, &k2);
            const int cost = n1[k1] + n2[k2];
            if (best < 0 || cost < best_cost) { best = r; best_cost = cost; }
        }
        azx_tile_slot_keys(R, best, &k1, &k2);
        ++n1[k1];
        ++n2[k2];
        taken[best] = true;
        out[best] = later[k];
    }
}

static inline void azx_tower_tiles_build(int N, int edge, AzxTowerTiles *t) {
    azx_tower_tiles_rows(t);
    if (!edge || N < 2 || N * N > 121) return;
    const int ncells = N * N;
    // class of every LDS row: 0 top, 1 bottom, 2 left, 3 right, 4 interior, 5 dead; its residue in the LDS image
    int cls[256], res[256];
    for (int L = 0; L < 256; ++L) {
        const int cell = L & 127, y = cell / N, x = cell % N;
        cls[L] = cell >= ncells ? 5 : y == 0 ? 0 : y == N - 1 ? 1 : x == 0 ? 2 : x == N - 1 ? 3 : 4;
        res[L] = azx_tile_lds_row(L) & 15;
    }
    bool used[256] = {false};
    int tile[16][16];                                    // [4 wave + slot]
    for (int c = 0; c < 4; ++c) {
        // 16 rows of the class (dead rows once it is exhausted), each time the free row whose residue is the rarest in
        // the tile so far: a full residue system wherever the class and the dead rows reach one
        int nres[16] = {0}, chosen[16];
        for (int k = 0; k < 16; ++k) {
            int best = -1;
            for (int pass = 0; pass < 2 && best < 0; ++pass)
                for (int L = 0; L < 256; ++L)
                    if (!used[L] && cls[L] == (pass ? 5 : c) && (best < 0 || nres[res[L]] < nres[res[best]])) best = L;
            if (best < 0) { azx_tower_tiles_rows(t); return; }     // not even with dead rows: the identity
            used[best] = true;
            ++nres[res[best]];
            chosen[k] = best;
        }
        azx_tile_place(chosen, tile[4 * c + AZX_TOWER_LIGHT_SLOT]);
    }
    // every other row into the other 12 tiles: tile j takes the j-th free row of every residue, ascending (full light
    // tiles leave 12 rows of each residue); where a residue has run out the tile is topped up with the rows left over,
    // again the rarest residue first
    int other[12], members[12][16], count[12], nres[12][16];
    for (int w = 0, j = 0; w < 4; ++w)
        for (int m = 0; m < 4; ++m)
            if (m != AZX_TOWER_LIGHT_SLOT) other[j++] = 4 * w + m;
    for (int j = 0; j < 12; ++j) {
        count[j] = 0;
        for (int rho = 0; rho < 16; ++rho) nres[j][rho] = 0;
        for (int rho = 0; rho < 16; ++rho)
            for (int L = 0; L < 256; ++L)
                if (!used[L] && res[L] == rho) {
                    used[L] = true;
                    nres[j][rho] = 1;
                    members[j][count[j]++] = L;
                    break;
                }
    }
    for (int j = 0; j < 12; ++j) {
        while (count[j] < 16) {
            int best = -1;
            for (int L = 0; L < 256; ++L)
                if (!used[L] && (best < 0 || nres[j][res[L]] < nres[j][res[best]])) best = L;
            used[best] = true;
            ++nres[j][res[best]];
            members[j][count[j]++] = best;
        }
        azx_tile_place(members[j], tile[other[j]]);
    }
    for (int i = 0; i < 256; ++i) t->row[i] = (uint8_t)tile[i >> 4][i & 15];
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
