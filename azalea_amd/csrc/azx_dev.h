// azx_dev.h -- device-side data model shared by the tree and network kernels (gfx950 only).
//
// HBM layout, per game slot g (see DESIGN.md "Data layout"):
//   cells[g][SLOTS*64]  u32 per board cell: bits0-1 colour (0 empty, 1 X, 2 O),
//                       bits2-3 edge flags of the cell's group (low edge / high edge),
//                       bits8..  group label (cell index of the stone that last merged it).
//                       One wavefront owns one game; lane l holds cells l, l+64, l+128.
//   arena[a][g][cap]    Node (16 B): {num_visits, total_value, prior_prob, link}.
//                       link >= 0: first child id (children are contiguous, in ascending
//                       tile order); -1: unevaluated; <= -2: terminal (first_child value
//                       the reference would hold = -2 - link).  The reference's parent[] and
//                       num_children[] (search_tree.py:48-50) are implied: a Hex node with k
//                       legal moves has children with k-1, and paths are recorded on descent.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/azx.h"

#define AZX_LINK_UNEVAL (-1)
#define AZX_LINK_TERM(fc) (-2 - (fc))
#define AZX_LABEL_NONE 0x3FFFFFu

struct alignas(16) Node {
    float nv;      // num_visits   (float32 on purpose: search_tree.py:53)
    float tv;      // total_value  (own perspective, search_tree.py:37-38)
    float pp;      // prior_prob   (parent's perspective, search_tree.py:39-40)
    int32_t link;
};

struct alignas(64) TreeHdr {
    int32_t num_nodes;
    int32_t root_id;
    int32_t root_k;        // legal moves at the root
    int32_t k0;            // legal moves at node 0 (for the six-array dump)
    int32_t arena;         // which ping-pong arena holds the live tree
    int32_t status;        // 0 ok, 1 SearchTreeFull
    int32_t batches_left;  // select batches still to run in the current search
    int32_t pending;       // leaves selected and waiting for expand/backup
    int32_t pending_root;  // the pending leaf is the root evaluation (no backup)
    int32_t select_count;  // select_leaf calls so far in this search (noise row index)
    float   search_value;  // mcts.py:287 accumulator (float32)
    int32_t slow_div;      // a backed-up value was outside the range the unscaled divide is exact for
    int32_t defer_compact; // play mode: compact the arena (keep the subtree under root_id) before the next search
    int32_t dropped;       // nodes discarded by arena compactions since the last reset: num_nodes + dropped is the
                           // reference's never-reclaimed node count (search_tree.py:112 'search_tree_nodes')
    int32_t pad[2];
};

struct alignas(64) GameHdr {
    int32_t color;     // side to move, 1 = X, 2 = O
    int32_t winner;    // 0 / 1 / 2
    int32_t ply;
    int32_t active;    // slot takes part in search/advance
    int64_t uid;       // global game index (seeds the device RNG stream)
    int32_t move_id;   // device-chosen child index of the last azx_play step
    int32_t n_rows;    // replay rows this game has written so far
    int32_t gen;       // games this slot has started so far: uid = slot + n_games * gen (a fixed
                       // seed reproduces every game whatever order the GPU schedules the slots in)
    int32_t ply0;      // ply the game started from (azx_reset with a move prefix; 0 for restarts): its replay
                       // row r was recorded at ply ply0 + r (self-play keeps each row's ply in row_meta: with a
                       // playout cap only the full plies record a row)
    int32_t parked;    // play mode: the game is finished but the harvest queue had no room for its rows; the slot
                       // waits (active = 0) until the host has drained the queue (k_advance in unpark mode)
    int32_t rs_state;  // resignation (azx_set_resign), one word so that a slot starting a game clears it with one store:
                       // AZX_RS_CROSS bits: exempt game, 1 + the first ply at which the resign rule's other conditions
                       // held (0: none yet); AZX_RS_SKIP: the game was in progress when azx_set_resign was called and
                       // counts in no resign statistic; AZX_RS_DONE: the game ended by resignation (a parked slot's
                       // harvest needs it)
    int32_t book;      // self-play opening book (azx_set_selfplay_openings): the index of the opening this game was seated
                       // on, in the book installed now; -1: the game did not come from it (no book, azx_reset with a
                       // move table, a match's game, or a game that was in progress when the book was last set)
    int32_t pad[3];
};
#define AZX_RS_CROSS 0xFFFF
#define AZX_RS_SKIP 0x10000
#define AZX_RS_DONE 0x20000
#define AZX_MOVE_RESIGN (-2)   // GameHdr.move_id: the mover resigns (choose_body to advance_body, play mode 1 only)

enum {   // counters[] slots
    CTR_SELECTS = 0, CTR_SUM_DEPTH, CTR_SUM_K_INT, CTR_SUM_K_LEAF, CTR_EVALS, CTR_TERM_EVALS,
    CTR_GAMES, CTR_ERRORS, CTR_PLIES, CTR_ROWS, CTR_COUNT = 16
};
// playout cap (azx_set_playout_cap; counted only while the cap is on): plies searched in full, plies searched fast,
// games harvested with no recorded row.  (Slots 10-12 belong to the AZX_STAMP_PLAY diagnostic build.)
enum { CTR_CAP_FULL = 13, CTR_CAP_FAST = 14, CTR_CAP_EMPTY = 15 };

struct DevEngine {
    int32_t N, ncells, G, bs, cap, slots;
    int32_t selects_per_search;   // (simulations / bs + 1) * bs, mcts.py:268
    float c_puct;
    int32_t evaluator, flags;
    // games
    uint32_t *cells;        // [G][slots*64]
    GameHdr *ghdr;          // [G]
    // trees
    Node *arena[2];         // [G][cap] each
    TreeHdr *thdr;          // [G]
    // per-leaf scratch of the batch in flight
    int32_t *leaf_node;     // [G][bs]
    int32_t *leaf_len;      // [G][bs] path length (nodes below the root)
    int32_t *leaf_eval;     // [G][bs] index into ev_* or -1 (terminal)
    int32_t *leaf_link;     // [G][bs] the leaf's link when it was selected (-1 or terminal code)
    int32_t *leaf_cells;    // [G][bs] first cell of the path | last cell << 16
    uint64_t *leaf_mask;    // [G][bs][4] empties bitmask at the leaf (original frame)
    int32_t *path;          // [G][bs][ncells]
    // evaluation requests / results (packed by atomic counter)
    uint8_t *ev_board;      // [E][AZX_CELL_STRIDE] network input (first player's view)
    int32_t *ev_src;        // [E] g*bs + i
    int32_t *ev_flip;       // [E] bit 0: the board was flipped (mover is O); bit 1: turned by 180 degrees (AZX_FLAG_RANDOM_REFLECT)
    float *ev_value;        // [E]
    float *ev_prior;        // [E][AZX_CELL_STRIDE] by ORIGINAL cell index
    int32_t *n_eval;        // [1]
    // noise (parity: host rows; throughput: device RNG)
    const double *noise;    // [G][n_select][noise_stride] or null
    int32_t n_select, noise_stride;
    double noise_scale;
    float noise_alpha;
    const float *gamma_tab;    // [AZX_GAMMA_TAB_FLOATS] device gamma sampler table for noise_alpha (mcts_kernels.hip)
    int32_t device_noise;
    uint64_t seed;
    int32_t uid_stride, uid_offset;   // uid = (slot + G * gen) * uid_stride + uid_offset (azx_config.game_index_*)
    int32_t slot_base, pool_games;    // a view of slots [slot_base, slot_base + G) of a pool of pool_games (the pipelined
                                      // schedule's half-pools): the uid above is taken with slot_base + g and pool_games
    const float *prior_by_k;   // [ncells+1]
    int32_t prior_default;     // 1: prior_by_k is the default float32 1/k table
    unsigned long long *counters;   // [G][CTR_COUNT] per-game (no atomics); the host sums over games
    // throughput mode (azx_play): per-slot replay rows of the game in progress ...
    int32_t exploration_depth;
    float temperature;
    uint8_t *row_board;     // [G][ncells][AZX_CELL_STRIDE] absolute colours before the move
    float *row_prob;        // [G][ncells][AZX_CELL_STRIDE] moves_prob dense by child index
    int32_t *row_k;         // [G][ncells]
    float *row_meta;        // [G][ncells][8] per-ply search metrics of the game in progress: search_value, root
                            // width, log-probability of the move drawn, (the row's ply as int bits here; first-row
                            // flag once harvested), mean root-child visits,
                            // tree nodes (search_tree.py:109-112; play_game.py:41-43 averages them per game)
    // ... and the output queue finished games are appended to (whole games only)
    int64_t q_cap;
    int32_t q_ring;         // 1: wrap around instead of stalling (bench)
    uint8_t *q_board;       // [Q][AZX_CELL_STRIDE]
    float *q_prob;          // [Q][AZX_CELL_STRIDE]
    int32_t *q_color, *q_k; // [Q]
    float *q_reward;        // [Q]
    int64_t *q_uid;         // [Q]
    float *q_meta;          // [Q][8] the rows' per-ply search metrics (AZX_ROW_METRICS floats per row)
    unsigned long long *q_count;   // [1] rows appended
    double *stat_sums;      // [G][8] per game: search_value, root_width, action_logprob, reward_last
    // playout cap randomisation (azx_set_playout_cap; NOT the reference's behaviour).  The host hands the configured
    // values to the launches of throughput self-play only and "off" (cap_fast_batches == 0) to every other launch.
    int32_t cap_fast_batches;   // 0: off; else the select batches of a fast search (fast_simulations / bs + 1)
    uint32_t cap_thr_m1;        // the ply is a full search iff azx_cap_word(seed, uid, ply) <= cap_thr_m1 (playout_cap.h)
    // resignation (azx_set_resign; NOT the reference's behaviour), handed to the same launches only: resign_mode is
    // AZX_RESIGN_OFF in every other launch (resign.h)
    int32_t resign_mode;
    int32_t resign_min_ply;
    float resign_thr;           // the mover resigns iff root.total_value / root.num_visits < resign_thr
    uint32_t resign_keep_m1;    // the game is exempt iff azx_resign_word(seed, uid) <= resign_keep_m1 (mode DRAW_EXEMPT)
    unsigned long long *resign_ctr;   // [G][RS_COUNT] per game (no atomics), azx_resign_stats' array; the host sums
    // early stop (azx_set_early_stop; NOT the reference's behaviour), handed to the same launches only and 0 in every
    // other: a ply drawn at temperature 0 ends its search at the first batch boundary at which the most-visited root
    // child leads the second by more than the selects still to come (include/azx.h states the rule)
    int32_t early_stop;
    unsigned long long *estop_ctr;    // [G][ES_COUNT] per game (no atomics), azx_early_stop_stats' array; the host sums
    // training targets of the recorded rows (azx_set_train_targets; NOT the reference's behaviour), handed to the same
    // launches only and "off" (AZX_ROWS_REFERENCE, 0.0f) in every other (include/azx.h has the definition)
    int32_t tt_rows;            // AZX_ROWS_VISITS: the row is counts / sum(counts) at every recorded ply, whatever T
    float tt_mix;               // lambda: the harvest stores (1 - lambda) * z + lambda * v, v = row metric 7
    unsigned long long *tt_ctr;       // [G][TT_COUNT] per game (no atomics), azx_train_targets_stats' array; the host sums
    // forced playouts and policy target pruning (azx_set_forced_playouts; NOT the reference's behaviour), handed to the
    // same launches only and "off" (0.0f, 0) in every other (include/azx.h states the rule)
    float fp_k;                 // > 0: a full search's root select descends into the lowest-index child with
                                // n > 0 and n * n < (k * P) * S, if there is one, instead of the PUCT argmax
    int32_t fp_prune;           // 1: the move draw and the row of a full ply are made from the pruned counts
    unsigned long long *fp_ctr;       // [G][FP_COUNT] per game (no atomics), azx_forced_playouts_stats' array; the host sums
    // Gumbel root search with sequential halving (azx_set_gumbel; NOT the reference's behaviour), handed to the same
    // launches only and "off" (gm_m == 0) in every other (include/azx.h has the definition)
    int32_t gm_m;               // 0: off; else the number of root candidates sampled without replacement
    int32_t gm_rows;            // 1: a recorded row is the policy improved by the completed Q-values
    float gm_c_visit, gm_c_scale;
    uint64_t *gm_state;         // [G][GM_STATE_WORDS] per game: the candidate mask of the slot's last searched ply (bit
                                // c & 63 of word c >> 6, c the child index) and, from GM_SURV on, the survivors'
    float *gm_g;                // [G][2][AZX_CELL_STRIDE] per game, by child index: g_j of the ply being searched (0 on a
                                // greedy ply), written by the launch that begins the ply's search; the top of batch 0
                                // makes it a_j = g_j + ln P_j and puts ln P_j in the second row
    unsigned long long *gm_ctr;       // [G][GM_COUNT] per game (no atomics), azx_gumbel_stats' array; the host sums
    // self-play opening book (azx_set_selfplay_openings; NOT the reference's behaviour).  Unlike the options above it is
    // in every launch: it acts wherever the engine itself starts a game (k_reset without a move table, advance_body's
    // restart, k_book_seat) and nowhere else; bk_n == 0 is "off" (selfplay_openings.h has the draw)
    int32_t bk_n, bk_stride;
    const int16_t *bk_moves;    // [bk_n][bk_stride] tile + 1 in play order, colour 1 at the even plies
    const int32_t *bk_len;      // [bk_n]
    const uint64_t *bk_ub;      // [bk_n] game uid starts from the least o with azx_book_word(seed, uid) < bk_ub[o]
    unsigned long long *bk_ctr; // [bk_n][BK_COUNT] per OPENING (several slots share one: atomics), azx_selfplay_openings_stats' array
    // first-play urgency (azx_set_fpu; NOT the reference's behaviour).  A property of the engine's search, not a self-play
    // option: like the book it is in every launch -- azx_search, the phase API, self-play, matches and tournaments -- and
    // AZX_FPU_OFF (0) is the reference's rule (fpu.h has the rule, include/azx.h the definition)
    int32_t fpu_mode;           // AZX_FPU_OFF / AZX_FPU_ABSOLUTE / AZX_FPU_REDUCTION
    float fpu_value;            // ABSOLUTE: Q of an unvisited child
    float fpu_red, fpu_root_red;   // REDUCTION: r below the root, r at the root
    unsigned long long *fpu_ctr;   // [G][FPU_COUNT] per game (no atomics), azx_fpu_stats' array; the host sums
    // policy temperature of the priors (azx_set_policy_temp; NOT the reference's behaviour).  Like first-play urgency a
    // property of the engine's search, in every launch; (8, 8) is off, the reference's rule (policy_temp.h has the
    // rule, include/azx.h the definition).  These are the values IN FORCE: (8, 8) while the rollout evaluator is set
    int32_t pt_eighths;         // exponent, in eighths, of the prior rows an expansion stores
    int32_t pt_root_eighths;    // exponent, in eighths, of the priors the root select scores with
    unsigned long long *pt_ctr; // [G][PT_COUNT] per game (no atomics), azx_policy_temp_stats' array; the host sums
};
// expansions tempered, rows left as delivered by the guard (expansion or root), searches begun with root_eighths != 8
enum { PT_TEMPERED = 0, PT_GUARDED, PT_ROOT_SEARCHES, PT_RESERVED, PT_COUNT = 4 };
// selects made under the option, node levels scored under it with an unvisited child, selects that ended on an unvisited child
enum { FPU_SELECTS = 0, FPU_LEVELS, FPU_UNVISITED, FPU_RESERVED, FPU_COUNT = 4 };
// games started, games finished, finished games won by colour 1, plies of finished games counted from the empty board
enum { BK_STARTED = 0, BK_FINISHED, BK_WON1, BK_PLIES, BK_COUNT = 4 };
// plies chosen under the option, halvings performed, root selects made under the option, rows recorded as the improved policy
enum { GM_PLIES = 0, GM_HALVINGS, GM_SELECTS, GM_ROWS, GM_COUNT = 4 };
enum { GM_CAND = 0, GM_SURV = 4, GM_STATE_WORDS = 8 };
// full plies chosen under the option, selects whose forced set was non-empty, recorded rows with a reduced child,
// visits removed from recorded rows
enum { FP_PLIES = 0, FP_FORCED, FP_ROWS_PRUNED, FP_REMOVED, FP_COUNT = 4 };
// rows recorded while the option is on; of those, rows of greedy plies; of those, rows with more than one visited child
enum { TT_ROWS = 0, TT_GREEDY, TT_GREEDY_WIDE, TT_COUNT = 4 };
// T = 0 plies searched under the option, plies stopped before their last batch, batches skipped (batches_left at the stops)
enum { ES_T0_PLIES = 0, ES_STOPPED, ES_SKIPPED, ES_COUNT = 4 };
enum { RS_RESIGNED = 0, RS_PLAYED_OUT, RS_EXEMPT, RS_EXEMPT_CROSSED, RS_FALSE_POS, RS_SUM_RESIGN_PLY, RS_SUM_SAVED, RS_COUNT = 8 };

// ---- wave64 reductions on DPP (no LDS crossbar round trips) ---------------------------------
// row_shr 1/2/4/8 build an inclusive scan inside each 16-lane row, row_bcast15 / row_bcast31
// fold the rows; the total lands in lane 63 and is broadcast with v_readlane.
#define AZX_DPP(old, v, ctrl, rmask) \
    __builtin_amdgcn_update_dpp((old), (v), (ctrl), (rmask), 0xf, false)

__device__ __forceinline__ float wave_sum(float v) {
    v += __int_as_float(AZX_DPP(0, __float_as_int(v), 0x111, 0xf));
    v += __int_as_float(AZX_DPP(0, __float_as_int(v), 0x112, 0xf));
    v += __int_as_float(AZX_DPP(0, __float_as_int(v), 0x114, 0xf));
    v += __int_as_float(AZX_DPP(0, __float_as_int(v), 0x118, 0xf));
    v += __int_as_float(AZX_DPP(0, __float_as_int(v), 0x142, 0xa));
    v += __int_as_float(AZX_DPP(0, __float_as_int(v), 0x143, 0xc));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ int wave_sum_i(int v) {
    v += AZX_DPP(0, v, 0x111, 0xf);
    v += AZX_DPP(0, v, 0x112, 0xf);
    v += AZX_DPP(0, v, 0x114, 0xf);
    v += AZX_DPP(0, v, 0x118, 0xf);
    v += AZX_DPP(0, v, 0x142, 0xa);
    v += AZX_DPP(0, v, 0x143, 0xc);
    return __builtin_amdgcn_readlane(v, 63);
}
// the same sum over unsigned words (wraps modulo 2^32 by definition: the policy temperature's Z may pass 2^31)
__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
    v += (uint32_t)AZX_DPP(0, (int)v, 0x111, 0xf);
    v += (uint32_t)AZX_DPP(0, (int)v, 0x112, 0xf);
    v += (uint32_t)AZX_DPP(0, (int)v, 0x114, 0xf);
    v += (uint32_t)AZX_DPP(0, (int)v, 0x118, 0xf);
    v += (uint32_t)AZX_DPP(0, (int)v, 0x142, 0xa);
    v += (uint32_t)AZX_DPP(0, (int)v, 0x143, 0xc);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// unsigned max: 0 is the identity, so bound_ctrl DPP reads need no 'old' operand
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#define AZX_DPPZ(v, ctrl, rmask) (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), (rmask), 0xf, true)
    uint32_t t;
    t = AZX_DPPZ(v, 0x111, 0xf); v = t > v ? t : v;
    t = AZX_DPPZ(v, 0x112, 0xf); v = t > v ? t : v;
    t = AZX_DPPZ(v, 0x114, 0xf); v = t > v ? t : v;
    t = AZX_DPPZ(v, 0x118, 0xf); v = t > v ? t : v;
    t = AZX_DPPZ(v, 0x142, 0xa); v = t > v ? t : v;
    t = AZX_DPPZ(v, 0x143, 0xc); v = t > v ? t : v;
#undef AZX_DPPZ
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ float wave_max(float v) {
    const int ninf = 0xff800000;   // -inf: identity of max
    v = fmaxf(v, __int_as_float(AZX_DPP(ninf, __float_as_int(v), 0x111, 0xf)));
    v = fmaxf(v, __int_as_float(AZX_DPP(ninf, __float_as_int(v), 0x112, 0xf)));
    v = fmaxf(v, __int_as_float(AZX_DPP(ninf, __float_as_int(v), 0x114, 0xf)));
    v = fmaxf(v, __int_as_float(AZX_DPP(ninf, __float_as_int(v), 0x118, 0xf)));
    v = fmaxf(v, __int_as_float(AZX_DPP(ninf, __float_as_int(v), 0x142, 0xa)));
    v = fmaxf(v, __int_as_float(AZX_DPP(ninf, __float_as_int(v), 0x143, 0xc)));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// ---- Hex rules on one wavefront: azalea/game/hex.py:137-231 ------------------------------
// The reference flood-fills the last mover's group (hex.py:204-231); here every cell carries
// its group's label and edge flags, so placing a stone is one O(1) wave-parallel relabel
// (a union of <= 6 neighbouring groups) and the win test is "merged flags == both edges".
// Board geometry in constant memory (scalar loads): for every board size N = 2..13 and every cell
// four u64: the neighbour bitmask (hex.py:190-195 neighbourhood) over cell slots 0..2, and the
// cell's own edge bits (bit0/1: row 0 / row N-1 for colour 1, bit2/3: column 0 / N-1 for colour 2).
#define AZX_GEO_CELLS 820            // sum of N^2 for N = 2..13 is 818
extern __constant__ uint64_t c_geo[AZX_GEO_CELLS * 4];
// float32 sqrt of the integers 0..AZX_SQRT_TAB-1 (correctly rounded, filled by the host): the
// sum of child visit counts under the square root of mcts.py:132 is always a small integer
#define AZX_SQRT_TAB 4096
extern __constant__ float c_sqrt[AZX_SQRT_TAB];
__host__ __device__ inline int azx_geo_base(int N) {   // cells of all smaller boards
    int b = 0;
    for (int n = 2; n < N; ++n) b += n * n;
    return b;
}

template <int SLOTS>
struct HexWave {
    uint32_t c[SLOTS];        // per-lane cells: colour | group flags << 2 | group label << 8
    uint64_t occ[2][SLOTS];   // wave-uniform bitboards of the X / O stones
    int color;                // 1 = X to move, 2 = O (hex.py:148)
    int winner;               // hex.py:149
    int gbase;                // this board size's offset into c_geo

    __device__ __forceinline__ void geom(int N, int lane) { (void)lane; gbase = azx_geo_base(N); }
    __device__ __forceinline__ void load(const uint32_t *p, int lane) {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            c[s] = p[s * 64 + lane];
            occ[0][s] = __ballot((c[s] & 3u) == 1u);
            occ[1][s] = __ballot((c[s] & 3u) == 2u);
        }
    }
    __device__ __forceinline__ void store(uint32_t *p, int lane) const {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) p[s * 64 + lane] = c[s];
    }
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) { c[s] = 0; occ[0][s] = 0ull; occ[1][s] = 0ull; }
        color = 1;
        winner = 0;
    }
    // empties bitmask, slot s (hex.py:151-159: legal moves are the empty cells while winner==0):
    // pure scalar arithmetic on the stone bitboards
    __device__ __forceinline__ uint64_t empties(int s, int lane, int ncells) const {
        (void)lane;
        const int nv = ncells - 64 * s;
        const uint64_t valid = nv >= 64 ? ~0ull : (nv <= 0 ? 0ull : ((1ull << nv) - 1ull));
        return ~(occ[0][s] | occ[1][s]) & valid;
    }
    // hex.py:172-179 step + :204-231 check_win.  `cell` must be wave-uniform, empty, winner==0.
    // The same-colour neighbours are the AND of the cell's neighbour mask (constant memory) with
    // the mover's bitboard -- scalar work; their groups' edge flags are OR-ed and their groups
    // relabelled with one vector compare per neighbouring stone.
    __device__ __forceinline__ void step(int cell, int N, int lane) {
        (void)N;
        const int col = color;
        const uint64_t *g = c_geo + (size_t)(gbase + cell) * 4;
        uint32_t flags = (uint32_t)(g[3] >> (2 * (col - 1))) & 3u;
        uint64_t nb[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            nb[s] = g[s] & (col == 1 ? occ[0][s] : occ[1][s]);
            uint64_t m = nb[s];
            while (m) {
                const int j = (int)__ffsll((long long)m) - 1;
                m &= m - 1;
                flags |= ((uint32_t)__builtin_amdgcn_readlane((int)c[s], j) >> 2) & 3u;
            }
        }
        const uint32_t nv = (uint32_t)col | (flags << 2) | ((uint32_t)cell << 8);
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            uint64_t m = nb[s];
            while (m) {
                const int j = (int)__ffsll((long long)m) - 1;
                m &= m - 1;
                const uint32_t lab = (uint32_t)__builtin_amdgcn_readlane((int)c[s], j) >> 8;
#pragma unroll
                for (int t = 0; t < SLOTS; ++t)
                    if ((int)(c[t] & 3u) == col && (c[t] >> 8) == lab) c[t] = nv;
            }
        }
        const uint64_t bit = 1ull << (cell & 63);
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            if (s * 64 + lane == cell) c[s] = nv;
            if (s == (cell >> 6)) {
                if (col == 1) occ[0][s] |= bit; else occ[1][s] |= bit;
            }
        }
        winner = (flags == 3u) ? col : 0;
        color = 3 - col;
    }
};

