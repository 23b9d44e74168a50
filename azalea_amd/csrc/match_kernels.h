// match_kernels.h -- device-resident matches between two engines (azx_match_*): the match's own device state and
// the launchers of its bookkeeping kernels (match_kernels.hip, compiled as part of mcts_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "azx_dev.h"

enum {   // MatchDev::ctr slots
    MCTR_NEXT = 0,      // game indices handed out so far, relative to first_game (the refill claims the next one)
    MCTR_DECIDED,       // games settled (won or voided): the one word the host reads back per ply
    MCTR_WINS0, MCTR_WINS1, MCTR_FIRST_WINS, MCTR_VOIDED, MCTR_PLIES,
    MCTR_ROWS_LOST,     // harvest: replay rows of won games that could NOT be queued (queue too small, or the two
                        // engines' row counts do not add up to the game's length): the host turns > 0 into AZX_ESTATE
    MCTR_COUNT = 8
};

// An opening book (azx_match_set_openings / azx_tournament_set_openings): game u starts from the position after
// the `len[o]` moves moves[o * stride + 0 ..] (tile + 1 in play order, colour 1 at the even plies) of opening
// o = (u >> 1) % n under the alternating first mover, u % n under a fixed one.  n == 0: no book, every game starts
// from the empty board.  The host has checked every opening (azx_openings_check): moves in range, no tile twice,
// undecided after every move.
struct MatchBook {
    const int16_t *moves;          // [n][stride]
    const int32_t *len;            // [n]
    int32_t n, stride;
};

struct MatchDev {
    int64_t *slot_game;            // [G] game index u the slot is playing, -1 = idle
    int64_t first_game, n_games;   // the call plays games first_game .. first_game + n_games - 1
    unsigned long long *ctr;       // [MCTR_COUNT]
    int8_t *outcome;               // [n_games] +1 agent 0 won, -1 agent 1 won, 0 voided
    int16_t *length;               // [n_games] plies played
    int16_t *moves;                // [n_games][ncells] tile + 1 in play order, 0-padded; null = not recorded
    int32_t harvest;               // 1: every won game's replay rows are appended to the harvest queue (q_*, q_count) of
                                   // engine A when the game settles (match_harvest); 0 = off
    int32_t first_mode;            // -1: agent u & 1 moves first in game u; 0 / 1: that agent moves first in every game
    MatchBook book;                // the games' opening positions (n == 0: the empty board)
};

// slot g takes game first_game + g (idle beyond n_games); both engines' slots get uid = game index
void azx_launch_match_init(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st);
// with a book only, after azx_launch_match_init: every slot's first game is set up from its opening, exactly as
// the refill of azx_launch_match_step sets up a later one
void azx_launch_match_open(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st);
// whose turn: GameHdr.active in both engines (mover's 1, the other 0; idle slots 0 in both)
void azx_launch_match_turn(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st);
// hand the mover's drawn move over, step both engines' slots, settle finished / voided games and refill
void azx_launch_match_step(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st);

// ---- tournaments (azx_tournament_*): P matches side by side in one ply loop, sharing K engines ----------------
// A table plays one game of its pair at a time: slot sa of engine ea and slot sb of engine eb hold the two agents'
// trees (ea is the pair's first engine, "agent 0").  The layout is static and computed on the host: an engine's
// pool is partitioned among its opponents, so a table's two slots generally have different indices.
struct TourTable {
    int32_t ea, sa, eb, sb;        // engine index and slot of agent 0 / agent 1
    int32_t pair, local;           // the pair the table plays for, and its index among that pair's tables
};

struct TourDev {
    const DevEngine *eng;          // [n_engines] the engines' device structs, in device memory
    const TourTable *tab;          // [n_tables], pair-major
    int64_t *tab_game;             // [n_tables] game index u the table is playing, -1 = idle
    int32_t n_engines, n_pairs, n_tables, max_g;   // max_g: the largest n_games of the engines
    int64_t first_game, rounds;    // round r of pair s is game first_game + s * rounds + r
    unsigned long long *ctr;       // [n_pairs + 1][MCTR_COUNT]: per pair, then the totals row (MCTR_DECIDED over all
                                   // pairs: the one word the host reads back per ply)
    int8_t *outcome;               // [n_pairs * rounds] by u - first_game, as MatchDev's
    int16_t *length;               // [n_pairs * rounds]
    int16_t *moves;                // [n_pairs * rounds][ncells]; null = not recorded
    int32_t sink;                  // harvest target: -1 = off, else the index in eng[] of the engine whose harvest queue
                                   // takes the won games' replay rows of ALL pairs (as MatchDev::harvest)
    int32_t first_mode;            // as MatchDev::first_mode
    MatchBook book;                // as MatchDev::book
};

// every table takes its pair's round `local` (idle beyond `rounds`) and both its slots that game's uid; every slot
// of every engine gets active = 0, so the slots no table owns are never searched
void azx_launch_tour_init(const TourDev &T, hipStream_t st);
// azx_launch_match_open for every table (with a book only, after azx_launch_tour_init)
void azx_launch_tour_open(const TourDev &T, int slots, hipStream_t st);
// whose turn: GameHdr.active of each table's two slots (mover's 1, the other 0; idle tables 0 in both)
void azx_launch_tour_turn(const TourDev &T, hipStream_t st);
// k_match_step for a table: hand-over, game step in both slots, settle into the pair's tallies, refill from the
// pair's own round counter.  `slots` is the engines' common cell-slot count (DevEngine::slots)
void azx_launch_tour_step(const TourDev &T, int slots, hipStream_t st);
