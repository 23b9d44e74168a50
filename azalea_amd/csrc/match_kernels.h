// match_kernels.h -- device-resident matches between two engines (azx_match_*): the match's own device state and
// the launchers of its bookkeeping kernels (match_kernels.hip, compiled as part of mcts_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "azx_dev.h"

enum {   // MatchDev::ctr slots
    MCTR_NEXT = 0,      // game indices handed out so far, relative to first_game (the refill claims the next one)
    MCTR_DECIDED,       // games settled (won or voided): the one word the host reads back per ply
    MCTR_WINS0, MCTR_WINS1, MCTR_FIRST_WINS, MCTR_VOIDED, MCTR_PLIES, MCTR_COUNT = 8
};

struct MatchDev {
    int64_t *slot_game;            // [G] game index u the slot is playing, -1 = idle
    int64_t first_game, n_games;   // the call plays games first_game .. first_game + n_games - 1
    unsigned long long *ctr;       // [MCTR_COUNT]
    int8_t *outcome;               // [n_games] +1 agent 0 won, -1 agent 1 won, 0 voided
    int16_t *length;               // [n_games] plies played
    int16_t *moves;                // [n_games][ncells] tile + 1 in play order, 0-padded; null = not recorded
};

// slot g takes game first_game + g (idle beyond n_games); both engines' slots get uid = game index
void azx_launch_match_init(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st);
// whose turn: GameHdr.active in both engines (mover's 1, the other 0; idle slots 0 in both)
void azx_launch_match_turn(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st);
// hand the mover's drawn move over, step both engines' slots, settle finished / voided games and refill
void azx_launch_match_step(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st);
