// match_kernels.hip -- bookkeeping kernels of a device-resident match between two engines (azx_match_play).
//
// NOT a translation unit of its own: mcts_kernels.hip includes this file at its end.  The game step and subtree
// carry are advance_body's, and the rules read the board geometry from that unit's constant memory (c_geo), which
// a second unit could not share without relocatable device code.
//
// The reference plays an evaluation game with one search tree per agent: the mover's agent searches and draws,
// then EVERY agent follows the move in its own tree (azalea/play_game.py:27-52, policy.py:170-176,
// search_tree.py:115-132).  Here slot g of engine A and slot g of engine B hold the two agents' views of the same
// game; these kernels decide whose turn it is, hand the drawn move over, settle finished games and refill the
// slot, so that the host reads back one word per ply.  Plain stores and atomics only.
// A tournament (azx_tournament_play, second half of this file) is P such matches side by side in one ply loop: the
// same bookkeeping per table, a table's two slots being any slot of any two of K engines.
#include "match_kernels.h"

// agent (0 = engine A, 1 = engine B) that moves first in game u: agent u & 1, or the one first_mode 0 / 1 fixes for
// every game (the reference's play_game always starts with agents[0], play_game.py:47)
__device__ __forceinline__ int match_first(int64_t u, int mode) { return mode < 0 ? (int)(u & 1) : mode; }
// agent to move in game u at `ply`
__device__ __forceinline__ int match_mover(int64_t u, int ply, int mode) { return match_first(u, mode) ^ (ply & 1); }
// opening of game u (MatchBook::n > 0): games 2j and 2j + 1 of the alternating first mover share one, so that every
// opening is played with the colours both ways round; keyed on the game index alone, like the draws
__device__ __forceinline__ int match_opening(int64_t u, int n, int mode) { return (int)((mode < 0 ? u >> 1 : u) % n); }

__global__ void k_match_init(DevEngine A, DevEngine B, MatchDev M) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.G) return;
    const int64_t u = g < M.n_games ? M.first_game + g : -1;
    M.slot_game[g] = u;
    if (u >= 0) {        // every draw of game u is keyed by (engine seed + u, ply): not by the slot
        A.ghdr[g].uid = u;
        B.ghdr[g].uid = u;
    }
}

__global__ void k_match_turn(DevEngine A, DevEngine B, MatchDev M) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= A.G) return;
    const int64_t u = M.slot_game[g];
    int a = 0, b = 0;
    if (u >= 0) {
        const int mover = match_mover(u, A.ghdr[g].ply, M.first_mode);
        a = mover == 0;
        b = mover == 1;
    }
    A.ghdr[g].active = a;
    B.ghdr[g].active = b;
}

// fresh game in slot g of one engine (what advance_body's play-mode restart does, with the uid given): the empty
// board, or with a book the position after game uid's opening, in the state k_reset leaves for that move prefix
// (stones, colour, ply = ply0 = the opening's length, a one-node tree over the position's legal moves in arena 0)
template <int SLOTS>
__device__ __forceinline__ void match_restart(const DevEngine &E, int g, int64_t uid, const MatchBook &bk, int mode,
                                              int lane) {
    HexWave<SLOTS> z;
    z.clear();
    int ply = 0, k = E.ncells;
    const bool opened = bk.n > 0 && uid >= 0;
    if (opened) {
        const int o = match_opening(uid, bk.n, mode);
        const int16_t *mv = bk.moves + (size_t)o * bk.stride;
        ply = __builtin_amdgcn_readfirstlane(bk.len[o]);
        z.geom(E.N, lane);
        for (int p = 0; p < ply; ++p) z.step(__builtin_amdgcn_readfirstlane(mv[p] - 1), E.N, lane);   // (wave-uniform)
        k = make_masks<SLOTS>(z, lane, E.ncells).k;
    }
    z.store(E.cells + (size_t)g * SLOTS * 64, lane);
    GameHdr *gh = E.ghdr + g;
    if (lane == 0) {
        gh->color = z.color;
        gh->winner = z.winner;
        gh->ply = ply;
        gh->active = 0;            // k_match_turn decides
        gh->move_id = -1;
        gh->n_rows = 0;
        gh->ply0 = ply;
        gh->parked = 0;
        gh->rs_state = 0;
        gh->book = -1;             // (a match's book is the match's own: azx_match_set_openings)
        if (uid >= 0) gh->uid = uid;
        if (opened) E.thdr[g].arena = 0;
    }
    __builtin_amdgcn_s_waitcnt(0);
    tree_reset<SLOTS>(E, g, E.thdr + g, k, lane);
}

// game u's record begins with its opening (MatchBook::n > 0; `rec` is the game's row of the moves buffer)
__device__ __forceinline__ void match_record_opening(int16_t *rec, int64_t u, const MatchBook &bk, int mode, int lane) {
    const int o = match_opening(u, bk.n, mode);
    const int16_t *mv = bk.moves + (size_t)o * bk.stride;
    const int len = bk.len[o];
    for (int p = lane; p < len; p += 64) rec[p] = mv[p];
}

// with a book, after k_match_init: one wave per slot sets up the slot's first game, as the refill does later ones
template <int SLOTS>
__global__ __launch_bounds__(64) void k_match_open(DevEngine A, DevEngine B, MatchDev M) {
    const int lane = threadIdx.x;
    const int g = blockIdx.x;
    const int64_t u = M.slot_game[g];
    if (u < 0) return;
    match_restart<SLOTS>(A, g, u, M.book, M.first_mode, lane);
    match_restart<SLOTS>(B, g, u, M.book, M.first_mode, lane);
    if (M.moves) match_record_opening(M.moves + (size_t)(u - M.first_game) * A.ncells, u, M.book, M.first_mode, lane);
}

// ---- settle-time harvest: a won game's replay rows into a harvest queue (play_game.py:59-67 for two agents) ----
// Each engine's move draw (choose_body) has written the rows of the plies IT moved at into its own slot's row area, at
// row index GameHdr.n_rows: the first mover holds plies 0, 2, 4, ... at rows 0, 1, 2, ..., the other agent plies 1, 3,
// 5, ....  Row p of the game is therefore row p >> 1 of the engine that moved at ply p (a game from an opening of
// ply0 moves: row (p - ply0) >> 1, the agent that moved at ply0 holding the even offsets).  `src` rows of PIECES 16-byte
// pieces each go to every second row of `dst` (which points at the game's first or second queue row), eight pieces
// in flight per lane.
template <int PIECES>
__device__ __forceinline__ void match_copy_rows(uint4 *dst, const uint4 *src, int n_rows, int lane) {
    // eight named registers, not an array: an indexed array of sixteen stayed in scratch memory in these kernels
    const int n16 = n_rows * PIECES;
#define MATCH_LD(k) const uint4 v##k = src[min(i0 + k * 64 + lane, n16 - 1)];     /* (the tail repeats the last piece) */
#define MATCH_ST(k)                                                       \
    {                                                                     \
        const int i = i0 + k * 64 + lane;                                 \
        if (i < n16) {                                                    \
            const int r = i / PIECES;                                     \
            dst[(size_t)(2 * r) * PIECES + (i - r * PIECES)] = v##k;      \
        }                                                                 \
    }
    for (int i0 = 0; i0 < n16; i0 += 64 * 8) {
        MATCH_LD(0) MATCH_LD(1) MATCH_LD(2) MATCH_LD(3) MATCH_LD(4) MATCH_LD(5) MATCH_LD(6) MATCH_LD(7)
        MATCH_ST(0) MATCH_ST(1) MATCH_ST(2) MATCH_ST(3) MATCH_ST(4) MATCH_ST(5) MATCH_ST(6) MATCH_ST(7)
    }
#undef MATCH_LD
#undef MATCH_ST
}

// the harvest queue of an engine, by value (a reference picked among kernel arguments would put them in scratch)
struct MatchSink {
    uint8_t *q_board;
    float *q_prob;
    int32_t *q_color, *q_k;
    float *q_reward;
    int64_t *q_uid;
    float *q_meta;
    unsigned long long *q_count;
    int64_t q_cap;
};
__device__ __forceinline__ MatchSink match_sink(const DevEngine &E) {
    return MatchSink{E.q_board, E.q_prob, E.q_color, E.q_k, E.q_reward, E.q_uid, E.q_meta, E.q_count, E.q_cap};
}

// the `n` rows of slot `slot` of engine E are the game's plies ply0 + off, ply0 + off + 2, ... (ply0: the ply the
// game's first search ran at, its opening's length): queue rows pos + off, pos + off + 2, ...
__device__ __forceinline__ void match_harvest_rows(const DevEngine &E, int slot, int n, int off, int ply0,
                                                   const MatchSink &Q, unsigned long long pos, int64_t u, int winner,
                                                   int lane) {
    const size_t sr = (size_t)slot * E.ncells;                     // the slot's first row
    const size_t q0 = (size_t)pos + off;
    match_copy_rows<AZX_CELL_STRIDE / 16>(reinterpret_cast<uint4 *>(Q.q_board + q0 * AZX_CELL_STRIDE),
                                          reinterpret_cast<const uint4 *>(E.row_board + sr * AZX_CELL_STRIDE), n, lane);
    match_copy_rows<AZX_CELL_STRIDE / 4>(reinterpret_cast<uint4 *>(Q.q_prob + q0 * AZX_CELL_STRIDE),
                                         reinterpret_cast<const uint4 *>(E.row_prob + sr * AZX_CELL_STRIDE), n, lane);
    for (int r = lane; r < n; r += 64) {
        const int p = ply0 + 2 * r + off;                          // the ply from the empty board: colour and reward sign
        const size_t q = (size_t)pos + 2 * r + off;
        Q.q_color[q] = p & 1;
        Q.q_k[q] = E.row_k[sr + r];
        float rew = winner == 1 ? 1.0f : -1.0f;                    // play_game.py:64-65
        if (p & 1) rew = -rew;
        Q.q_reward[q] = rew;
        Q.q_uid[q] = u;
        const float4 *ms = reinterpret_cast<const float4 *>(E.row_meta) + (sr + r) * 2;
        float4 mt = ms[0];
        mt.w = p == ply0 ? 1.0f : 0.0f;                            // marks the first row of a game
        reinterpret_cast<float4 *>(Q.q_meta)[q * 2] = mt;
        reinterpret_cast<float4 *>(Q.q_meta)[q * 2 + 1] = ms[1];
    }
}

// One wave.  Slots sa of A and sb of B hold the finished game u (`len` plies of which the first `ply0` were its
// opening, colour `winner` won, agent `first` owns the even plies); Q is the engine whose queue takes the rows.  The
// agent that moved at ply0 holds plies ply0, ply0 + 2, ... at its rows 0, 1, ..., the other one ply0 + 1, ....  The
// game's rows are reserved with one atomicAdd and stay contiguous, plies ascending.  The queue is no ring here and the host sizes it for the worst case; should the rows
// not fit after all, or the two engines' row counts not add up to the game, the reservation is given back, nothing
// is written and `lost` counts the rows (the host reports that as an internal error).
__device__ __forceinline__ void match_harvest(const DevEngine &A, int sa, const DevEngine &B, int sb, const MatchSink &Q,
                                              unsigned long long *lost, int64_t u, int first, int winner, int len,
                                              int ply0, int lane) {
    const int nA = A.ghdr[sa].n_rows, nB = B.ghdr[sb].n_rows;
    const int opener = first ^ (ply0 & 1);                               // the agent that moved at ply0
    len -= ply0;                                                         // the rows of the game: one per searched ply
    bool ok = nA + nB == len && (opener ? nB : nA) == (len + 1) >> 1;
    unsigned long long pos = 0;
    if (ok) {
        if (lane == 0) pos = atomicAdd(Q.q_count, (unsigned long long)len);
        pos = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(pos >> 32)) << 32) |
              (unsigned int)__builtin_amdgcn_readfirstlane((int)pos);
        if (pos + (unsigned long long)len > (unsigned long long)Q.q_cap) {
            if (lane == 0) atomicAdd(Q.q_count, (unsigned long long)(-(long long)len));
            ok = false;
        }
    }
    if (!ok) {
        if (lane == 0) atomicAdd(lost, (unsigned long long)len);
        return;
    }
    match_harvest_rows(A, sa, nA, opener, ply0, Q, pos, u, winner, lane);      // agent 0 holds the even rows iff it opened
    match_harvest_rows(B, sb, nB, 1 - opener, ply0, Q, pos, u, winner, lane);
}

// One wave per slot, after both engines' searches and move draws of this ply.
template <int SLOTS>
__global__ __launch_bounds__(64) void k_match_step(DevEngine A, DevEngine B, MatchDev M) {
    const int lane = threadIdx.x;
    const int g = blockIdx.x;
    const int64_t u = M.slot_game[g];
    if (u < 0) return;                                         // idle slot
    GameHdr *ga = A.ghdr + g, *gb = B.ghdr + g;
    const int ply = ga->ply, ply0 = ga->ply0;                  // (the two slots hold the same game)
    const int first = match_first(u, M.first_mode);
    const int mover = first ^ (ply & 1);
    const int mid = mover ? gb->move_id : ga->move_id;
    const int status = mover ? B.thdr[g].status : A.thdr[g].status;
    // SearchTreeFull in the searching agent's tree voids the game (parallel_player.py:73-76 skips such a game);
    // a search that ended without a draw cannot happen on a live game and is treated alike, so no slot can spin
    bool voided = status != 0 || mid < 0;
    const int64_t idx = u - M.first_game;
    int winner = 0, len = ply;

    if (!voided) {
        // the mid-th legal move in ascending tile order (search_tree.py:306): the same tile in both engines
        HexWave<SLOTS> h;
        h.load(A.cells + (size_t)g * SLOTS * 64, lane);
        h.color = ga->color;
        h.winner = ga->winner;
        const Masks<SLOTS> mk = make_masks<SLOTS>(h, lane, A.ncells);
        int cell = -1;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const uint64_t hit = __ballot(lane_bit(mk.m[s]) && mk.base[s] + rank_below(mk.m[s]) == mid);
            if (hit) cell = s * 64 + (int)__ffsll((long long)hit) - 1;
        }
        if (cell < 0 || ply >= A.ncells) {
            voided = true;
        } else {
            if (lane == 0) {
                if (M.moves) M.moves[(size_t)idx * A.ncells + ply] = (int16_t)(cell + 1);
                ga->move_id = mid;  gb->move_id = mid;         // Policy.execute_action for every agent
                ga->active = 1;     gb->active = 1;
            }
            wave_mem_sync();
            advance_body<SLOTS>(A, g, nullptr, 0);
            advance_body<SLOTS>(B, g, nullptr, 0);
            wave_mem_sync();
            winner = ga->winner;
            len = ply + 1;
        }
    }
    if (!voided && winner == 0) return;                        // the game goes on

    if (M.harvest && !voided)
        match_harvest(A, g, B, g, match_sink(A), M.ctr + MCTR_ROWS_LOST, u, first, winner, len, ply0, lane);

    // ---- settle: outcome by agent, tallies, the next game for this slot ----
    long long next_u = -1;
    if (lane == 0) {
        int outcome = 0;
        if (!voided) {
            const int won = winner == 1 ? first : 1 - first;   // colour 1 = the first mover
            outcome = won == 0 ? 1 : -1;
            atomicAdd(M.ctr + (won == 0 ? MCTR_WINS0 : MCTR_WINS1), 1ull);
            if (winner == 1) atomicAdd(M.ctr + MCTR_FIRST_WINS, 1ull);
        } else {
            atomicAdd(M.ctr + MCTR_VOIDED, 1ull);
        }
        M.outcome[idx] = (int8_t)outcome;
        M.length[idx] = (int16_t)len;
        atomicAdd(M.ctr + MCTR_PLIES, (unsigned long long)(len - ply0));     // the moves searched and played
        atomicAdd(M.ctr + MCTR_DECIDED, 1ull);
        // the lowest game index not yet started, or idle
        const unsigned long long nx = atomicAdd(M.ctr + MCTR_NEXT, 1ull);
        next_u = nx < (unsigned long long)M.n_games ? M.first_game + (long long)nx : -1;
        M.slot_game[g] = next_u;
    }
    next_u = ((long long)__builtin_amdgcn_readfirstlane((int)(next_u >> 32)) << 32) |
             (unsigned int)__builtin_amdgcn_readfirstlane((int)next_u);
    match_restart<SLOTS>(A, g, next_u, M.book, M.first_mode, lane);
    match_restart<SLOTS>(B, g, next_u, M.book, M.first_mode, lane);
    if (M.book.n > 0 && next_u >= 0 && M.moves)
        match_record_opening(M.moves + (size_t)(next_u - M.first_game) * A.ncells, next_u, M.book, M.first_mode, lane);
}

void azx_launch_match_init(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st) {
    hipLaunchKernelGGL(k_match_init, dim3((A.G + 255) / 256), dim3(256), 0, st, A, B, M);
}

void azx_launch_match_open(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st) {
#define CALL(S) hipLaunchKernelGGL((k_match_open<S>), dim3(A.G), dim3(64), 0, st, A, B, M)
    DISPATCH_SLOTS(A.slots, CALL);
#undef CALL
}

void azx_launch_match_turn(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st) {
    hipLaunchKernelGGL(k_match_turn, dim3((A.G + 255) / 256), dim3(256), 0, st, A, B, M);
}

void azx_launch_match_step(const DevEngine &A, const DevEngine &B, const MatchDev &M, hipStream_t st) {
#define CALL(S) hipLaunchKernelGGL((k_match_step<S>), dim3(A.G), dim3(64), 0, st, A, B, M)
    DISPATCH_SLOTS(A.slots, CALL);
#undef CALL
}

// ============================================================================================
// tournaments (azx_tournament_play): the same bookkeeping per TABLE.  The K engines' structs are read from a device
// array (a kernel argument indexed by a table's engine number would live in scratch), and a table's two slots are
// its descriptor's, not the block index.
// ============================================================================================
__global__ void k_tour_init(TourDev T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    // no slot is searched unless k_tour_turn says so (k_reset left every slot active)
    const int e = t / T.max_g, g = t - e * T.max_g;
    if (e < T.n_engines && g < T.eng[e].G) T.eng[e].ghdr[g].active = 0;
    if (t >= T.n_tables) return;
    const TourTable tb = T.tab[t];
    const int64_t u = tb.local < T.rounds ? T.first_game + (int64_t)tb.pair * T.rounds + tb.local : -1;
    T.tab_game[t] = u;
    if (u >= 0) {
        T.eng[tb.ea].ghdr[tb.sa].uid = u;
        T.eng[tb.eb].ghdr[tb.sb].uid = u;
    }
}

// k_match_open for a table
template <int SLOTS>
__global__ __launch_bounds__(64) void k_tour_open(TourDev T) {
    const int lane = threadIdx.x;
    const int t = blockIdx.x;
    const int64_t u = T.tab_game[t];
    if (u < 0) return;
    const TourTable tb = T.tab[t];
    const DevEngine &A = T.eng[tb.ea], &B = T.eng[tb.eb];
    match_restart<SLOTS>(A, tb.sa, u, T.book, T.first_mode, lane);
    match_restart<SLOTS>(B, tb.sb, u, T.book, T.first_mode, lane);
    if (T.moves) match_record_opening(T.moves + (size_t)(u - T.first_game) * A.ncells, u, T.book, T.first_mode, lane);
}

__global__ void k_tour_turn(TourDev T) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T.n_tables) return;
    const TourTable tb = T.tab[t];
    GameHdr *ga = T.eng[tb.ea].ghdr + tb.sa, *gb = T.eng[tb.eb].ghdr + tb.sb;
    const int64_t u = T.tab_game[t];
    int a = 0, b = 0;
    if (u >= 0) {
        const int mover = match_mover(u, ga->ply, T.first_mode);
        a = mover == 0;
        b = mover == 1;
    }
    ga->active = a;
    gb->active = b;
}

// One wave per table, after all engines' searches and move draws of this ply.
template <int SLOTS>
__global__ __launch_bounds__(64) void k_tour_step(TourDev T) {
    const int lane = threadIdx.x;
    const int t = blockIdx.x;
    const int64_t u = T.tab_game[t];
    if (u < 0) return;                                         // idle table
    const TourTable tb = T.tab[t];
    const DevEngine &A = T.eng[tb.ea], &B = T.eng[tb.eb];
    const int sa = tb.sa, sb = tb.sb;
    GameHdr *ga = A.ghdr + sa, *gb = B.ghdr + sb;
    const int ply = ga->ply, ply0 = ga->ply0;                  // (the two slots hold the same game)
    const int ncells = A.ncells;
    const int first = match_first(u, T.first_mode);
    const int mover = first ^ (ply & 1);
    const int mid = mover ? gb->move_id : ga->move_id;
    const int status = mover ? B.thdr[sb].status : A.thdr[sa].status;
    bool voided = status != 0 || mid < 0;                      // as k_match_step
    const int64_t idx = u - T.first_game;
    int winner = 0, len = ply;

    if (!voided) {
        HexWave<SLOTS> h;
        h.load(A.cells + (size_t)sa * SLOTS * 64, lane);
        h.color = ga->color;
        h.winner = ga->winner;
        const Masks<SLOTS> mk = make_masks<SLOTS>(h, lane, ncells);
        int cell = -1;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const uint64_t hit = __ballot(lane_bit(mk.m[s]) && mk.base[s] + rank_below(mk.m[s]) == mid);
            if (hit) cell = s * 64 + (int)__ffsll((long long)hit) - 1;
        }
        if (cell < 0 || ply >= ncells) {
            voided = true;
        } else {
            if (lane == 0) {
                if (T.moves) T.moves[(size_t)idx * ncells + ply] = (int16_t)(cell + 1);
                ga->move_id = mid;  gb->move_id = mid;
                ga->active = 1;     gb->active = 1;
            }
            wave_mem_sync();
            advance_body<SLOTS>(A, sa, nullptr, 0);
            advance_body<SLOTS>(B, sb, nullptr, 0);
            wave_mem_sync();
            winner = ga->winner;
            len = ply + 1;
        }
    }
    if (!voided && winner == 0) return;                        // the game goes on

    if (T.sink >= 0 && !voided)
        match_harvest(A, sa, B, sb, match_sink(T.eng[T.sink]), T.ctr + (size_t)tb.pair * MCTR_COUNT + MCTR_ROWS_LOST, u, first, winner,
                      len, ply0, lane);

    // ---- settle into the pair's tallies; the pair's next round for this table ----
    long long next_u = -1;
    if (lane == 0) {
        unsigned long long *ctr = T.ctr + (size_t)tb.pair * MCTR_COUNT;
        int outcome = 0;
        if (!voided) {
            const int won = winner == 1 ? first : 1 - first;   // colour 1 = the first mover
            outcome = won == 0 ? 1 : -1;
            atomicAdd(ctr + (won == 0 ? MCTR_WINS0 : MCTR_WINS1), 1ull);
            if (winner == 1) atomicAdd(ctr + MCTR_FIRST_WINS, 1ull);
        } else {
            atomicAdd(ctr + MCTR_VOIDED, 1ull);
        }
        T.outcome[idx] = (int8_t)outcome;
        T.length[idx] = (int16_t)len;
        atomicAdd(ctr + MCTR_PLIES, (unsigned long long)(len - ply0));       // the moves searched and played
        atomicAdd(ctr + MCTR_DECIDED, 1ull);
        atomicAdd(T.ctr + (size_t)T.n_pairs * MCTR_COUNT + MCTR_DECIDED, 1ull);
        const unsigned long long nx = atomicAdd(ctr + MCTR_NEXT, 1ull);
        next_u = nx < (unsigned long long)T.rounds ? T.first_game + (long long)tb.pair * T.rounds + (long long)nx : -1;
        T.tab_game[t] = next_u;
    }
    next_u = ((long long)__builtin_amdgcn_readfirstlane((int)(next_u >> 32)) << 32) |
             (unsigned int)__builtin_amdgcn_readfirstlane((int)next_u);
    match_restart<SLOTS>(A, sa, next_u, T.book, T.first_mode, lane);
    match_restart<SLOTS>(B, sb, next_u, T.book, T.first_mode, lane);
    if (T.book.n > 0 && next_u >= 0 && T.moves)
        match_record_opening(T.moves + (size_t)(next_u - T.first_game) * ncells, next_u, T.book, T.first_mode, lane);
}

void azx_launch_tour_init(const TourDev &T, hipStream_t st) {
    const int n = T.n_tables > T.n_engines * T.max_g ? T.n_tables : T.n_engines * T.max_g;
    hipLaunchKernelGGL(k_tour_init, dim3((n + 255) / 256), dim3(256), 0, st, T);
}

void azx_launch_tour_open(const TourDev &T, int slots, hipStream_t st) {
#define CALL(S) hipLaunchKernelGGL((k_tour_open<S>), dim3(T.n_tables), dim3(64), 0, st, T)
    DISPATCH_SLOTS(slots, CALL);
#undef CALL
}

void azx_launch_tour_turn(const TourDev &T, hipStream_t st) {
    hipLaunchKernelGGL(k_tour_turn, dim3((T.n_tables + 255) / 256), dim3(256), 0, st, T);
}

void azx_launch_tour_step(const TourDev &T, int slots, hipStream_t st) {
#define CALL(S) hipLaunchKernelGGL((k_tour_step<S>), dim3(T.n_tables), dim3(64), 0, st, T)
    DISPATCH_SLOTS(slots, CALL);
#undef CALL
}
