/*
 * azx.h -- C ABI of the MI355X-native batched Hex self-play engine (libazx_hip.so).
 *
 * This is the drop-in boundary for azalea's MCTS self-play hot path.  The reference
 * (jseppanen/azalea) has no FFI layer: its seam is the duck-typed Python surface
 * Player.read / Policy.choose_action / SearchTree.search.  Each entry point below names
 * the reference interface (file:line under azalea/) it replaces; azalea_amd/ binds them
 * with ctypes and INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions: plain pointers and sizes only (no torch types).  Every function returns
 * 0 on success or a negative AZX_E* code; azx_last_error() gives the message.  Host
 * buffers are caller-allocated.  An engine handle is NOT thread-safe: one host thread
 * per handle, all device work stream-ordered on the engine's own HIP stream, calls block.
 *
 * Units follow the reference: a "move" is flat tile index + 1 (0 = padding,
 * game/hex.py:151-159); a "move_id"/child index i is the i-th legal move in ascending
 * tile order (search_tree.py:298-308); colour 1 = X/first player, 2 = O.
 */
#ifndef AZX_H
#define AZX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZX_MAX_BOARD 13          /* 11x11 and 13x13 are the BASELINE configs */
#define AZX_MAX_CELLS (AZX_MAX_BOARD * AZX_MAX_BOARD)
#define AZX_CELL_STRIDE 192       /* per-position row stride of dense [*, cells] buffers */
#define AZX_MAX_BATCH 16          /* search_batch_size upper bound */
#define AZX_ROW_METRICS 8         /* floats per replay row returned by azx_play_row_metrics */
/* bytes of one fixed-size replay record (azx_rows_pack / azx_replay_put_records) for a board of `cells` cells */
#define AZX_RECORD_BYTES(cells) ((size_t)((16 + 5 * (cells) + 15) / 16 * 16))

enum {
    AZX_OK = 0,
    AZX_EINVAL = -1,     /* bad argument / configuration */
    AZX_EHIP = -2,       /* HIP runtime failure (message has the hipError string) */
    AZX_ENOMEM = -3,
    AZX_ESTATE = -4,     /* call sequence error (e.g. apply without select) */
    AZX_ENODEV = -5,     /* no MI355X visible: there is no CPU fallback */
    AZX_ERANGE = -6,     /* a folded weight or a tower activation is outside the f16 range of the split-f16 kernels
                            (the reference computes in fp32 throughout, network.py:68-85): azx_set_weights rejects such
                            weights; a call whose evaluations overflowed reports it and its results are not valid */
    AZX_EEXTERNAL = -7   /* the registered external evaluator (azx_set_external_evaluator) returned non-zero, or a row
                            it produced failed the checks of mcts.py:211-213; the message names the first bad row */
};

/* evaluator = what plays the role of Network.run inside mcts.evaluate_batch (mcts.py:202-215) */
enum {
    AZX_EVAL_RESNET = 0,    /* HexNetwork forward on device (network.py:134-152) */
    AZX_EVAL_UNIFORM = 1,   /* uniform priors 1/k, value 0, evaluated inline (BASELINE config 2) */
    AZX_EVAL_UNIFORM_HASH = 2, /* parity stub: prior_by_k table + fnv1a value hash, inline */
    AZX_EVAL_EXTERNAL = 3   /* host supplies value/priors per leaf between select and apply */
};

enum {
    AZX_FLAG_NO_COMPACT = 1, /* keep the reference's never-free arena + moving root_id
                                (search_tree.py:115-132) instead of compacting on advance */
    AZX_FLAG_RANDOM_REFLECT = 2, /* NOT the reference's behaviour for Hex (off by default, outside every parity claim).
                                The reference calls game.random_reflect on every leaf batch before the network sees it
                                (mcts.py:183-186); its Hex implementation returns its inputs and names the one transform
                                that keeps the player's direction, np.rot90(b, 2) (game/hex.py:124-134).  With this flag
                                every evaluation request -- the root request of a search and every leaf -- draws one bit
                                that is a pure function of (seed, game uid, ply, ordinal of the request within that
                                move's search: 0 = root, then 1 + select index of the leaf's batch start + its place
                                among the batch's unique leaves), from the game's key on a stream of its own: it shares
                                nothing with the Dirichlet or move draws and does not depend on the slot, n_games, the
                                half-pool, the launch or the order requests were queued in.  A set bit hands the
                                evaluator the board turned by 180 degrees (cell c -> cells - 1 - c, composed with the
                                perspective flip; the two commute) and the legal list t -> cells + 1 - t in its ORIGINAL
                                order; priors are mapped back, so everything behind the evaluator (azx_put_evals /
                                azx_get_evals "prior j = child j", the trees, the rows) is indexed as without the flag.
                                Internally the engine's per-request word ev_flip carries the turn as bit 1 (bit 0 = the
                                perspective flip).  AZX_EVAL_RESNET and AZX_EVAL_EXTERNAL (phase API and registered
                                evaluator) only: azx_create with AZX_EVAL_UNIFORM / AZX_EVAL_UNIFORM_HASH, which have
                                no network input, is AZX_EINVAL.  Matches and tournaments take the flag per engine.
                                azx_kernel_info reports reflect=on|off.  An addition WITHIN ABI revision 7: azx_config
                                is unchanged. */
    AZX_FLAG_TOWER_F16 = 4   /* NOT the reference's arithmetic (off by default, outside every parity claim).  The 6x64-class
                                fused tower normally carries every fp32 operand as hi + lo f16 halves and issues three
                                MFMAs per product (fp32-class accuracy, the 1e-4 parity tolerance).  With this flag the
                                engine's network runs k_tower_f16_s16 instead: that arithmetic with every lo half taken as
                                zero.  The folded weights (stem with the embedding folded in, the conv layers, the six 1x1
                                head filters) enter as f16(w); the activations written back after each ReLU enter the next
                                conv and the head filters as f16(a); products accumulate in fp32; the folded-BN bias and
                                the residual (the unrounded block input) stay fp32; the one-hot stem input is exact;
                                everything behind the six head planes (FC layers, log-softmax, -99 padding) is unchanged
                                fp32.  An activation beyond 65504 is +inf in f16 and raises AZX_ERANGE as without the flag;
                                the weight range guard of azx_set_weights is the same.  Expect value errors of order 1e-4
                                to 1e-3 and log-prob errors up to a few 1e-2 on peaked trained networks.
                                The WIDE tower (tower variant 5: base_chans a multiple of 128, any board the engine
                                supports, at least one block) has the same switch: k_stem_wide_f16 + k_conv_wide_f16_s16
                                per layer instead of k_stem_wide_f16x3 + k_conv_wide_f16x3_s16.  Every convolution of the
                                tower takes the hi half of each operand only: the folded stem and conv weights enter as
                                f16(w) (part 0 of the same packs), the activation written back after each ReLU enters the
                                next convolution as f16(a), the one-hot stem input is exact; products accumulate in fp32,
                                the folded-BN bias is fp32.  The activation image in memory keeps its layout [cell][C hi |
                                C lo]: the epilogue still writes the split pair and the residual is still read as hi + lo,
                                so the residual stream is NOT rounded to f16 from block to block.  The last layer writes the
                                same unrounded fp32 copy, and k_heads is unchanged: unlike the 6x64 case the head filters
                                and their input are not rounded.  AZX_ERANGE and the weight packs as above.  Expect errors
                                of order 1e-5 to 1e-4 (value) and 1e-4 (log-prob) on randomly initialised networks
                                (DESIGN 7.8); no trained wide network has been measured.
                                AZX_EVAL_RESNET on a shape with such a tower -- the fused tower's (64 channels, at most 121
                                cells) or the wide tower's, at least one block either way -- only, and not together with
                                AZX_TOWER=fp32: azx_create is AZX_EINVAL otherwise.  Matches and tournaments take the flag
                                per engine.  The environment variable AZX_TOWER=f16 selects the same kernels wherever the
                                flag would be accepted and is ignored elsewhere.  azx_kernel_info names the tower.  An
                                addition WITHIN ABI revision 7: azx_config is unchanged. */
};

typedef struct {
    int32_t board_size;          /* N: policy.py:51 */
    int32_t n_games;             /* concurrent game slots on this GPU */
    int32_t simulations;         /* policy.py:55 */
    int32_t search_batch_size;   /* policy.py:56 (<= AZX_MAX_BATCH) */
    float   exploration_coef;    /* c_puct, policy.py:57 (f32: numpy weak-scalar semantics) */
    int32_t exploration_depth;   /* policy.py:58 */
    double  noise_alpha;         /* policy.py:59 */
    double  noise_scale;         /* policy.py:60 */
    double  temperature;         /* policy.py:61 */
    int32_t evaluator;           /* AZX_EVAL_* */
    int32_t num_blocks;          /* policy.py:52 (resnet only) */
    int32_t base_chans;          /* policy.py:53 (resnet only; 64 or multiples of 32) */
    int32_t nodes_per_game;      /* tree arena capacity per game (SearchTreeFull beyond it) */
    int32_t flags;               /* AZX_FLAG_* */
    int32_t device;              /* HIP device ordinal */
    uint64_t seed;               /* base seed; game uid u draws from stream seed+u */
    /* multi-GPU sharding: the j-th game this engine starts (j = slot + n_games * games
     * the slot has started before) has global index uid = j * game_index_stride + game_index_offset.
     * Rank r of W passes (W, r): a fixed seed then plays the same set of games whatever W is.
     * 0 stride = 1 (single engine). */
    int32_t game_index_stride;
    int32_t game_index_offset;
} azx_config;

typedef struct azx_engine azx_engine;

const char *azx_last_error(void);
int azx_version(void);            /* ABI revision: 7 = azx_set_external_evaluator, AZX_EEXTERNAL (throughput self-play and
                                   *     azx_search with a caller-supplied evaluator over device buffers); the azx_match_*
                                   *     entry points were added within revision 7 -- callers detect them by symbol; so
                                   *     were AZX_FLAG_RANDOM_REFLECT and AZX_FLAG_TOWER_F16 (azx_config unchanged) and azx_replay_set_reflect;
                                   * 6 = azx_reserve_cus, azx_replay_put_records_async (self-play beside training);
                                   * 5 = AZX_ERANGE, azx_debug_weights, weights packed on the device
                                   * (4 = 8-float row metrics, azx_kernel_info, azx_debug_set_queue_cap;
                                   *  3 = azx_config.game_index_*, azx_play_stats.sum_game_length) */

/* Policy.initialize / Policy.reset (policy.py:36-63, :76-80): allocate device arenas. */
int azx_create(const azx_config *cfg, azx_engine **out);
void azx_destroy(azx_engine *e);

/* Policy.net weights (policy.py:65-74, network.py:42-61,:120-132): copy + pack the
 * state_dict tensors.  names[i] are state_dict keys; ptrs[i] point at contiguous fp32 data,
 * on the device (torch tensor.data_ptr()) when on_device != 0, else on the host. */
int azx_set_weights(azx_engine *e, int n_tensors, const char *const *names,
                    const void *const *ptrs, const int64_t *counts, int on_device);
/* The trainer changes its weights every step (policy_trainer.py:85-90) and the engine is refreshed on every
 * Player.read, so azx_set_weights folds / splits / re-orders ON THE DEVICE, reading device tensors in place
 * (host arrays are staged first); blocking.  AZX_ERANGE: a BatchNorm-folded weight is not finite or -- for the
 * split-f16 towers -- beyond the f16 range (65504); the message names the tensor, nothing is installed and the
 * engine has no weights until a valid set arrives.
 * Debug / tests: packed operand number `which` as the kernels read it -- *nbytes = its size (-1 past the last one),
 * its name in `name`, its bytes in `out` when cap suffices.  AZX_PACK=host (read at azx_create) selects the scalar
 * host reference packer; the two are bit-identical (tests/test_gpu_weights.py). */
int azx_debug_weights(azx_engine *e, int which, void *out, int64_t cap, int64_t *nbytes, char *name, int name_cap);

/* AZX_EVAL_UNIFORM_HASH only: prior_by_k[k] = the f32 prior a k-move position gets. */
int azx_set_prior_table(azx_engine *e, const float *prior_by_k, int count);

/* HexGame.reset + SearchTree.reset (hex.py:47-49, search_tree.py:59-71) for the listed
 * slots (NULL = all), then replay `n_moves[i]` moves from `moves` (row stride `stride`). */
int azx_reset(azx_engine *e, const int32_t *slots, int n_slots, const int32_t *moves,
              const int32_t *n_moves, int stride);

/* ---- one search, split the way mcts.sample_paths is (mcts.py:258-293) ------------------ */

/* Mark which slots take part in azx_search* / azx_advance (active[n_games], 0 = parked).  All
 * slots are active after azx_create / azx_reset.  A tournament (evaluation.py:46-80) searches, per
 * agent, only the games whose turn it is. */
int azx_set_active(azx_engine *e, const int32_t *active);

/* SearchTree.search for every active slot from its current root (search_tree.py:73-113).
 * noise: NULL -> no noise if noise_scale==0, else device RNG Dirichlet (throughput mode);
 * else host Dirichlet draws [n_games][n_select][noise_stride] f64, one row per select_leaf
 * (mcts.py:126-131) -- parity mode keeps numpy's RandomState on the host.
 * With AZX_EVAL_EXTERNAL this returns AZX_ESTATE -- drive the phases below instead -- unless an evaluator is
 * registered (azx_set_external_evaluator): the search then calls it between its phases. */
int azx_search(azx_engine *e, const double *noise, int n_select, int noise_stride,
               double noise_scale);

/* external-evaluator phases (parity tests; also how a custom network would plug in):
 *   begin -> [pending>0: get_leaves, put_evals] -> repeat { step -> get_leaves -> put_evals }
 * azx_search_begin emits the root evaluation requests (mcts.py:272-273),
 * azx_search_step applies the pending evaluations (expand mcts.py:226-239, backup :242-255)
 * and, if batches remain, selects the next batch (mcts.py:46-76).  *n_pending receives the
 * number of positions waiting for evaluation; *done is 1 when all batches are applied. */
int azx_search_begin(azx_engine *e, const double *noise, int n_select, int noise_stride,
                     double noise_scale, int *n_pending);
int azx_search_step(azx_engine *e, int *n_pending, int *done);
/* pending positions in (slot, leaf order) order: boards[n][cells] int32 already flipped to
 * the first player's view (mcts.py:178-181), legal_moves[n][cells] padded with 0 (flipped
 * tiles, original order), slot[n], k[n].  With AZX_FLAG_RANDOM_REFLECT about half the rows come
 * turned by 180 degrees as well (board and tiles alike). */
int azx_get_leaves(azx_engine *e, int cap, int32_t *boards, int32_t *legal_moves,
                   int32_t *slot, int32_t *k, int *n_out);
/* value[n], prior[n][cells] (prior j = child j, first k entries) in the same order */
int azx_put_evals(azx_engine *e, int n, const float *value, const float *prior);
/* AZX_EVAL_RESNET driven through the phase API: the device network has already evaluated the
 * pending positions; read its (value, prior) back in azx_get_leaves order (call that first).
 * This is the "evaluation tape" parity tests replay through the CPU oracle. */
int azx_get_evals(azx_engine *e, int cap, float *value, float *prior, int *n_out);

/* ---- a caller-supplied evaluator on the device (custom networks, policy.py:11-18) ------------------------
 * The reference's evaluate_batch hands net.run every leaf of a batch (mcts.py:170-215).  Registered on an
 * AZX_EVAL_EXTERNAL engine, fn plays that role for the whole pool at once: wherever the resnet path evaluates
 * (root requests of a search, then each selected batch) the engine calls
 *   fn(user, n, kmax, board_dev, legal_moves_dev, value_dev, prior_dev, hip_stream)
 * once, with every pending position of every active slot -- up to n_games * search_batch_size rows, in
 * (slot, leaf) order (azx_get_leaves' order, whatever order the GPU queued them in):
 *   board_dev        int32 [n][cells]  the first player's view (mcts.py:178-181), 0 empty / 1 / 2
 *   legal_moves_dev  int32 [n][cells]  tile + 1 in the flipped frame, original order, 0-padded; kmax = the batch's
 *                                      largest legal-move count (a network takes [:, :kmax], prep.batch_games)
 *   value_dev        f32   [n]         out: value for the player to move
 *   prior_dev        f32   [n][cells]  out: entry j = prior of legal move j; the first k_i entries of row i are read
 *   hip_stream       the engine's hipStream_t: fn enqueues its work on it (or finishes it before returning).
 * All four buffers belong to the engine and are valid during the call only.  fn returns 0, or non-zero to fail
 * the call.  The engine checks every row as mcts.py:211-213 asserts (priors >= 0, |sum of the k priors - 1| <
 * 1e-4) and that the value is finite.  A non-zero return or a failed check fails the call with AZX_EEXTERNAL
 * (the message names the first bad row); the searches in flight are left half done (virtual loss applied), so
 * the engine refuses search and play calls with AZX_ESTATE until all its slots have been azx_reset.
 * With fn registered, azx_search, azx_play, azx_play_device, azx_replay_fill and azx_play_steps run on the
 * engine's one stream, and azx_play_stats.net_seconds / net_launches count the hand-overs (export + fn +
 * import).  azx_match_play calls fn as well, for the slots in which this engine is the mover, and there advances
 * two such engines' searches in turn (the match section below); fn still gets its own engine's stream.
 * Without fn every entry point behaves as before (AZX_ESTATE for search and play on this evaluator; azx_match_create
 * refuses the engine).  The phase API above is unaffected. */
typedef int (*azx_eval_fn)(void *user, int n, int kmax, const int32_t *board_dev, const int32_t *legal_moves_dev,
                           float *value_dev, float *prior_dev, void *hip_stream);
/* AZX_EVAL_EXTERNAL engines only (else AZX_EINVAL); fn = NULL unregisters */
int azx_set_external_evaluator(azx_engine *e, azx_eval_fn fn, void *user);

/* ---- results ---------------------------------------------------------------------------- */

/* root.move_stats + root stats (search_tree.py:106-112, :192-204): per slot, child arrays
 * [n_games][cells] dense by child index (first k valid). Any pointer may be NULL. */
int azx_get_root(azx_engine *e, int32_t *k, int32_t *legal_moves, float *child_visits,
                 float *child_value, float *child_prior, float *root_visits,
                 float *root_value, int32_t *num_nodes, float *search_value);
/* per slot: 0 ok, 1 = the arena overflowed during the last search (SearchTreeFull,
 * search_tree.py:258-259): the caller skips the game as parallel_player.py:73-76 does */
int azx_get_status(azx_engine *e, int32_t *status);
/* per slot: SearchTree.num_nodes as the reference counts it (search_tree.py:112 'search_tree_nodes'): nodes
 * allocated since the tree's last reset and never reclaimed (search_tree.py:115-132) -- the arena compaction
 * here frees nodes, azx_get_root's num_nodes is the arena's live count. */
int azx_get_tree_nodes(azx_engine *e, int32_t *nodes);

/* game state per slot: HexGame.state (hex.py:55-60): board [n_games][cells] int32,
 * color (0/1), result (0/1/3), ply. */
int azx_get_games(azx_engine *e, int32_t *board, int32_t *color, int32_t *result,
                  int32_t *ply);

/* Policy.execute_action + HexGame.step (policy.py:170-176, hex.py:172-179): per slot the
 * chosen child index (move_id), or -1 to leave the slot untouched. */
int azx_advance(azx_engine *e, const int32_t *move_ids);

/* raw tree of one slot in the reference's six-array model (search_tree.py:48-55) */
int azx_tree_dump(azx_engine *e, int slot, int cap, int32_t *parent, int32_t *first_child,
                  int32_t *num_children, float *num_visits, float *total_value,
                  float *prior_prob, int32_t *num_nodes, int32_t *root_id);

/* ---- network only: Network.run inference branch (network.py:87-91,:103-105) ------------- */
int azx_forward(azx_engine *e, int B, int K, const int32_t *boards,
                const int32_t *legal_moves, float *value, float *moves_logprob);

/* ---- rules only: HexGameImpl.step/legal_moves/result over move lists (hex.py:151-179) --- */
/* moves[n_games][stride]; outputs per ply p < length: result after the move, number of
 * legal moves before it, and the empties bitmask before it (4 x u64 per ply).
 * board_size need not match any engine. */
int azx_hex_replay(int device, int board_size, int n_games, const int32_t *moves,
                   const int32_t *length, int stride, int32_t *result_out,
                   int32_t *nlegal_out, uint64_t *empties_out, int32_t *final_board);

/* ---- throughput mode: Player.read (parallel_player.py:24-28, :41-52) -------------------- */
typedef struct {
    int64_t positions;        /* rows written */
    int64_t games;            /* games finished (metrics['games']) */
    int64_t game_errors;      /* SearchTreeFull games skipped (parallel_player.py:73-76) */
    int64_t plies;            /* engine moves executed over all slots */
    int64_t selects;          /* select_leaf calls */
    int64_t evals;            /* positions evaluated */
    int64_t sum_depth, sum_k_interior, sum_k_leaf;   /* roofline byte model inputs */
    double  sum_search_value, sum_root_width, sum_action_logprob, sum_reward_last;
    double  seconds;          /* device time of the call (hipEvents on the engine stream) */
    double  mcts_seconds;     /* device time in the tree kernels */
    int64_t mcts_launches;    /* engine moves those launches covered (one per k_mcts search launch) */
    double  net_seconds;      /* device time in the network kernels (tower + heads), per batch */
    int64_t net_launches;
    int64_t mcts_kernel_launches;   /* kernel launches behind mcts_seconds (k_play: many moves each) */
    double  sum_game_length;  /* plies of the finished games, counted from the empty board (metrics: moves_per_game
                                 of games that started from an azx_reset prefix; rows only cover the plies searched) */
} azx_play_stats;

/* Self-play until >= min_positions rows from FINISHED games are available (whole games
 * only, like batch_examples) or max_plies engine steps have run (0 = unbounded).
 * Rows: board int32[cap][cells] (absolute colours), color[cap], nlegal[cap],
 * moves_prob f32[cap][cells] dense by child index, reward f32[cap], game_uid[cap]. */
int azx_play(azx_engine *e, int64_t min_positions, int64_t max_plies, int64_t cap,
             int32_t *board, int32_t *color, int32_t *nlegal, float *moves_prob,
             float *reward, int64_t *game_uid, azx_play_stats *stats);

/* per-ply search metrics of the rows the last azx_play / azx_play_device / azx_replay_fill call harvested, in row order:
 * metrics[n][AZX_ROW_METRICS] = {search_value (mcts.py:291), search_root_width (search_tree.py:110), log-probability
 * of the move drawn (play_game.py:43), 1 on the first row of a game else 0, search_root_visits (mean child
 * visits, search_tree.py:110), search_tree_nodes (nodes allocated since the tree's last reset, never reclaimed:
 * search_tree.py:112), search_root_children (search_tree.py:111), 0}.
 * play_game averages them over a game's plies and Player.read sums those means over the games it returns
 * (play_game.py:73-76, parallel_player.py:50-51). */
int azx_play_row_metrics(azx_engine *e, int64_t cap, float *metrics, int64_t *n_out);

/* bench hook: run `plies` lock-step engine moves on all slots (device RNG, finished games
 * restart in place), no row transfer; fills stats. */
int azx_play_steps(azx_engine *e, int64_t plies, azx_play_stats *stats);

/* ---- device-resident replay buffer ------------------------------------------
 * Replaces, for a trainer that keeps its minibatches on the GPU: ReplayBuffer.put's wrap-around
 * FIFO (azalea/replay_buffer.py:134-149), Player.read feeding it (parallel_player.py:41-52,
 * replay_buffer.py:121-132) and the DataLoader + prep.torch_batch_replays collate
 * (policy_trainer.py:51-56, prep.py:24-39).  Rows live in a fixed-capacity ring in HBM.
 * The fresh-example accounting of ReplayBuffer.consume (a float counter) stays with the caller. */

/* allocate (or replace) the ring: `capacity` rows, empty */
int azx_replay_create(azx_engine *e, int64_t capacity);
/* capacity, rows held (<= capacity) and the next write position */
int azx_replay_state(azx_engine *e, int64_t *capacity, int64_t *size, int64_t *write_idx);
/* restore size/write position (ReplayBuffer.load_state_dict, replay_buffer.py:160-165) */
int azx_replay_set_state(azx_engine *e, int64_t size, int64_t write_idx);
/* ReplayBuffer.put of n host rows (same row layout as azx_play's outputs): written at the write
 * position in order, wrapping; when n > capacity only the last `capacity` rows survive, as with
 * the reference's recursive put. */
int azx_replay_put(azx_engine *e, int64_t n, const int32_t *board, const int32_t *color,
                   const int32_t *nlegal, const float *moves_prob, const float *reward);
/* Player.read(min_positions) + ReplayBuffer.put without a host round trip: plays whole games
 * (throughput mode, like azx_play) until >= min_positions rows were harvested and moves them
 * into the ring.  *rows_out = rows added. */
int azx_replay_fill(azx_engine *e, int64_t min_positions, int64_t max_plies, int64_t *rows_out,
                    azx_play_stats *stats);
/* ---- multi-GPU replay exchange -------------------------------------------------------
 * Replaces the reference's only data-parallel return path -- pickled ReplayDataFrames over worker pipes
 * (process_pool.py:31-47, parallel_player.py:41-52) -- by one all-gather of fixed-size records between
 * DEVICE buffers: every rank plays its share (azx_play_device), packs the harvested rows into records
 * (azx_rows_pack), the caller all-gathers the record buffers (RCCL over xGMI) and appends all of them to
 * its ring (azx_replay_put_records).  Record layout (AZX_RECORD_BYTES(cells) bytes):
 *   0 game_uid i64 | 8 reward f32 | 12 color i16 | 14 nlegal i16 | 16 moves_prob f32[cells] |
 *   16+4*cells board u8[cells] | zero padding to a multiple of 16. */

/* Player.read(min_positions) that leaves the rows in the engine's harvest queue (whole games only,
 * like azx_play); *rows_out = rows now queued, valid until the next azx_play* / azx_replay_fill call. */
int azx_play_device(azx_engine *e, int64_t min_positions, int64_t max_plies, int64_t *rows_out,
                    azx_play_stats *stats);
/* queue rows [first, first+n) -> records in the DEVICE buffer records_dev (n * AZX_RECORD_BYTES). Blocking. */
int azx_rows_pack(azx_engine *e, int64_t first, int64_t n, void *records_dev);
/* queue rows [first, first+n) -> host arrays in azx_play's row layout (board int32[n][cells], color[n], nlegal[n],
 * moves_prob f32[n][cells], reward[n], game_uid[n]); any pointer may be NULL.  Valid for whatever filled the queue
 * last: azx_play / azx_play_device, or a harvesting match / tournament (azx_match_set_harvest,
 * azx_tournament_set_harvest), until that engine's next play, match or tournament call.  AZX_EINVAL for rows outside
 * the rows queued.  Blocking.  An addition WITHIN ABI revision 7: callers detect it by symbol (dlsym azx_rows_read). */
int azx_rows_read(azx_engine *e, int64_t first, int64_t n, int32_t *board, int32_t *color, int32_t *nlegal,
                  float *moves_prob, float *reward, int64_t *game_uid);
/* ReplayBuffer.put of n records held in a DEVICE buffer: FIFO with the wrap-around / overflow behaviour
 * of azx_replay_put.  Blocking. */
int azx_replay_put_records(azx_engine *e, int64_t n, const void *records_dev);
/* The same put ENQUEUED on the caller's stream (a hipStream_t) and not synchronised: ordered with the
 * azx_replay_collate_async reads and the training step on that stream, and independent of the engine's own stream --
 * so a trainer thread can take rows into the ring while another host thread is inside azx_play_device on the same
 * handle (the one pairing of concurrent calls a handle allows; play-ahead self-play, replay_buffer.py:121-132 over
 * process_pool.py:29-47).  records_dev must stay valid until the stream has passed this point. */
int azx_replay_put_records_async(azx_engine *e, int64_t n, const void *records_dev, void *hip_stream);
/* Leave `cus_per_xcd` compute units of every XCD free of this engine's kernels (0 = use all): the engine's streams are
 * re-made with a CU mask (hipExtStreamCreateWithCUMask), so a training step on another stream finds empty CUs at
 * once instead of queueing behind resident tower blocks.  Rounded up to a multiple of 4: an XCD deals workgroups
 * round-robin to its 4 shader engines, so taking CUs from fewer than all of them costs the same throughput as taking
 * one from each (tools/microbench/cu_mask.hip).  Call between plays (the streams are drained).  *reserved_out = CUs
 * actually left free on the whole device. */
int azx_reserve_cus(azx_engine *e, int cus_per_xcd, int *reserved_out);

/* prep.batch_replays of the rows `indices[0..batch)` (host array; each < rows held) into DEVICE
 * buffers with row stride board_size^2: color i64[batch], legal_moves i32[batch][cells] (ascending
 * tile+1, zero padded), result i64[batch] (always 0), board i32[batch][cells],
 * moves_prob f32[batch][cells] (zero padded), reward f32[batch].  *max_k_out (host) = the batch's
 * largest legal-move count: the reference's collate pads legal_moves/moves_prob to exactly that
 * width, so callers slice [:, :max_k].  Blocking. */
int azx_replay_collate(azx_engine *e, int64_t batch, const int64_t *indices, int64_t *color_dev,
                       int32_t *legal_moves_dev, int64_t *result_dev, int32_t *board_dev,
                       float *moves_prob_dev, float *reward_dev, int32_t *max_k_out);

/* azx_replay_collate enqueued on the CALLER's stream (hipStream_t; NULL = default) and NOT synchronised, without
 * max_k (the consumer takes full-width rows): a trainer whose step runs on that stream (azx_train_step) queues collate
 * + step and moves on.  `indices` is copied before the call returns.  Ring writes (azx_replay_fill / azx_replay_put*,
 * blocking calls on the engine's stream) must be ordered after these reads by the caller: synchronise the stream
 * before a refill. */
int azx_replay_collate_async(azx_engine *e, int64_t batch, const int64_t *indices, int64_t *color_dev,
                             int32_t *legal_moves_dev, int64_t *result_dev, int32_t *board_dev,
                             float *moves_prob_dev, float *reward_dev, void *hip_stream);

/* NOT the reference's batch (off by default).  The reference trains on the boards as the replay rows hold them --
 * absolute colours, the second player's positions included (policy_trainer.py:84-85 -> network.py:92-102: no use of
 * `color`) -- while its search hands the network every position in the FIRST player's view (mcts.py:178-181:
 * flip_player_board_moves on the rows with color == 1).  With on != 0 both collates hand out the rows of the second
 * player in that view: colours swapped, board mirrored along the anti-diagonal, each legal move mapped with it in its
 * original list position (moves_prob stays aligned; `color` still reports the mover).  The training distribution then
 * is the distribution the search evaluates. */
int azx_replay_set_mover_view(azx_engine *e, int on);

/* NOT the reference's batch either (off by default): the training-side twin of AZX_FLAG_RANDOM_REFLECT.  The reference
 * calls game.random_reflect on every training batch (policy_trainer.py:84); for Hex that is the identity
 * (game/hex.py:124-134).  With on != 0 both collates draw one bit per OUTPUT row from (seed, number of collates --
 * blocking or enqueued -- since this call, row b of the batch), never from the ring index, and hand a row whose bit is
 * set out turned by 180 degrees: the board with its cell index reversed (c -> cells - 1 - c), every legal entry t as
 * cells + 1 - t in its ORIGINAL list position (moves_prob stays aligned), colour, reward, max_k and padding untouched.
 * It composes with the mover view: view first, then the turn.  The ring never changes; every call resets the collate
 * count.  An addition WITHIN ABI revision 7 (azx_version stays 7): callers detect it by symbol
 * (dlsym azx_replay_set_reflect). */
int azx_replay_set_reflect(azx_engine *e, int on, uint64_t seed);

/* Playout cap randomisation for throughput self-play (Wu 2019, "Accelerating Self-Play Learning in Go", 3.1).  NOT the
 * reference's behaviour (off by default, outside every parity claim): the reference searches every ply with
 * `simulations` and records every ply.  With the cap set, every ply of a self-play game is with probability full_prob
 * a FULL search -- exactly today's ply: cfg.simulations / search_batch_size + 1 select batches, Dirichlet noise, one
 * replay row -- and otherwise a FAST search of fast_simulations / search_batch_size + 1 batches (the reference's
 * rounding rule, mcts.py:268, applied to fast_simulations) that takes NO Dirichlet noise whatever noise_scale is,
 * writes NO replay row and no per-row metrics, and only keeps the game moving: its move is drawn exactly as a full
 * ply's (temperature while ply < exploration_depth, then the most-visited child, from the same Philox words) and the
 * tree is carried to the next ply as always.
 *   The draw is one bit per ply, a pure function of (cfg.seed, the game's uid, the ply counted from the empty board),
 * from the game's key on a stream of its own: nothing of it is shared with the Dirichlet words, the reflection bits
 * or the move draw, and it does not depend on the slot, n_games, the half-pool or the launch.  The ply is full iff
 * the 32-bit word is below the integer threshold ceil(full_prob * 2^32), clamped to [1, 2^32]; device and host use
 * the same function, azx_playout_cap_is_full is it on the host.
 *   It applies to azx_play, azx_play_device, azx_replay_fill and azx_play_steps (persistent k_play, per-move launches,
 * the pipelined half-pools, a registered external evaluator) and to nothing else: azx_search, the phase API and
 * azx_forward run cfg.simulations whatever the cap is, and azx_match_play / azx_tournament_play refuse an engine whose
 * cap is on with AZX_EINVAL before touching any engine (their harvest assumes one row per moved ply).
 *   A game's recorded rows stay contiguous with plies ascending; colour and the sign of the reward come from each
 * row's own ply; row metric 3 flags the game's first RECORDED row; search_value is normalised by the full search's
 * select count.  A game with no full ply counts in azx_play_stats.games and sum_game_length and contributes no rows
 * and nothing to sum_reward_last.  plies, selects and evals count every ply; sum_search_value, sum_root_width and
 * sum_action_logprob cover the recorded plies only (they stay sums over the rows).
 *   full_prob must be in (0, 1] and fast_simulations in [1, cfg.simulations]; anything else is AZX_EINVAL before any
 * device work and leaves the previous setting in place.  (1.0, cfg.simulations) clears the cap, and so does the named
 * form (1.0, 0).  With the cap never set, or cleared, every call launches the same kernels and returns the same bytes
 * as without this entry point.  May be called between calls, for any evaluator.  azx_kernel_info reports cap=off or
 * cap=<full_prob>/<fast_simulations>.  A play call waits for recorded rows: with a full_prob so small that hardly any
 * ply is full, give azx_play / azx_play_device / azx_replay_fill a max_plies.  Playing strength and training
 * efficiency under a cap are not measured.
 * Additions WITHIN ABI revision 7 (azx_version stays 7; azx_config and azx_play_stats are unchanged): callers detect
 * them by symbol (dlsym azx_set_playout_cap). */
int azx_set_playout_cap(azx_engine *e, double full_prob, int fast_simulations);
/* host only, no device call: 1 if ply `ply` of game `uid` under engine seed `seed` is a full search at full_prob, else
 * 0; AZX_EINVAL (negative) for full_prob outside (0, 1] or ply < 0. */
int azx_playout_cap_is_full(uint64_t seed, int64_t uid, int ply, double full_prob);
/* out4 = {full plies, fast plies, games harvested with zero rows, 0}, counted since the cap was last set (all 0 while
 * it has never been set). */
int azx_playout_cap_stats(azx_engine *e, int64_t out4[4]);

/* Resignation for throughput self-play, with no-resign calibration games (AlphaGo Zero, Methods "Self-play").  NOT the
 * reference's behaviour (off by default, outside every parity claim): the reference plays every game to the end.
 *   The resign statistic of a ply is v = root.total_value / root.num_visits of the slot's root after the ply's search:
 * ONE float32 IEEE division of the two numbers azx_get_root returns as root_value and root_visits.  total_value is kept
 * in the node's own perspective, so v is the mean backed-up value for the player to move: positive is good for the
 * mover.  The decision is taken in the move draw, after the move is drawn: a ply that resigns has consumed the same
 * Philox words and has written the same replay row as the ply that plays on.
 *   The mover resigns at a ply iff resignation is set, the game is not exempt, ply >= min_ply (ply counted from the
 * empty board), root.num_visits > 0 and v < threshold.  Every searched ply is judged, the fast plies of a playout cap
 * included.  A resigning ply places no stone: the game ends there and the winner is the colour that did not resign.
 * The ply's replay row is recorded as always (one row on a full ply, none on a fast ply of a playout cap): a searched
 * position with a known outcome.  The game is harvested exactly as a won game is: rows contiguous with plies
 * ascending, colour and reward sign from each row's own ply, metric 3 on the first recorded row, games,
 * sum_reward_last and the queue-full parking path as always.  azx_play_stats.plies, selects and evals count the
 * resigning ply (it was searched); sum_game_length adds the stones on the board at resignation.
 *   Exempt games: one bit per game, a pure function of (cfg.seed, the game's uid), from the game's key on a stream of
 * its own -- nothing of it is shared with the Dirichlet words, the reflection bits, the playout-cap word or the move
 * draw, and it does not depend on the slot, n_games, the half-pool or the launch.  The game is exempt iff the 32-bit
 * word is <= ceil(keep_prob * 2^32) - 1: keep_prob == 0 exempts none, keep_prob == 1 all.  Device and host use the same
 * function; azx_resign_is_exempt is it on the host.  An exempt game plays to the end, bit for bit as with resignation
 * off, and remembers the first ply at which the rule's other conditions held: its "crossing".
 *   Row metric 7 (always 0 otherwise) carries v for every recorded row while resignation is set, exempt games included.
 *   It applies to azx_play, azx_play_device, azx_replay_fill and azx_play_steps (persistent k_play, per-move launches,
 * the pipelined half-pools, a registered external evaluator) and to nothing else: azx_search, the phase API and
 * azx_advance never resign, and azx_match_play / azx_tournament_play refuse an engine whose resignation is set with
 * AZX_EINVAL before touching any engine (their harvest assumes one row per moved ply).
 *   threshold must be in [-1, 1], min_ply >= 0 and keep_prob in [0, 1], all finite; anything else is AZX_EINVAL before
 * any device work and leaves the previous setting in place.  May be called between calls, for any evaluator; games in
 * progress are judged from their next ply on.  The call zeroes the statistics of azx_resign_stats.  With resignation
 * never set, or cleared (azx_clear_resign), every call launches the same kernels and returns the same bytes as without
 * these entry points.  azx_kernel_info reports resign=off or resign=<threshold>/<min_ply>/<keep_prob>.  The effect on
 * playing strength and training efficiency is NOT measured.
 * Additions WITHIN ABI revision 7 (azx_version stays 7; azx_config and azx_play_stats are unchanged): callers detect
 * them by symbol (dlsym azx_set_resign). */
int azx_set_resign(azx_engine *e, double threshold, int min_ply, double keep_prob);
int azx_clear_resign(azx_engine *e);
/* host only, no device call: 1 if game `uid` under engine seed `seed` is exempt from resigning at keep_prob, else 0;
 * AZX_EINVAL (negative) for a keep_prob that is not a finite number in [0, 1]. */
int azx_resign_is_exempt(uint64_t seed, int64_t uid, double keep_prob);
/* Counted since the last azx_set_resign, over the games that both started and finished after it (a game is in progress
 * once a ply of it has been played; SearchTreeFull games count in none):
 *   out8[0] games resigned                        out8[1] non-exempt games played to the end
 *   out8[2] exempt games finished                 out8[3] exempt games with a crossing
 *   out8[4] of those, games the crossing mover went on to WIN (the false positives)
 *   out8[5] sum of the ply at resignation over [0]
 *   out8[6] sum over [3] of (final length - crossing ply): the plies resignation would have saved
 *   out8[7] 0
 * They live in an array of their own: azx_debug_counters keeps its 16 words. */
int azx_resign_stats(azx_engine *e, int64_t out8[8]);
/* tests and analysis: v[n_games] = the resign statistic of every slot's current root, by the device function the move
 * draw uses, whatever the setting; NaN where the root is unevaluated or unvisited. */
int azx_resign_value(azx_engine *e, float *v);

/* Early stop of a search whose move can no longer change, for throughput self-play.  NOT the reference's behaviour
 * (off by default, outside every parity claim): the reference runs every search to its last simulation.
 *   From exploration_depth on the move is drawn at temperature 0: the most-visited root child is played, and the
 * replay row is the same distribution, one-hot on that child.  Once the leading root child is further ahead than the
 * selects still to come, those selects can change neither the move nor the row; they only deepen the subtree that is
 * carried to the next ply.
 *   The rule.  The search of a ply stops early iff all of the following hold:
 *     - the option is set;
 *     - the ply is drawn at temperature 0, i.e. ply >= exploration_depth or temperature == 0, the same expression the
 *       move draw uses;
 *     - at a batch boundary, n1 - n2 > batches_left * search_batch_size.
 *   A batch boundary means all earlier batches are expanded and backed up and their virtual losses undone (the top of
 * the select loop with nothing pending).  n1 and n2 are the largest and second-largest num_visits among the root's
 * children; n2 = 0 with one child.  The counts are integers held in float32, so the comparison is exact.  The
 * inequality is strict: at a stop the leader is unique, and no tie can form later, because a select adds at most one
 * visit to one root child.  An unevaluated root (all counts 0) never satisfies the rule.
 *   Stopping means batches_left = 0: the slot then behaves as a slot whose batches are used up already does -- no
 * selects and no queued rows in the move's remaining launches, the same launch structure.  Everything else is as
 * always: Dirichlet noise per select, the Philox move draw, the row, the carried subtree.  Resignation's judgement
 * (azx_set_resign) is then made on the stopped search's root.  A playout cap's fast plies stop early too when they are
 * temperature-0 plies.  While the option is on, row metric 0 and azx_play_stats.sum_search_value are divided by the
 * selects the ply made, not by the full search's select count (0 where a stopped ply made none).
 *   It applies to azx_play, azx_play_device, azx_replay_fill and azx_play_steps (persistent k_play, per-move launches,
 * the pipelined half-pools, a registered external evaluator) and to nothing else: azx_search and the phase API run
 * cfg.simulations whatever the option is, and azx_match_play / azx_tournament_play refuse an engine with the option
 * set with AZX_EINVAL before touching any engine.
 *   on must be 0 or 1; anything else is AZX_EINVAL and leaves the setting in place.  May be called between calls, for
 * any evaluator.  The call zeroes the statistics of azx_early_stop_stats.  With the option never set, or cleared
 * (on = 0), every call launches the same kernels and returns the same bytes as without these entry points.
 * azx_kernel_info reports estop=on or estop=off.  What the option buys in plies per second depends on the network and
 * is given in DESIGN 7.11; its effect on playing strength and training efficiency (the cost is a thinner carried
 * subtree) is not measured.
 * Additions WITHIN ABI revision 7 (azx_version stays 7; azx_config and azx_play_stats are unchanged): callers detect
 * them by symbol (dlsym azx_set_early_stop). */
int azx_set_early_stop(azx_engine *e, int on);
/* out4 = {temperature-0 plies searched under the option, plies stopped before their last batch, batches skipped (the
 * sum of batches_left at the stops), 0}, counted since the last azx_set_early_stop.  They live in an array of their
 * own: azx_debug_counters keeps its 16 words. */
int azx_early_stop_stats(azx_engine *e, int64_t out4[4]);

/* Training targets of the rows throughput self-play records: visit-share policy rows and z/q-blended rewards.  NOT the
 * reference's behaviour (off by default, outside every parity claim): the reference records as_distribution(counts, T)
 * with the T of the move draw -- one-hot on the most-visited child from exploration_depth on, because its
 * Policy.choose_action has one `probs` array for the draw and for the row -- and gives every row of a game the final
 * outcome z.  AlphaZero trains on the visit distribution at every ply and makes only the played move greedy.
 *   The move draw is untouched: the same weights, the same total, the same Philox words, the same chosen child.  Row
 * metric 2 stays the log-probability of the drawn move under the draw's distribution.  A game is move for move the game
 * the same seed plays with the option off; only what its rows teach differs.
 *   policy_rows = AZX_ROWS_VISITS: the row written at a recorded ply is row[j] = nv_j / nv_sum.  nv_j are the root
 * children's num_visits, integers held in float32, and nv_sum is their sum, which is exact.  The division is ONE float32
 * IEEE division: the expression the reference row already is at T = 1, so rows of T = 1 plies are bit for bit what they
 * were.  Rows of greedy plies (ply >= exploration_depth or temperature == 0) and of plies with any other T become the
 * visit shares.  A root with nv_sum == 0 cannot occur at a recorded ply; if it does, the reference row is written.
 *   value_mix = lambda > 0: the move draw leaves v = root.total_value / root.num_visits in row metric 7 -- the resign
 * statistic of azx_set_resign, the mover's view, the same float resignation stores there -- and the harvest stores
 * reward = (1 - lambda) * z + lambda * v.  z is the reward as it is without the option, already in the mover's view, as
 * v is.  The blend is two float32 products and one sum, unfused.  If v is not finite the reward is z; lambda = 0 stores
 * z itself, with no arithmetic.  azx_play_stats.sum_reward_last keeps summing z.
 *   Row metric 7 carries v whenever resignation or either part of this option is set, and 0 otherwise.
 *   Beside the other options.  A fast ply of a playout cap still records nothing.  Resignation judges as before, and
 * the rows of a resigned game blend the conceded z.  Under early stop the row is the visit shares AT THE STOP: early
 * stop's statement that the skipped selects cannot change the row holds for the reference's one-hot row only, not for
 * AZX_ROWS_VISITS -- the move is still the one a full search plays, the row is that of the shorter search.
 *   It applies to azx_play, azx_play_device, azx_replay_fill and azx_play_steps (persistent k_play, per-move launches,
 * the pipelined half-pools, a registered external evaluator) and to nothing else: every other launch reads "off", and
 * azx_match_play / azx_tournament_play refuse an engine with the option set with AZX_EINVAL before touching any engine
 * (their harvest records the reference's rows and the outcome).
 *   value_mix must be in [0, 1]; NaN, a value outside [0, 1] or an unknown policy_rows is AZX_EINVAL and leaves the
 * setting in place.  (AZX_ROWS_REFERENCE, 0.0f) is "off", the state of an engine on which the call was never made.  May
 * be called between calls, for any evaluator; rows of games in progress are written under the new setting from their
 * next ply on, and a game is harvested under the setting of the call that harvests it.  The call zeroes the statistics
 * of azx_train_targets_stats.  With the option never set, or cleared, every call launches the same kernels and returns
 * the same bytes as without these entry points: rows, rewards, metrics (metric 7 = 0), play statistics.
 * azx_kernel_info reports targets=off or targets=<visits|reference>/<value_mix>.  What the option does to playing
 * strength is given in DESIGN 7.12 as far as it is measured.
 * Additions WITHIN ABI revision 7 (azx_version stays 7; azx_config and azx_play_stats are unchanged): callers detect
 * them by symbol (dlsym azx_set_train_targets). */
#define AZX_ROWS_REFERENCE 0   /* row = as_distribution(counts, T of the move draw): today's rows */
#define AZX_ROWS_VISITS    1   /* row = counts / sum(counts) at every recorded ply, whatever T */
int azx_set_train_targets(azx_engine *e, int policy_rows, float value_mix);
int azx_get_train_targets(azx_engine *e, int *policy_rows, float *value_mix);
/* out4 = {rows recorded while the option is on, of those the rows of greedy plies, of those the rows with more than one
 * visited child (the rows that differ from the reference's), 0}, counted since the last azx_set_train_targets by the
 * lane that writes the row's metrics.  They live in an array of their own: azx_debug_counters keeps its 16 words. */
int azx_train_targets_stats(azx_engine *e, int64_t out4[4]);

/* Forced playouts at the root and policy target pruning, for throughput self-play (Wu 2019, "Accelerating Self-Play
 * Learning in Go", section 3.2).  NOT the reference's behaviour (off by default, outside every parity claim): the
 * reference selects by PUCT alone and records every visit.
 *   Every root select draws fresh Dirichlet noise, so a child the noise lifts once gets one visit and is then usually
 * dropped: the search never learns whether the move was good.  Forcing gives such a child about sqrt(k * P * S)
 * visits; pruning then takes out of the move draw and of the recorded row the visits PUCT would not have spent.
 *   All arithmetic is float32 and unfused, divide and sqrt IEEE; counts are integers held in float32.
 *   Forcing, in the root level of every select of a FULL search (a playout cap's fast plies never force; with the cap
 * off every search is full).  n_j = the root children's num_visits as that select sees them, virtual losses of the
 * batch in flight included; S = their sum (the integer under the square root of mcts.py:132); P_j = the prior that
 * select scores with (noised if noise is on, the stored prior otherwise).  The forced set is
 *       { j : n_j > 0 and n_j * n_j < (k * P_j) * S }.
 * If it is non-empty the select descends into its lowest-index member instead of the PUCT argmax.  Below the root
 * nothing changes; virtual loss, dedup, expand and backup are as always.
 *   Pruning (prune = 1), where the move is drawn, on full plies that are not drawn at temperature 0 and on every full
 * ply under AZX_ROWS_VISITS.  n_i, w_i (total_value), P_i (the stored, un-noised prior) are the root's children at
 * that time; S = sum n_i, sq = sqrtf(S), c = c_puct, n_max = max n_i, b = the first index with n_b == n_max,
 *       puct_b = (-w_b) / n_b + (c * P_b) * (sq / (1 + n_b)).
 * For each i with 0 < n_i < n_max:
 *       Q_i  = (-w_i) / n_i
 *       gap  = puct_b - Q_i                      ; if !(gap > 0): r_i = n_i
 *       f_i  = sqrtf((k * P_i) * S)
 *       need = ((c * P_i) * sq) / gap - 1        ; the smallest real n' whose PUCT does not exceed puct_b
 *       r_i  = ceilf(max(n_i - f_i, need)), clamped to [0, n_i]
 *       if r_i < n_i and r_i <= 1: r_i = 0       ; a child reduced to a single playout is pruned outright
 * Children with n_i == n_max or n_i == 0 keep their count.  The pruned counts r replace n in the weights that BOTH the
 * move draw and the row are made from (a junk forced visit is not played at T = 1 either); under AZX_ROWS_VISITS the
 * row is r_i / sum r.  At a ply drawn at temperature 0 the draw and the one-hot row cannot change (the maxima are
 * untouched); only a visit-share row differs there.  Row metrics stay on the raw counts (width, mean child visits, the
 * resign value); metric 2 is the log-probability under the distribution the move was drawn from, the pruned one.
 *   Beside the other options: early stop stays sound (a forced select still adds at most one visit to one root child);
 * resignation judges the raw root; a playout cap's fast plies neither force nor prune.
 *   It applies to azx_play, azx_play_device, azx_replay_fill and azx_play_steps (persistent k_play, per-move launches,
 * the pipelined half-pools, a registered external evaluator) and to nothing else: azx_search and the phase API select
 * by PUCT whatever the option is, and azx_match_play / azx_tournament_play refuse an engine with the option set with
 * AZX_EINVAL before touching any engine.
 *   k must be finite and in [0, 64], prune 0 or 1; (0, 0) is off; k == 0 with prune == 1 is AZX_EINVAL (the prune
 * gives back at most the forced quota).  A bad call is AZX_EINVAL and leaves the setting in place.  May be called
 * between calls, for any evaluator.  The call zeroes the statistics of azx_forced_playouts_stats.  With the option
 * never set, or cleared, every call launches the same kernels and returns the same bytes as without these entry
 * points.  azx_kernel_info reports forced=off or forced=<k>/<prune|noprune>.  What was measured is given in DESIGN
 * 7.13; the option's effect on playing strength and training efficiency is not measured.
 * Additions WITHIN ABI revision 7 (azx_version stays 7; azx_config and azx_play_stats are unchanged): callers detect
 * them by symbol (dlsym azx_set_forced_playouts). */
int azx_set_forced_playouts(azx_engine *e, float k, int prune);
int azx_get_forced_playouts(azx_engine *e, float *k, int *prune);
/* out4 = {full plies chosen under the option, selects whose forced set was non-empty, recorded rows with at least one
 * reduced child, visits removed from recorded rows}, counted since the last azx_set_forced_playouts.  They live in an
 * array of their own: azx_debug_counters keeps its 16 words. */
int azx_forced_playouts_stats(azx_engine *e, int64_t out4[4]);

/* Gumbel root search with sequential halving, for throughput self-play (Danihelka et al. 2022, "Policy improvement by
 * planning with Gumbel"; the paper was not at hand: THIS text is the definition, and it names its two deviations).
 * NOT the reference's behaviour (off by default, outside every parity claim): the reference draws and records from PUCT
 * visit counts under per-select Dirichlet noise, which carry a policy improvement only at a few hundred simulations per
 * move.  Under the option m root candidates are sampled without replacement with Gumbel noise, the simulations are
 * divided among them by sequential halving, the final survivor is played and the recorded row is the policy improved
 * by the completed Q-values: a move and a row that are sound at 32-100 simulations.
 *   All float32 arithmetic is unfused, with IEEE divide; counts are integers held in float32.  j = a root child by
 * index; n_j, w_j, P_j = its num_visits, total_value and stored, un-noised prior; k = the number of root children;
 * NBt = the select batches of this ply's search (simulations / search_batch_size + 1 on a full ply, the playout cap's
 * fast batch count on a fast ply); bs = search_batch_size.
 *   1. Noise.  r = Philox4x32-10(key of the game's uid).gen(0x47554D42, ply, j >> 2, 0x4E4F4953),
 * u = ((r[j & 3] >> 8) + 1/2) / 2^24, g_j = -ln(-ln u).  azx_gumbel_variate is this function in double precision; the
 * device computes a float32 with accurate logarithms (not the fast intrinsics; for the upper half of the 24-bit values,
 * where u is no float32, -ln u is -log1pf(-(1 - u)) of the exact complement), once per ply and child, not per select.
 * On a greedy ply (ply >= exploration_depth, or temperature == 0) g_j = 0 for all j.  Temperatures other than 0 and 1
 * are ignored under the option.
 *   2. No Dirichlet noise is mixed into any select of a search made under the option, whatever noise_scale is.
 *   3. Candidates, chosen at the top of batch 0 (the root is expanded, nothing is pending): m0 = min(m, k); the m0
 * children with the largest a_j = g_j + ln P_j, ties to the lower index.  R = max(1, ceil(log2 m0)) phases.
 *   4. Halving, at the top of batch b = 0 .. NBt-1, before its first select (the earlier batches backed up, their
 * virtual losses undone): the survivor set S is halved once for every r in 1..R-1 with floor(r * NBt / R) == b
 * (several times at one b, b = 0 included, when NBt < R).  A halving keeps the ceil(|S| / 2) survivors with the largest
 * key_j = a_j + sigma_j, ties to the lower index, where
 *       sigma_j = ((c_visit + n_max) * c_scale) * qh_j,          n_max = max of n_j over ALL root children,
 *       qh_j    = 0.5 * ((-w_j) / n_j) + 0.5 where n_j > 0, else vh,
 *       vh      = (sum over n_j > 0 of P_j * qh_j) / (sum over n_j > 0 of P_j), 0.5 when no child is visited.
 * DEVIATION 1: vh is the paper's v_mix without the root's own network value, which the reference's tree discards
 * (mcts.py:18-27).
 *   5. The root level of every select of that search descends into the survivor with the smallest n_j as that select
 * sees it (virtual losses of the batch in flight included), ties to the lower index.  Below the root PUCT stays as it
 * is, and so do virtual loss, dedup, expand and backup.  DEVIATION 2: this is root-only Gumbel; the paper's
 * deterministic interior rule is not built.
 *   6. The move: at the end of the search the survivor with the largest key_j, ties to the lower index.  Resignation
 * judges the raw root as before.
 *   7. The row of a recorded ply: with improved_rows = 1, pi_j = softmax_j(ln P_j + sigma_j) over ALL children (the
 * maximum subtracted first); with improved_rows = 0 what the engine records otherwise from the visit counts (the
 * reference's row, or AZX_ROWS_VISITS) -- a diagnostic and test mode, the row's maximum need not be the played move.
 * value_mix works as always.  Row metric 2 is ln pi_chosen under the option, in either rows mode; metrics 0, 1 and
 * 3..7 are unchanged.
 *   8. Beside the playout cap: fast plies search under the option over their own NBt and record nothing.
 *   9. It applies to azx_play, azx_play_device, azx_replay_fill and azx_play_steps (persistent k_play, per-move
 * launches, the generic instantiation, the pipelined half-pools, a registered external evaluator) and to nothing else:
 * azx_search and the phase API read "off", and azx_match_play / azx_tournament_play refuse an engine with the option
 * set with AZX_EINVAL before touching any engine.
 *   m == 0 is off; otherwise 2 <= m <= 64, c_visit finite in [0, 1e4], c_scale finite in (0, 100], improved_rows 0 or
 * 1.  A bad call is AZX_EINVAL and leaves the setting in place.  It is AZX_EINVAL while forced playouts or early stop
 * is set on the engine, and azx_set_forced_playouts / azx_set_early_stop refuse values other than off while this
 * option is on: both are rules about PUCT visit leaders.  May be called between calls, for any evaluator; the call
 * zeroes the statistics of azx_gumbel_stats.  With the option never set, or cleared, every call launches the same
 * kernels and returns the same bytes as without these entry points.  azx_kernel_info reports gumbel=off or
 * gumbel=<m>/<c_visit>/<c_scale>/<rows|norows>.  DESIGN 7.14 has what was measured; the option's effect on playing
 * strength and training efficiency is NOT measured.
 * Additions WITHIN ABI revision 7 (azx_version stays 7; azx_config and azx_play_stats are unchanged): callers detect
 * them by symbol (dlsym azx_set_gumbel). */
int azx_set_gumbel(azx_engine *e, int m, float c_visit, float c_scale, int improved_rows);
int azx_get_gumbel(azx_engine *e, int *m, float *c_visit, float *c_scale, int *improved_rows);
/* out4 = {plies chosen under the option, halvings performed, root selects made under the option, rows recorded as the
 * improved policy}, counted since the last azx_set_gumbel.  They live in an array of their own: azx_debug_counters keeps
 * its 16 words. */
int azx_gumbel_stats(azx_engine *e, int64_t out4[4]);
/* g_j of rule 1 for (the engine's seed, the game's uid, the ply from the empty board, the child index), in double
 * precision: the definition of the noise, as azx_playout_cap_is_full is of the cap's draw.  A host function.
 * AZX_EINVAL for a negative ply or a child outside [0, AZX_CELL_STRIDE). */
int azx_gumbel_variate(uint64_t seed, int64_t uid, int ply, int child, double *g);
/* self-test (tests): the device's float32 g of n raw Philox words, by the function the tree kernels use. */
int azx_selftest_gumbel(int device, int n, const uint32_t *words, float *g_out);
/* candidates, survivors: [n_games][3] words each, bit c & 63 of word c >> 6 for child index c -- the m0 candidates
 * chosen at the top of each slot's last searched ply and the survivors left at its end.  Blocking; meant for tests. */
int azx_gumbel_state(azx_engine *e, uint64_t *candidates, uint64_t *survivors);

/* float32 arithmetic self-test (tests): the tree kernels need IEEE-rounded sqrt and divide and
 * no FMA contraction (mcts.py:132-135).  sq=sqrtf(a), dv=a/(1+b), mul=(0.75f*a)*b+a. */
int azx_selftest_arith(int device, int n, const float *a, const float *b, float *sq, float *dv,
                       float *mul);

/* self-test of the two shortcuts in the search kernel's score path (mcts.py:132-134): quot[i] =
 * num[i]/den[i] through its unscaled reciprocal-refine divide, and sqrt_tab[i] = the constant-memory
 * sqrt table entry of the integer den[i] (0 beyond the table).  Both must equal the IEEE results
 * for den in [1, 2^24] and num 0 or 2^-100 <= |num| <= 2^100. */
int azx_selftest_divide(int device, int n, const float *num, const float *den, float *quot,
                        float *sqrt_tab);

/* throughput mode draws its Dirichlet noise on the device (mcts.py:128 uses numpy): n_rows
 * draws of Dirichlet(alpha * 1_k), k <= 128, exactly as the search kernel generates them, for
 * distribution tests. */
int azx_selftest_dirichlet(int device, double alpha, int k, int n_rows, uint32_t seed, float *out);

/* throughput mode's move draw on its own (tests): runs the device stand-in for as_distribution +
 * rng.multinomial (search_tree.py:327-344, policy.py:142-160) on every active slot's CURRENT root
 * statistics (call azx_search first) and returns the child index it drew, move_id[n_games] (-1: no draw),
 * and the moves_prob row it recorded for the replay, moves_prob[n_games][cells] dense by child index.
 * The slots are left with that row appended and the move pending: azx_reset them afterwards. */
int azx_debug_choose(azx_engine *e, int32_t *move_id, float *moves_prob);

/* raw device counters (16 x u64) since engine creation: selects, sum_depth, sum_k_interior,
 * sum_k_leaf, evals, terminal evals, games, errors, plies, rows, then diagnostic slots */
int azx_debug_counters(azx_engine *e, uint64_t *out16);
/* the same counters per game slot, not summed: out[n_games][16] (diagnostics: load balance) */
int azx_debug_counters_raw(azx_engine *e, uint64_t *out, int64_t n_games);
/* tests, read-only: out[n_games] = 1 for every slot whose scores are computed with the IEEE divide, 0 while the slot is on
 * the unscaled divide.  A slot switches when a value reaches its tree that is neither 0 nor 2^-60 <= |v| <= 1e30 (an
 * evaluation applied to it, its root's own included) and stays switched through moves, subtree reuse and arena
 * compaction; only azx_reset of that slot switches it back.  Both divides give the same bits, so this changes no
 * result: it tells a test which copy of the score arithmetic ran.  Always 0 with the inline evaluators
 * (AZX_EVAL_UNIFORM, AZX_EVAL_UNIFORM_HASH), whose values are 0, -1 or multiples of 2^-15.  Blocking.
 * An addition WITHIN ABI revision 7: callers detect it by symbol (dlsym azx_debug_slow_div). */
int azx_debug_slow_div(azx_engine *e, int32_t *out);

/* Which kernels this engine launches, as one line of text ("tree=... play=... tower=... heads=..."): the
 * diagnostic switches AZX_MCTS_GENERIC / AZX_NO_PERSISTENT / AZX_TOWER /
 * AZX_WIDE_STREAMS are read ONCE, by azx_create, into the engine; this reports what they selected so a run
 * can prove which kernels it used.  Returns the length of the full text (it is truncated to cap - 1 bytes). */
int azx_kernel_info(azx_engine *e, char *buf, int cap);
/* tests: bound the harvest queue of the following azx_play* calls to `rows` rows (0 = no bound) so that finished
 * games find it full and park (parallel_player.py has no counterpart: its pipes block instead). */
int azx_debug_set_queue_cap(azx_engine *e, int64_t rows);
/* tests: the staggered start of the pipelined play loop (AZX_PIPELINE_STAGGER) since engine creation.
 * out4[0] = rows the last second sub-launch evaluated, [1] = rows that were queued for that evaluation, [2] = staggered
 * moves so far, [3] = those whose second sub-launch found no row to evaluate.  All 0 before the first pipelined play.
 * An addition WITHIN ABI revision 7: callers detect it by symbol (dlsym azx_debug_stagger). */
int azx_debug_stagger(azx_engine *e, int32_t *out4);
/* tests, host only (no engine, no GPU): the position-tile map of the fused split-f16 tower k_tower_f16x3_s16 for a
 * board size 2..11.  map = "edge" (the default of AZX_TOWER_TILES, read once per network like AZX_TOWER) or
 * "rows".  rows256[64 * wave + 16 * slot + tile row] = the row 128 * board + cell of the block's two-board LDS image
 * (cell >= board_size^2: a dead row); skip4[wave] = the taps (bit 3 * (dy + 1) + dx + 1) the wave does not compute for
 * its tile in slot *light_slot, each of them padding for all 16 rows of that tile.  Returns 1 when the edge map exists
 * for the size, 0 when the map is `rows` (always for "rows"), AZX_EINVAL otherwise.  azx_kernel_info names the map an
 * engine runs (AZX_TOWER_TILES=edge|rows; engines on another tower report the setting, which they do not use).  Results do not depend on the map, bit for bit.
 * An addition WITHIN ABI revision 7: callers detect it by symbol (dlsym azx_debug_tower_tiles). */
int azx_debug_tower_tiles(int board_size, const char *map, uint8_t *rows256, uint32_t *skip4, int32_t *light_slot);
/* tests, host only (no engine, no GPU): which tower and heads kernels azx_create would give an AZX_EVAL_RESNET engine
 * of this shape and these flags (AZX_FLAG_TOWER_F16 is the one that matters) under the switches AZX_TOWER, AZX_HEADS,
 * AZX_TOWER_TILES, AZX_WIDE_STREAMS and AZX_PACK as the environment holds them now.  Writes the text of azx_kernel_info's
 * `net=` field for that engine to buf (truncated to cap - 1 bytes) and returns its full length; where azx_create would
 * refuse the network, returns its error code (AZX_EINVAL: the shape, or AZX_FLAG_TOWER_F16 on a shape without a plain-f16
 * tower or against AZX_TOWER=fp32) with its message in azx_last_error.  The engine and this call build the text with
 * the same code.
 * An addition WITHIN ABI revision 7: callers detect it by symbol (dlsym azx_debug_tower_choice). */
int azx_debug_tower_choice(int board_size, int num_blocks, int base_chans, int flags, char *buf, int cap);

/* ---- evaluation matches between two engines, entirely on the device -------------------------
 * An addition WITHIN ABI revision 7 (azx_version stays 7): callers detect it by symbol (dlsym azx_match_create).
 * Replaces, in throughput form, the reference's tournament games (azalea/evaluation.py:17-80 -> play_game.py ->
 * policy.py:132-176): two agents play each other, the mover's agent searches and draws a move, EVERY agent then
 * follows that move in its own search tree (play_game.py calls each agent's execute_action; search_tree.py:115-132).
 * A match joins two existing engines, one per agent: slot g of engine a and slot g of engine b are the two agents'
 * trees of the same game.  The engines must be on the same device with the same board_size and the same n_games
 * (= G slots), a != b, evaluator AZX_EVAL_RESNET (weights set), AZX_EVAL_UNIFORM, AZX_EVAL_UNIFORM_HASH, or
 * AZX_EVAL_EXTERNAL with an evaluator registered (azx_set_external_evaluator), in any combination -- anything else
 * is AZX_EINVAL (an AZX_EVAL_EXTERNAL engine with no evaluator registered among them).  If the evaluator has been
 * unregistered by the time of azx_match_play, that call fails with AZX_ESTATE before it touches either engine; so
 * does a match with an engine whose earlier external evaluation failed, until all its slots have been azx_reset.
 * Everything else may differ per agent:
 * simulations, search batch, c_puct, temperature, exploration depth, noise, seed, nodes_per_game, network shape.
 * The engines must outlive the match; while azx_match_play runs both belong to the calling thread.
 *
 * azx_match_play plays exactly the games u = first_game .. first_game + n_games - 1, each to its end: slot g starts
 * with game first_game + g, a slot whose game has ended takes the lowest game index not yet started, and goes idle
 * when none is left (n_games may be smaller or much larger than G).  Game u:
 *   - agent u & 1 moves first (colour 1).  DEVIATION: the reference flips a coin per game (evaluation.py:70-72);
 *     alternating has the same expectation and no variance in the colour balance.
 *   - at every ply only the mover's engine searches the slot, with ITS OWN configuration, and draws the move on the
 *     device exactly as throughput-mode self-play does (azx_play: temperature while ply < exploration_depth, then
 *     the most-visited child; noise at every ply when noise_scale != 0 -- policy.py:142-160); then BOTH engines step
 *     the game and move their trees to that child (same board, same ascending legal list, same move_id).
 *   - both engines use uid = u for game u: every draw of the game depends on (that engine's seed, u, ply) only, not
 *     on the slot, on G or on the games in flight beside it.  The same games come out of any pool size.
 *   - outcome +1: agent 0 (engine a) won; -1: agent 1 won; 0: voided.  Hex has no draws.
 *   - SearchTreeFull (azx_get_status) in the searching engine voids the game: outcome 0, length = the plies played
 *     so far, the slot takes the next game; the call goes on and returns AZX_OK.
 * Outputs, indexed by u - first_game, any may be NULL: outcome[n_games], length[n_games] (plies),
 * moves[n_games][cells] (tile + 1 in play order, 0-padded: the game record).
 * The call resets all slots of both engines at entry and leaves them as azx_reset leaves them (fresh games, all
 * active, the engine's own uid numbering); it writes no replay rows to the harvest queue unless azx_match_set_harvest
 * turned that on (below), and empties both engines' queues either way.  It blocks.  Per ply the
 * host reads back one counter; nothing it transfers grows with G.  a's searches run on a's stream and b's on b's,
 * concurrently.  A call that fails (AZX_EHIP, AZX_ERANGE, ...) leaves the engines where the failure found them:
 * azx_reset both before using them again.
 *
 * An engine with a registered evaluator takes the host at each of its simulations / search_batch_size + 1 evaluation
 * points per search: fn gets the pending rows of the slots in which that engine is the mover only (about
 * G / 2 * search_batch_size rows at most times), in (slot, leaf) order, on that engine's stream.  Per ply the host
 * first enqueues whatever needs no host (the whole search and draw of a device-evaluated engine), then advances the
 * external engines point by point in turn, so that each engine's next tree phase is on its stream before the host
 * waits for the other's rows; host syncs per ply = the external engines' evaluation points + 1.  The games do not
 * depend on that order, nor on G.  AZX_MATCH_INTERLEAVE=0 in the environment at azx_match_create selects the plain
 * order (a's whole search, then b's): a diagnostic.  A non-zero return of fn or a row that fails the checks fails
 * the call with AZX_EEXTERNAL before the next ply's searches are enqueued (the message names engine a or b, and the
 * first bad row); the error word of a search's last hand-over comes with the per-ply read-back.  The failing engine
 * then refuses search, play and match calls with AZX_ESTATE until all its slots have been azx_reset. */
typedef struct {
    int64_t games;              /* games decided (= n_games) */
    int64_t wins[2];            /* by agent: 0 = engine a, 1 = engine b */
    int64_t first_player_wins;
    int64_t voided;             /* SearchTreeFull in the searching agent's tree: outcome 0 */
    int64_t plies;              /* moves played over all games */
    double  seconds;            /* device time of the call */
} azx_match_stats;
typedef struct azx_match azx_match;
int azx_match_create(azx_engine *a, azx_engine *b, azx_match **out);
void azx_match_destroy(azx_match *m);
int azx_match_play(azx_match *m, int64_t first_game, int64_t n_games, int8_t *outcome, int16_t *length,
                   int16_t *moves, azx_match_stats *stats);

/* ---- replay rows from matches (data-collecting games between two agents) --------------------------------------
 * Additions WITHIN ABI revision 7 (azx_version stays 7): callers detect them by symbol (dlsym azx_match_set_harvest).
 * The reference's play_game(agents, collect_data=True) records a replay row at every ply from whichever agent moves
 * (play_game.py:29-67, :81-98).  Every engine's move draw already writes that row (pre-move board, moves_prob, legal
 * count, search metrics) into its own slot; with harvesting on, the step that settles a WON game copies the game's
 * rows -- row p from the engine that moved at ply p -- into the harvest queue of one engine, where they are what
 * throughput self-play leaves there: azx_rows_read, azx_rows_pack, azx_play_row_metrics (metric 3 flags a game's
 * first row) and, through records, azx_replay_put_records consume them.  color = p & 1, reward = +1 / -1 for the
 * winner's / loser's rows (play_game.py:64-65), game_uid = u.  A voided game leaves no rows (parallel_player.py:73-76).
 * Row order: games in the order their settling steps reserved queue space (NOT by u: it depends on the pool size and
 * on the scheduling of a ply's waves), a game's rows contiguous with plies ascending.
 *   azx_match_set_harvest(m, on)        the following azx_match_play calls harvest into engine a's queue (on != 0)
 *   azx_match_set_first_mover(m, mode)  -1 (default): agent u & 1 moves first in game u; 0 / 1: that agent moves first
 *                                       in EVERY game, as play_game always starts with agents[0] (play_game.py:47);
 *                                       anything else is AZX_EINVAL.  Independent of harvesting; first_player_wins
 *                                       keeps counting colour 1's wins.
 *   azx_match_rows(m, rows_out)         rows the last azx_match_play harvested (0 with harvesting off)
 * A harvesting call sizes the queue for the worst case, n_games * cells rows (a game has at most `cells` plies; the
 * queue is no ring and nothing is parked): a row takes 192 + 768 + 4 + 4 + 4 + 8 + 32 = 1012 bytes of device memory,
 * so 16384 games of 11x11 reserve about 2.0 GB, kept by the engine until azx_destroy.  AZX_ENOMEM (the message names
 * the bytes) when that cannot be had.  The rows stay readable until engine a's next play, match or tournament call.
 * Rows are never dropped silently: should a game's rows not fit, or the two engines' row counts not add up to the
 * game, the call fails with AZX_ESTATE after the games have been played.
 * Note what EVERY match and tournament call, harvesting or not, does to the queues of all its engines: it empties them
 * (rows a previous azx_play_device left there are no longer readable afterwards).  With harvesting off a call enqueues
 * the same work and returns the same bytes as before these entry points existed. */
int azx_match_set_harvest(azx_match *m, int on);
int azx_match_set_first_mover(azx_match *m, int mode);
int azx_match_rows(azx_match *m, int64_t *rows_out);

/* ---- tournaments: several matches side by side in one ply loop, sharing engines ----------------------------------
 * An addition WITHIN ABI revision 7 (azx_version stays 7): callers detect it by symbol (dlsym azx_tournament_create).
 * The reference hands every round's pairs to its pool at once (azalea/evaluation.py:29-58).  A tournament joins
 * n_engines >= 2 existing engines; azx_tournament_play then plays a list of n_pairs pairs of them -- a round robin, a
 * gauntlet of one candidate against N others, any list without a repeated pair -- as n_pairs matches that share ONE
 * ply loop.  A small match is latency-bound (a ply costs about simulations / search_batch_size + 1 dependent tree ->
 * tower -> heads rounds however few rows they carry); here each engine searches the slots of ALL its pairs together,
 * one leaf batch per engine per evaluation point, and the K engines' searches run side by side on their own streams.
 * azx_tournament_create checks what azx_match_create checks -- same device, same board_size, evaluator ready, no engine
 * given twice (AZX_EINVAL) -- but NOT equal n_games: every engine needs room for its own pairs only.
 *
 * Layout: every pair gets tables_per_pair tables; a table plays one game of its pair at a time and refills from that
 * pair's own round counter.  An engine's pool is partitioned among its opponents: engine i, in d_i pairs, uses slots
 * 0 .. d_i * tables_per_pair - 1 -- the table `l` of its r-th pair (in list order) is its slot r * tables_per_pair + l
 * -- and its other slots stay idle (never searched).  The two slots of a table generally have different indices.
 *
 * Games: round r of pair s = (pair_a[s], pair_b[s]) is game u = first_game + s * rounds + r; both engines use uid = u;
 * engine pair_a[s] is agent 0 of the rules under azx_match_play above (agent u & 1 moves first, outcome +1 = agent 0
 * won, SearchTreeFull in the searching engine voids the game).  So pair s plays, bit for bit, the games of
 * azx_match_play(match of its two engines, first_game + s * rounds, rounds): they depend neither on tables_per_pair,
 * nor on the other pairs, nor on how many slots the engines have.
 * Outputs, indexed by u - first_game = s * rounds + r, any may be NULL: outcome[n_pairs * rounds],
 * length[n_pairs * rounds], moves[n_pairs * rounds][cells]; stats[n_pairs], per pair as azx_match_stats (wins[0] =
 * engine pair_a[s]), except that `seconds` is the whole call's device time in every entry.
 * AZX_EINVAL: a pair with a == b, a pair that repeats (in either order), an index out of range, rounds < 1,
 * tables_per_pair < 1, or an engine whose n_games < d_i * tables_per_pair (the message names the engine and both
 * numbers).  AZX_ESTATE as for azx_match_play (evaluator unregistered since, an earlier external failure).
 * The call resets all slots of all engines at entry and leaves them as azx_reset leaves them; it writes no replay
 * rows unless azx_tournament_set_harvest turned that on (below).  It blocks.  Per ply the host reads back one counter (the games decided over all pairs), plus the info words
 * of each engine with a registered evaluator; nothing it transfers grows with the slot count.  Engines with a
 * registered evaluator take part as in a match: per ply the host first enqueues every device-evaluated engine's whole
 * search and draw, then advances all external engines' searches point by point in turn.  A failure of an evaluator
 * fails the call with AZX_EEXTERNAL (the message names the engine's index); that engine then refuses search, play,
 * match and tournament calls until all its slots have been azx_reset.  The engines must outlive the tournament;
 * while azx_tournament_play runs they all belong to the calling thread. */
typedef struct azx_tournament azx_tournament;
int azx_tournament_create(azx_engine *const *engines, int n_engines, azx_tournament **out);
void azx_tournament_destroy(azx_tournament *t);
int azx_tournament_play(azx_tournament *t, int n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                        int64_t first_game, int64_t rounds, int32_t tables_per_pair,
                        int8_t *outcome, int16_t *length, int16_t *moves, azx_match_stats *stats);
/* Replay rows from a tournament, as from a match (see azx_match_set_harvest above; detected by symbol alike):
 * sink_engine is the index of the engine whose harvest queue takes the rows of ALL pairs (-1 = off, the default; any
 * other value out of range is AZX_EINVAL); the queue is sized for n_pairs * rounds * cells rows.  The rows of pair s
 * are those with game_uid in [first_game + s * rounds, first_game + (s + 1) * rounds): bit for bit the rows of the
 * harvesting match of its two engines, whichever engine is the sink.  azx_tournament_set_first_mover: as for a match. */
int azx_tournament_set_harvest(azx_tournament *t, int sink_engine);
int azx_tournament_set_first_mover(azx_tournament *t, int mode);
int azx_tournament_rows(azx_tournament *t, int64_t *rows_out);

/* ---- opening books: matches and tournaments from a set of opening positions ---------------------------------------
 * Additions WITHIN ABI revision 7 (azx_version stays 7): callers detect them by symbol (dlsym azx_match_set_openings).
 * NOT in the reference: its evaluation games all start from game.reset() (play_game.py:44-47).  Two greedy agents
 * (move_sampling off: no noise, temperature 0) then play nearly the same two games over and over, and the empty Hex
 * board favours the first mover.  With a book every game starts from a given short move sequence instead, and every
 * opening is played with the colours both ways round.  Opt-in and off by default.
 *
 * Opening format: moves[o * stride + p] is the p-th move of opening o as tile + 1, in play order -- a row of a game
 * record (azx_match_play's `moves`), so a record's prefix can be fed back; colour 1 plays the even plies.  lengths[o]
 * moves count, 0 <= lengths[o] <= stride; 0 is the empty board.
 *   azx_openings_check(board_size, n_openings, stride, moves, lengths, bad_opening, bad_ply)
 *       host only (no device call).  AZX_OK when board_size is in [2, AZX_MAX_BOARD], every length is in [0, stride],
 *       every move is in 1 .. cells, no opening plays a tile twice, and the game is UNDECIDED after every move of every
 *       opening (a won position cannot be searched; an undecided one always has a legal move).  Else AZX_EINVAL:
 *       azx_last_error names the opening, the ply and the reason, and *bad_opening / *bad_ply (either may be NULL)
 *       receive the first offending opening and ply (ply = -1 for a bad length).  Both are untouched on success.
 *       n_openings in [0, 1 << 20]; the tables may be NULL only when n_openings == 0.
 *   azx_match_set_openings(m, n_openings, stride, moves, lengths)
 *   azx_tournament_set_openings(t, ...)
 *       check the arguments (null handle, n_openings outside [0, 1 << 20], stride < 0, null tables with n_openings > 0:
 *       AZX_EINVAL before any device work), then the book as azx_openings_check does for the handle's board size, then
 *       copy it to device memory the handle owns, until it is replaced or the handle destroyed.  n_openings == 0
 *       clears the book.  A call that fails leaves the previous book in place.
 * Which game plays which opening: with the alternating first mover (azx_match_set_first_mover -1, the default) game u
 * starts from opening (u >> 1) % n_openings, so games 2j and 2j + 1 are the same opening with the two agents' colours
 * swapped; with a fixed first mover (0 or 1) from opening u % n_openings.  The rule is keyed on the absolute game index
 * u -- not on u - first_game, the slot or the pool size -- so a tournament pair still plays, bit for bit, the games of
 * the match over its own range of u.  Colour-balanced pairs therefore need an EVEN first_game (first_game + s * rounds
 * for pair s of a tournament) and an even number of games / rounds; this is not enforced.
 * A game from an opening of length L: the stones are placed, ply = L, colour and winner as the moves leave them, both
 * engines' trees fresh over the position's cells - L legal moves -- the state azx_reset leaves for that prefix.  The
 * agent to move is first ^ (L & 1), `first` (the game's first mover under the rules above) owning the even plies;
 * draws stay keyed by (engine seed + u, ply), and the temperature gate ply < exploration_depth counts from the empty
 * board, as after azx_reset with a prefix.  Records: moves[u - first_game] begins with the L opening moves followed by
 * the played ones and length[] is the total ply count (a voided game: L + the plies played), so a record still
 * replays under the rules; azx_match_stats.plies counts only the moves searched and played (total length - L, summed).
 * Harvested rows (azx_match_set_harvest) begin at ply L: length - L rows per won game, color and reward sign from the
 * ply counted from the empty board, metric 3 on the row of ply L.
 * With no book -- never set, or cleared -- every call enqueues the same kernels and returns the same bytes as before
 * these entry points existed. */
int azx_openings_check(int board_size, int n_openings, int stride, const int16_t *moves, const int32_t *lengths,
                       int32_t *bad_opening, int32_t *bad_ply);
int azx_match_set_openings(azx_match *m, int n_openings, int stride, const int16_t *moves, const int32_t *lengths);
int azx_tournament_set_openings(azx_tournament *t, int n_openings, int stride, const int16_t *moves,
                                const int32_t *lengths);

/* ---- a weighted opening book for device self-play --------------------------------------------------------------
 * Additions WITHIN ABI revision 7 (azx_version stays 7; azx_config and azx_play_stats are unchanged): callers detect
 * them by symbol (dlsym azx_set_selfplay_openings).  NOT the reference's behaviour (its games start from game.reset()):
 * opt-in, off by default, outside every parity claim.  This block is the normative text.
 *
 * Every game the engine itself starts begins from an opening drawn from the book ON THE DEVICE, a pure function of
 * (cfg.seed, the game's uid):
 *   the word    azx_selfplay_opening_word(seed, uid): 32 bits from the game's key (the two key words of seed + uid, as
 *               the other per-game draws have them) on a stream of its own -- both key words are salted with constants
 *               used nowhere else, so the word shares no intermediate with the Dirichlet, reflection, move-draw, cap,
 *               resign-exemption or Gumbel words.  Nothing else enters: not the slot, n_games, the half-pool, the
 *               launch or the ply.
 *   the bounds  for a book of n openings with weights W[o] >= 0 (NULL: all equal), cum the float64 running sum taken
 *               left to right: ub[o] = (uint64) floor(ldexp(cum[o] / cum[n-1], 32)), and ub[n-1] is forced to 2^32.
 *               The host computes the table once (azx_selfplay_openings_bounds is that function).
 *   the draw    game u starts from the least o with word < ub[o].  A zero-weight opening is never drawn, one in first
 *               place included.  All weights zero, a negative or a non-finite weight: AZX_EINVAL.
 * azx_set_selfplay_openings(e, n_openings, stride, moves, lengths, weights)
 *     The book format and its checks are azx_openings_check's for the engine's board size, with the same messages;
 *     then the weights.  Book, bounds and tallies are copied to device memory the engine owns until they are replaced
 *     or the engine destroyed.  n_openings == 0 clears the book.  A failing call leaves the previous book in place and
 *     playing.  A successful one zeroes the statistics below.  May be called between calls, for any evaluator.
 * Which games follow the book: the restart of a slot whose game finished or was dropped (in azx_play, azx_play_device,
 * azx_replay_fill and azx_play_steps: persistent k_play, per-move launches, the pipelined half-pools, a registered
 * external evaluator, and a parked slot that rejoins), and azx_reset called WITHOUT a move table.  At the moment the
 * book is set (or cleared) every slot whose game has not begun -- no ply played, no row recorded, a bare unevaluated
 * root with no search under way, not parked -- is seated again in place, KEEPING its uid: generation 0 follows the book
 * too, and a fixed seed plays the same set of games whatever n_games and the sharding (game_index_stride / _offset)
 * are.  Games in progress finish as they are; they count in no tally.  azx_reset WITH a move table seats what it is
 * given (book index -1) for that one game: between azx_reset with a table and azx_set_selfplay_openings THE LAST CALL
 * WINS for a slot whose game has not begun; either way the slot's next game follows the book.
 * A game seated on an opening of length L is in the state azx_reset leaves for that prefix: stones placed,
 * ply = ply0 = L, colour and winner as the moves leave them, the tree fresh over cells - L moves, no resign mark.
 * Everything keyed on the ply counts from the empty board: the temperature gate, the playout-cap word, resign's min_ply,
 * the Gumbel variates, the reflection bits, the rows' colour and reward sign.  Rows cover the searched plies only
 * (length - L of a game played in full); azx_play_stats.sum_game_length and the per-opening plies count from the empty
 * board; azx_play_stats.plies counts the engine's moves only.
 * azx_selfplay_openings_slots(e, opening[n_games])
 *     per slot the book index of the game in progress, or -1 if it did not come from the installed book (no book,
 *     azx_reset with a table, or in progress when the book was last set).  The index is kept with the game when it is
 *     seated, not recomputed.
 * azx_selfplay_openings_stats(e, cap, out[cap][4])
 *     per opening {games started, games finished, finished games won by colour 1, plies of finished games counted from
 *     the empty board}, counted on the device at seating and at harvest since the book was last set.  A game dropped
 *     for SearchTreeFull counts as started only; a resigned game counts with the winner the resignation leaves.
 *     Returns the number of openings written (0 with no book), or AZX_EINVAL when cap is smaller than the book.
 * azx_selfplay_opening_word / azx_selfplay_openings_bounds are host only (no device call); bounds takes n in
 * [1, 1 << 20] and weights or NULL.
 * With the book never set, or cleared, every call enqueues the same kernels and returns the same bytes as before these
 * entry points existed.  azx_kernel_info reports book=off or book=<n>.  azx_match_play and azx_tournament_play refuse an
 * engine with a self-play book (AZX_EINVAL, before touching any engine): they have books of their own.  The effect on
 * playing strength and training efficiency is not measured. */
int azx_set_selfplay_openings(azx_engine *e, int n_openings, int stride, const int16_t *moves, const int32_t *lengths,
                              const double *weights /* NULL = uniform */);
int azx_selfplay_opening_word(uint64_t seed, int64_t uid, uint32_t *word);
int azx_selfplay_openings_bounds(int n_openings, const double *weights /* NULL = uniform */, uint64_t *ub);
int azx_selfplay_openings_slots(azx_engine *e, int32_t *opening);
int azx_selfplay_openings_stats(azx_engine *e, int64_t cap, int64_t *out /* [n][4] */);

/* ---- Rollout evaluator: a network-free MCTS opponent on the device -----------------------------------------------
 * NOT the reference's behaviour (its only network-free agent is RandomPolicy); additive, off unless asked for, and
 * outside every parity claim.  A registered rollout evaluator takes the place of an azx_eval_fn on an AZX_EVAL_EXTERNAL
 * engine: every pending position's value is the share of uniformly random playouts the mover wins, its priors are
 * uniform.  A filled Hex board has exactly one winner and further stones never undo a win, so a uniformly random
 * playout to the end is a uniformly random fill of the empty cells plus one connectivity test.
 *
 * THE DEFINITION (the kernel, azx_rollout_value and the tests' restatement are held to it bit for bit).  All
 * arithmetic is unsigned and wraps at the stated width.  The two mixers:
 *   sm(x):  x += 0x9E3779B97F4A7C15; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *           x = (x ^ (x >> 27)) * 0x94D049BB133111EB; return x ^ (x >> 31)            (64 bit)
 *   lb(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (32 bit)
 * Input: seed, a u64; N, the board size, 2..13; board[N*N], int32 in {0, 1, 2} in the first player's view as the
 *   hand-over exports it (azx_eval_fn's board_dev; mcts.py:174-181), so the side to move is colour 1.  Colour 1 wins by
 *   connecting row 0 to row N-1, colour 2 by connecting column 0 to column N-1.  The neighbours of (i, j) are (i-1, j),
 *   (i-1, j+1), (i, j-1), (i, j+1), (i+1, j-1), (i+1, j) where on the board (hex.py:192-197).  R, the number of
 *   rollouts, 1..4096.
 * Position key: H = sm(seed) ^ XOR over cells c with board[c] != 0 of sm(seed + 4*c + board[c]).
 * Rollout r (0 <= r < R): k_r = lb((u32)H ^ lb((u32)(H >> 32) + r)).  With e the number of empty cells, need =
 *   (e + 1) >> 1 (the mover places first) and rem = e, visit the empty cells in ascending index c:
 *     w = lb(k_r + c * 0x9E3779B9); the cell becomes colour 1 iff ((u64)w * rem) >> 32 < need, and then need -= 1;
 *     otherwise it becomes colour 2; then rem -= 1.
 *   This is selection sampling: exactly (e + 1) >> 1 cells become colour 1.  The rollout is a win iff colour 1 connects
 *   row 0 to row N-1 on the filled board.
 * Result: wins = the number of winning rollouts; value = (float)(2*wins - R) / (float)R, one correctly rounded f32
 *   division, in the mover's view; prior[j] = 1.0f / (float)e for each of the e legal moves.  e = 0 (a full board) is
 *   legal for the self-test and the host function -- all rollouts are then the same board; the engine never asks for a
 *   terminal position.
 * The value is a pure function of (seed, board): it does not depend on slot, call order, or how the GPU scheduled
 * anything.  So the same position gets the same estimate in every game of a match; games differ through the move draw.
 *
 * azx_set_rollout_evaluator: AZX_EVAL_EXTERNAL engines only (anything else is AZX_EINVAL); rollouts in 1..4096, 0
 *   unregisters; AZX_EINVAL on an engine created with AZX_FLAG_RANDOM_REFLECT.  It allocates the hand-over buffers as
 *   azx_set_external_evaluator does; at every evaluation point the pending rows are exported, the rollout kernel runs
 *   on them and its results are imported, all on the engine's stream, with no callback.  From then on the engine counts
 *   as "evaluator registered" everywhere that is asked (azx_search, azx_play*, azx_replay_fill, azx_match_create,
 *   azx_tournament_create).  It and azx_set_external_evaluator replace each other: the last call wins.  Registering
 *   zeroes azx_rollout_stats.  azx_kernel_info reports eval=rollout(R) while one is registered.
 * azx_rollout_value: the definition on the host in plain C++, no GPU.  AZX_EINVAL for a board size outside 2..13,
 *   rollouts outside 1..4096, a cell outside {0, 1, 2} or a null pointer.
 * azx_selftest_rollout: the kernel alone on n host boards [n][cells]: wins[n], value[n], prior[n][cells] (entry j =
 *   1/e for j < e, 0 after) and, unless NULL, fills[n][min(rollouts, 64)][cells], the filled boards (cells in {1, 2}) of
 *   the first rollouts.  Argument errors as azx_rollout_value, before any device work.
 * azx_rollout_stats: {hand-overs, rows, rollouts, rollouts won by the mover} since the evaluator was last registered.
 * Additions WITHIN ABI revision 7 (azx_version stays 7; azx_config and azx_play_stats are unchanged): callers detect
 * them by symbol (dlsym azx_set_rollout_evaluator). */
int azx_set_rollout_evaluator(azx_engine *e, int rollouts, uint64_t seed);
int azx_rollout_value(uint64_t seed, int board_size, const int32_t *board, int rollouts, int32_t *wins, float *value);
int azx_selftest_rollout(int device, int board_size, int n, const int32_t *boards, int rollouts, uint64_t seed,
                         int32_t *wins, float *value, float *prior, uint8_t *fills /* NULL or [n][min(rollouts,64)][cells] */);
int azx_rollout_stats(azx_engine *e, int64_t out4[4]);

/* ---- First-play urgency (FPU) for the PUCT search -----------------------------------------------------------------
 * NOT the reference's behaviour (an unvisited child scores with Q = 0 there: mcts.py:119-136, oracle/mcts.c:101-113,
 * and that stays the default); additive, off unless asked for, and outside every parity claim.  A property of the
 * ENGINE'S SEARCH, not a self-play option: it holds in every search the engine runs -- azx_search, the phase API,
 * throughput self-play, matches and tournaments (each engine with its own setting; they are not refused).
 *
 * THE DEFINITION (the tree kernels, azx_fpu_score and the tests' restatement are held to it bit for bit; csrc/fpu.h is
 * the one text the kernels and the host compile).  Every place that computes PUCT scores over a node's children
 * changes in exactly one term: a child with nv_j == 0.0f takes Q_j = fpu in place of -tv_j / max(nv_j, 1).  nv and tv
 * are the arrays as they stand at that select, virtual losses included; they are integer-valued, so the test is exact.
 * Everything else is untouched: U, the noise mix at the root, visited children, the first-maximum argmax, virtual
 * loss, dedup, expand, backup.
 *   AZX_FPU_ABSOLUTE:  fpu = value, in [-1, 1].
 *   AZX_FPU_REDUCTION: fpu = Qp - (r * sqrtf(mass)), every operation a separate float32 operation (no contraction,
 *     IEEE divide and square root), where
 *       Qp   = tv_p / max(nv_p, 1.0f), the node's own mean value in its mover's view (the root's evaluation is not
 *              backed up and the root takes no virtual loss, so a fresh root has Qp = 0);
 *       r    = root_reduction at the search's root, reduction at every other node;
 *       mass = (float)M * (1.0f / 16777216.0f);
 *       M    = the sum, over the node's children with nv_j > 0, of (uint32_t)(prior_prob_j * 16777216.0f) -- the
 *              STORED prior, not the noise-mixed one; an integer sum, so neither lane order nor the shape of the
 *              reduction can change a bit.  (Priors are taken to lie in [0, 1]; others are not defined here.)
 *   No clamp is applied.
 * Interactions: forced playouts still override the root argmax, and the argmax they override is computed with FPU;
 * the Gumbel root search replaces the root's selection, so root_reduction is unused there and FPU acts below the root;
 * playout cap, resignation, early stop, training targets, opening books and the random reflection are orthogonal.
 * With the option never set, or set and then set back to AZX_FPU_OFF, every output of the library is the same bytes
 * as before this addition.  Not part of this: AlphaZero's visit-dependent c(s), a root policy temperature, any change
 * of default.
 *
 * azx_set_fpu: mode AZX_FPU_OFF ignores the three parameters (they are stored as 0).  AZX_EINVAL, leaving the setting
 *   in place, for an unknown mode, a NaN parameter, |value| > 1 or a negative reduction; AZX_ESTATE while a phase-API
 *   search is in flight (between azx_search_begin and the last azx_search_step).  Zeroes azx_fpu_stats.
 * azx_fpu_stats: since the last azx_set_fpu, summed over the engine's games:
 *   [0] selects made under the option (a select that ends on a leaf already in flight in its batch counts too, so this
 *       equals the search counters' select count of the same searches);
 *   [1] node levels scored under the option at which at least one unvisited child existed;
 *   [2] selects that ended on a child with no visit (virtual losses count as visits);
 *   [3] selects whose choice differs from the OFF rule's: NOT computed -- it needs a second scoring pass at every level
 *       -- and always 0.
 * azx_fpu_score: the definition on the host for ONE node without root noise, no GPU: child_out = the index PUCT takes
 *   among k children with (nv[j], tv[j], prior[j]) at a node with (nv_p, tv_p), c_puct as a float32; is_root chooses
 *   root_reduction.  mode AZX_FPU_OFF gives the reference's choice.  AZX_EINVAL for k < 1, null pointers or parameters
 *   azx_set_fpu would refuse.
 * Additions WITHIN ABI revision 7 (azx_version stays 7; azx_config and azx_play_stats are unchanged): callers detect
 * them by symbol (dlsym azx_set_fpu). */
#define AZX_FPU_OFF       0
#define AZX_FPU_ABSOLUTE  1
#define AZX_FPU_REDUCTION 2
int azx_set_fpu(azx_engine *e, int mode, float value, float reduction, float root_reduction);
int azx_get_fpu(azx_engine *e, int *mode, float *value, float *reduction, float *root_reduction);
int azx_fpu_stats(azx_engine *e, int64_t out4[4]);
int azx_fpu_score(int mode, float value, float reduction, float root_reduction, int is_root, int k, float nv_p, float tv_p,
                  const float *nv, const float *tv, const float *prior, float c_puct, int32_t *child_out);

/* ---- Policy temperature for the search's priors ---------------------------------------------------------------------
 * NOT the reference's behaviour (the search uses the evaluator's prior row as delivered there: search_tree.py:254-274,
 * and that stays the default); additive, off unless asked for, and outside every parity claim.  Like first-play
 * urgency a property of the ENGINE'S SEARCH, not a self-play option: it holds in every search the engine runs --
 * azx_search, the phase API, throughput self-play, matches and tournaments (each engine with its own setting).
 *
 * azx_set_policy_temp(e, eighths, root_eighths): both in 1..8; (8, 8) is off, the default.  The temperature is 8 / m:
 * m = 7, 6, 5, 4 give 1.14, 1.33, 1.6, 2.  The exponent is restricted to eighths so that P^(m/8) is a product of IEEE
 * square roots, exact on the device and on the host alike (a powf or logf is not).
 *
 * THE DEFINITION (the tree kernels, azx_policy_temp_row and the tests' restatement are held to it bit for bit;
 * csrc/policy_temp.h is the one text the kernels and the host compile).  One row operation, temper(P[0..k), m):
 *   1. Each step is one float32 operation, unfused.  The square root and the divide are IEEE's.
 *   2. If m = 8, the row is returned as it is.
 *   3. GUARD.  If any P_j is not finite, is below 0 or is above 1, the row is returned as delivered.
 *   4. s1 = sqrtf(P_j), s2 = sqrtf(s1), s3 = sqrtf(s2).
 *   5. q_j is the left-to-right product of those s whose bit of m is set: bit 2 selects s1, bit 1 s2, bit 0 s3.
 *   6. Z is the sum over j of (uint32_t)(q_j * 16777216.0f), taken as an integer so that no lane order can change a bit.
 *   7. If Z == 0, the row is returned as delivered.
 *   8. Zf = (float)Z * (1.0f / 16777216.0f).
 *   9. The result is q_j / Zf.
 * The row sums stay within k * 2^-24 of 1 up to the rounding of the k divides.
 * A row the guard hands on is searched as the search of before searches it (the reference refuses a prior row with a
 * negative or NaN entry, mcts.py:211-213, and so does the registered device evaluator's hand-over; azx_put_evals does
 * not).  PUCT over non-finite priors is arithmetic on NaN and infinity, with one thing to know: below the root a node
 * whose children have no visit yet takes its first child unscored -- every score is -0 + 0 while the priors are
 * finite -- so a NaN or an infinite prior is first scored at the node's second visit.
 * Where the rule acts:
 *   AT EXPANSION.  When a node is expanded from a prior row (the network or an external evaluator), the children's
 *     stored prior_prob is temper(row over the legal cells, eighths).  Expansions with ONE TABLE PRIOR for all children
 *     are untouched -- tempering a constant row is the identity -- and so is the whole search of such an engine, the
 *     root included: the uniform and hash evaluators and the rollout evaluator run the kernels and produce the bytes of
 *     before this addition, whatever is set, and count nothing.
 *   AT THE ROOT.  The root select scores with R = temper(stored priors of the root's children, root_eighths) in place
 *     of the stored priors: the noise mix ((1 - eps) * R + eps * noise) and forced playouts' (k * Ps) * S read R.  The
 *     stored priors are not rewritten, so a carried subtree stays consistent.
 *   EVERYTHING ELSE reads the stored prior: first-play urgency's visited mass, the Gumbel root search's ln P, the
 *     recorded rows, azx_get_root, azx_tree_dump.  Under the Gumbel root search root_eighths is unused (and not counted),
 *     as first-play urgency's root_reduction is.
 * With the option never set, or set and then set back to (8, 8), every output of the library is the same bytes as
 * before this addition, from the same kernels.  Not part of this: AlphaZero's visit-dependent c(s) (with c_base near
 * 2e4 it changes c by about 0.02 at 400 simulations), any change of default.
 *
 * azx_set_policy_temp: AZX_EINVAL, leaving the setting in place, for a value outside 1..8; AZX_ESTATE while a phase-API
 *   search is in flight (between azx_search_begin and the last azx_search_step).  Zeroes azx_policy_temp_stats.
 * azx_get_policy_temp: the setting as made (also while the rollout evaluator keeps it from acting).
 * azx_policy_temp_stats: since the last azx_set_policy_temp, summed over the engine's games:
 *   [0] expansions whose row was tempered;
 *   [1] rows left as delivered by the guard or by Z == 0: expansions, and root rows (once per search, in the search's
 *       first launch that finds the root expanded);
 *   [2] searches begun whose root select scores with R (root_eighths != 8, no Gumbel root search);
 *   [3] 0.
 *   So [0] + [1] minus the root rows in [1] is the number of evaluated non-terminal positions expanded with eighths != 8.
 * azx_policy_temp_row: the definition on the host for ONE row, no GPU: p_out = temper(p_in[0..k), eighths), *tempered =
 *   1 where the row was changed by steps 4-9 and 0 where it came back as delivered (m = 8, the guard, Z == 0).  p_out
 *   may be p_in.  AZX_EINVAL for k outside 1..AZX_CELL_STRIDE, null pointers or eighths outside 1..8.
 * Additions WITHIN ABI revision 7 (azx_version stays 7; azx_config and azx_play_stats are unchanged): callers detect
 * them by symbol (dlsym azx_set_policy_temp).  azx_kernel_info gains a field at its end, "; temp=off" or "; temp=M/8,R/8". */
int azx_set_policy_temp(azx_engine *e, int eighths, int root_eighths);
int azx_get_policy_temp(azx_engine *e, int *eighths, int *root_eighths);
int azx_policy_temp_stats(azx_engine *e, int64_t out4[4]);
int azx_policy_temp_row(int eighths, int k, const float *p_in, float *p_out, int *tempered);

/* ---- the training step on the device ---------------------------------------------------------
 * Replaces policy_trainer.supervised_step(train=True) (azalea/policy_trainer.py:123-142: zero_grad, Network.run with
 * compute_loss, backward, optimizer.step) for HexNetwork (network.py:68-102, :120-152) under torch.optim.SGD
 * (momentum, weight decay): forward in TRAIN mode (BatchNorm on batch statistics, running statistics and
 * num_batches_tracked updated), the reference's loss, backward, and the SGD update written IN PLACE into the caller's
 * parameter and momentum tensors -- hand-written MFMA kernels queued on the caller's stream (the convolutions on the
 * split-f16 arithmetic of the self-play tower, fp32 accumulate, operands scaled per layer by powers of two: results
 * at fp32 accuracy whatever the magnitudes; environment AZX_TRAIN_FWD / _BWD / _WGRAD=fp32 selects exact-fp32 MFMA
 * kernels per pass).  The trainer keeps owning its tensors (PyTorch holds them); this handle owns the activations
 * and scratch.  16 / 32 / 64 channels on boards up to 11x11, and 128 / 256 channels on boards from 3x3 to 13x13 -- and
 * 64 channels on 12x12 / 13x13 -- through the
 * wide step (the self-play wide convolution kernel in its TRAIN modes for forward and backward-data, elementwise
 * BatchNorm / ReLU passes on split-f16 images); any batch (built for the reference's 128); other shapes are
 * AZX_EINVAL.  PERMANENT LIMIT of this ABI revision: 16 / 32 channels on 12x12 / 13x13 boards -- the narrow kernels
 * tile a board as 128 position rows and keep it whole in LDS beside 1024-wide head planes; 144 / 169 cells need the wide
 * step's 176-row tiling, whose convolution blocks are 64 output channels wide.  policy_trainer.train runs the stock
 * PyTorch step there (the reference's own, shape-agnostic: policy_trainer.py:123-142), correct and ~4x slower.  The
 * reference's width (64) and BASELINE's configs (6x64 on 11x11, 19x256 on 13x13) are covered on every board. */
typedef struct {
    int32_t board_size, num_blocks, base_chans;   /* policy.py:51-53 */
    int32_t batch_size;                           /* config batch_size (hex11_train_config.yml: 128) */
    int32_t device;
} azx_train_config;
typedef struct azx_trainer azx_trainer;
int azx_train_create(const azx_train_config *cfg, azx_trainer **out);
void azx_train_destroy(azx_trainer *t);
/* Every state_dict entry of the module by name (network.py:42-61, :120-132), as DEVICE pointers that stay valid and
 * are updated in place: parameters (fp32) with their SGD momentum buffers momentum[i] (fp32, same shape, zero before
 * the first step = torch's lazily created buffer), BatchNorm running_mean / running_var (fp32) and
 * num_batches_tracked (int64) with momentum[i] = NULL.  Call again after the tensors were re-allocated. */
int azx_train_bind(azx_trainer *t, int n, const char *const *names, void *const *tensors, const int64_t *counts,
                   void *const *momentum);
/* the step's static input buffers (device), row stride board_size^2, the layout azx_replay_collate writes:
 * board i32[B][cells], legal_moves i32[B][cells] (ascending tile + 1, zero padded), moves_prob f32[B][cells] (by child
 * index, zero padded), reward f32[B] */
int azx_train_inputs(azx_trainer *t, int32_t **board, int32_t **legal_moves, float **moves_prob, float **reward);
/* device buffers holding the last step's results: loss f32[3] = {total, value, moves} (network.py:92-102),
 * value f32[B], moves_logprob f32[B][cells] (entry j = log-probability of legal move j; padding as the reference's
 * -99 logits) */
int azx_train_outputs(azx_trainer *t, float **loss3, float **value, float **moves_logprob);
/* One optimizer step on the bound tensors with the inputs currently in the input buffers, enqueued on `hip_stream`
 * (a hipStream_t; NULL = the default stream) and NOT synchronised: order it after whatever filled the inputs and
 * before whatever reads the weights.  lr / momentum / weight_decay: torch.optim.SGD's (policy_trainer.py:44-49). */
int azx_train_step(azx_trainer *t, float lr, float momentum, float weight_decay, void *hip_stream);
/* tests: internal buffer by name ("raw<l>", "act<l>", "g<l>" [B][cells][C]; "sums"; "grad:<state_dict name>");
 * "flags" is three host int32: AZX_TRAIN_GRAPH on, the filter-gradient fork on (AZX_TRAIN_FORK), graph instantiated */
int azx_train_debug(azx_trainer *t, const char *name, void *out, int64_t cap, int64_t *nbytes);

/* engine stream (hipStream_t) so callers can bracket work with HIP events */
void *azx_stream(azx_engine *e);

#ifdef __cplusplus
}
#endif
#endif /* AZX_H */
