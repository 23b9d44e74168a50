// azx_capi.cpp -- host side of the C ABI declared in include/azx.h.
// Owns the device arenas, sequences the kernels on one HIP stream per engine, and converts
// between the reference's data model (six tree arrays, ragged legal-move lists) and the
// engine's HBM layout.  No CPU fallback: without a HIP device every entry point fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/azx.h"
#include "azx_dev.h"
#include "mcts_kernels.h"
#include "net.h"
#include "train.h"
#include "replay_kernels.h"
#include "ext_kernels.h"
#include "match_kernels.h"
#include "playout_cap.h"
#include "gumbel.h"
#include "fpu.h"
#include "policy_temp.h"
#include "resign.h"
#include "rollout_kernels.h"
#include "selfplay_openings.h"
#include "tower_tiles.h"

#ifndef AZX_SRC_SHA
#define AZX_SRC_SHA "unknown"      // the Makefile passes the digest of the kernel sources (profiles are keyed to it)
#endif

static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHECK(expr)                                                                    \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return fail(AZX_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),  \
                        __FILE__, __LINE__);                                              \
    } while (0)

// The self-play options as the host holds them (azx_set_playout_cap, azx_set_resign, azx_set_early_stop,
// azx_set_train_targets, azx_set_forced_playouts, azx_set_gumbel): a default-constructed value is every option off.
// e->d carries "off" except inside the throughput self-play calls (SelfplayScope).
struct SelfplayOptions {
    bool cap_on = false;
    double cap_full_prob = 1.0;
    int cap_fast_sims = 0;
    bool resign_on = false;
    double resign_thr = -1.0, resign_keep = 0.0;
    int resign_min_ply = 0;
    bool estop_on = false;
    int tt_rows = AZX_ROWS_REFERENCE;
    float tt_mix = 0.0f;
    bool tt_on() const { return tt_rows != AZX_ROWS_REFERENCE || tt_mix > 0.0f; }
    float fp_k = 0.0f;
    int fp_prune = 0;
    int gm_m = 0, gm_rows = 0;
    float gm_c_visit = 0.0f, gm_c_scale = 0.0f;

    // the option fields of a DevEngine for these settings, every one of them (so the default value writes "off")
    void write(DevEngine &d) const {
        d.cap_fast_batches = cap_on ? cap_fast_sims / d.bs + 1 : 0;      // mcts.py:268 applied to fast_simulations
        d.cap_thr_m1 = cap_on ? azx_cap_threshold_m1(cap_full_prob) : 0u;
        d.resign_mode = !resign_on ? AZX_RESIGN_OFF : resign_keep > 0.0 ? AZX_RESIGN_DRAW_EXEMPT : AZX_RESIGN_NONE_EXEMPT;
        d.resign_min_ply = resign_on ? resign_min_ply : 0;
        d.resign_thr = resign_on ? (float)resign_thr : 0.0f;
        d.resign_keep_m1 = resign_on && resign_keep > 0.0 ? azx_resign_threshold_m1(resign_keep) : 0u;
        d.early_stop = estop_on ? 1 : 0;
        d.tt_rows = tt_rows; d.tt_mix = tt_mix;
        d.fp_k = fp_k; d.fp_prune = fp_prune;
        d.gm_m = gm_m; d.gm_rows = gm_rows; d.gm_c_visit = gm_c_visit; d.gm_c_scale = gm_c_scale;
    }
};

// ---- the launch schedule of one search ---------------------------------------------------------------------
// With nb = num_batches, a search of an engine whose evaluations are launches of their own (the network, a registered
// evaluator, the phase API's caller) is the phases
//   0          k_mcts MODE_BEGIN                then an evaluation
//   1 .. nb    k_mcts MODE_APPLY | MODE_SELECT  then an evaluation
//   nb + 1     k_mcts MODE_APPLY                ends the search
// on one stream.  Every driver issues them through enqueue_tree_phase, and all but the pipelined play loop walk them
// with a SearchCursor (search_advance, further down).
struct PhaseMode { int bits; bool then_eval; };     // a tree launch's MODE_* bits; an evaluation of the leaves it queued follows
static PhaseMode phase_mode(int ph, int nb) {
    if (ph == 0) return {MODE_BEGIN, true};
    if (ph <= nb) return {MODE_APPLY | MODE_SELECT, true};
    return {MODE_APPLY, false};
}

// Where a search stands: the next phase to issue.  A cursor not yet begun is done.
struct SearchCursor {
    int next = 0, last = -1;
    bool timed = false;             // its launches go into the timing pool (the throughput calls)
    bool by_caller = false;         // the phase API's: on an AZX_EVAL_EXTERNAL engine the caller evaluates between the phases
    SearchCursor() {}
    SearchCursor(int nb, bool timed_, bool by_caller_) : last(nb + 1), timed(timed_), by_caller(by_caller_) {}
    bool done() const { return next > last; }
};

struct azx_engine {
    azx_config cfg;
    DevEngine d;
    hipStream_t stream = nullptr;
    int reserved_cus = 0;               // azx_reserve_cus: CUs of the device the engine's streams stay off
    std::mutex alloc_mu;                // dev_alloc from the trainer's thread (collate staging) beside the play thread's
    int num_batches = 0;
    int selects_per_search = 0;
    std::vector<void *> allocs;
    // gather buffers
    int32_t *g_k = nullptr, *g_legal = nullptr, *g_nn = nullptr;
    float *g_cv = nullptr, *g_cw = nullptr, *g_cp = nullptr, *g_rv = nullptr, *g_rw = nullptr,
          *g_sv = nullptr;
    double *noise_dev = nullptr;
    size_t noise_cap = 0;
    float *prior_table_dev = nullptr;
    int32_t *moveids_dev = nullptr;
    int32_t *slots_dev = nullptr, *moves_dev = nullptr, *nmoves_dev = nullptr;
    size_t moves_cap = 0;
    SearchCursor phase_api;                     // azx_search_begin / azx_search_step: their search, in flight while !done()
    // external evaluator bookkeeping
    std::vector<int> ext_order;                // eval indices sorted by (slot, leaf)
    std::vector<std::vector<int>> ext_cells;    // original legal cells per sorted entry
    // registered device evaluator (azx_set_external_evaluator): the hand-over buffers, the last host read of
    // ext.info, and the slots a failed evaluation left with half-done searches (refused until azx_reset)
    azx_eval_fn ext_fn = nullptr;
    void *ext_user = nullptr;
    ExtBufs ext = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int32_t ext_info[4] = {0, 0, AZX_EXT_NO_ERROR, 0};
    int32_t *ext_info_host = nullptr;           // pinned landing place of ext.info (a copy into it never blocks the host)
    std::vector<char> ext_dirty;
    bool ext_failed = false;
    // rollout evaluator (azx_set_rollout_evaluator): takes ext_fn's place at the evaluation points while ro_R > 0
    int ro_R = 0;
    // policy temperature as azx_set_policy_temp left it (d.pt_* are the values in force: pt_refresh)
    int pt_eighths = 8, pt_root_eighths = 8;
    uint64_t ro_seed = 0;
    int64_t ro_handovers = 0, ro_rows = 0;
    unsigned long long *ro_won = nullptr;       // device: rollouts won by the mover (one add per row)
    // play mode
    bool play_ready = false;
    int64_t q_alloc = 0;
    int64_t q_rows_valid = 0;           // rows the last azx_play_device left in the queue
    std::vector<void *> q_allocs;
    int32_t *export_board = nullptr;    // azx_play's device-side widening staging
    float *export_prob = nullptr;
    size_t export_cap = 0;
    // device-resident replay ring (azx_replay_*)
    ReplayRows ring = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int64_t ring_cap = 0, ring_size = 0, ring_write = 0;
    long long *ring_idx = nullptr;      // sampled row indices of the collate in flight
    int64_t ring_idx_cap = 0;
    int32_t *ring_maxk = nullptr;
    bool ring_mover_view = false;       // azx_replay_set_mover_view
    bool ring_reflect = false;          // azx_replay_set_reflect: its seed, and the collates (blocking + async) since
    uint64_t ring_reflect_seed = 0, ring_reflect_count = 0;
    std::vector<void *> ring_allocs;
    // azx_replay_collate_async: index staging, AZX_COLLATE_SLOTS deep (pinned host + device), one event per slot
    long long *cidx_host[8] = {nullptr}, *cidx_dev[8] = {nullptr};
    hipEvent_t cidx_ev[8] = {nullptr};
    int64_t cidx_cap = 0;
    uint64_t cidx_next = 0;
    int32_t *cidx_maxk = nullptr;
    // timing
    std::vector<hipEvent_t> ev_pool;
    std::vector<char> ev_tag;           // 0 = tree kernel, 1 = network (tower + heads), 2 = reference mark (not booked)
    std::vector<int> ev_weight;         // moves covered by the timed launch (k_play: several)
    // pipelined play: the two half-pools' launches of one phase share a group id (> 0) and count as ONE launch; their
    // time is the union of the grouped launches' spans (read against the reference mark ev_ref, recorded before them):
    // the device time during which such launches were running
    std::vector<int> ev_group, ev_ref;
    int ev_groups = 0;
    size_t ev_used = 0;
    AzxNet *net = nullptr;
    // diagnostic switches, read once at azx_create (azx_kernel_info reports them)
    bool force_generic = false;         // AZX_MCTS_GENERIC: every tree launch on the generic instantiation
    bool no_persistent = false;         // AZX_NO_PERSISTENT: per-move launches instead of k_play
    bool pipeline = true;               // AZX_PIPELINE=0: the resnet play loop on one stream (no half-pools)
    bool stagger = true;                // AZX_PIPELINE_STAGGER=0: half B's evaluations never wait for half A's
    // pipelined play: the second half-pool's stream, made on first use on the engine stream's CU mask
    hipStream_t stream_b = nullptr;
    std::vector<uint32_t> cu_mask;      // azx_reserve_cus's mask (empty = all CUs)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_stagger = nullptr;
    int32_t *stagger_ctr = nullptr;     // azx_net_eval_rows_behind's count and azx_debug_stagger's counters (4 ints)
    int64_t dbg_qcap = 0;               // azx_debug_set_queue_cap
    SelfplayOptions opt;                // what the azx_set_* of the self-play options last stored
    unsigned long long cap_base[3] = {0, 0, 0};   // CTR_CAP_* sums when the cap was last set
    // self-play opening book (azx_set_selfplay_openings): the device tables e->d.bk_* point at (the engine owns them;
    // replaced as a whole, freed by azx_destroy).  Not scoped: e->d carries the book in every launch (azx_dev.h)
    void *book_allocs[4] = {nullptr, nullptr, nullptr, nullptr};
};

// The throughput self-play calls hand their launches the engine's self-play options; every other launch of the engine
// (azx_search, the phase API, matches) reads "off" from e->d.  (The opening book is not scoped: azx_dev.h.)
struct SelfplayScope {
    DevEngine &d;
    explicit SelfplayScope(azx_engine *e) : d(e->d) { e->opt.write(d); }
    ~SelfplayScope() { SelfplayOptions().write(d); }
    SelfplayScope(const SelfplayScope &) = delete;
    SelfplayScope &operator=(const SelfplayScope &) = delete;
};

template <typename T>
static int dev_alloc(azx_engine *e, T **p, size_t count, bool zero = true) {
    void *q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    hipError_t err = hipMalloc(&q, bytes);
    if (err != hipSuccess)
        return fail(AZX_ENOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(err));
    if (zero) {
        err = hipMemsetAsync(q, 0, bytes, e->stream);
        if (err != hipSuccess) return fail(AZX_EHIP, "hipMemset failed: %s", hipGetErrorString(err));
    }
    std::lock_guard<std::mutex> lock(e->alloc_mu);
    e->allocs.push_back(q);
    *p = reinterpret_cast<T *>(q);
    return AZX_OK;
}

// Every entry point runs with the engine's device current and puts the caller's device back on
// return (hipSetDevice is per host thread and also moves torch.cuda.current_device()).
struct DevGuard {
    int prev = -1;
    bool changed = false;
    explicit DevGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DevGuard() { if (changed) (void)hipSetDevice(prev); }
    DevGuard(const DevGuard &) = delete;
    DevGuard &operator=(const DevGuard &) = delete;
};
#define ENGINE_GUARD(e) DevGuard _dev_guard((e)->cfg.device)

#define TRY(expr)            \
    do {                     \
        int _rc = (expr);    \
        if (_rc) return _rc; \
    } while (0)

extern "C" const char *azx_last_error(void) { return g_err.c_str(); }
extern "C" int azx_version(void) { return 7; }   // 7: azx_set_external_evaluator, AZX_EEXTERNAL (include/azx.h)

extern "C" int azx_create(const azx_config *cfg, azx_engine **out) {
    if (!cfg || !out) return fail(AZX_EINVAL, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(AZX_ENODEV, "no HIP device visible: the engine has no CPU fallback");
    if (cfg->board_size < 2 || cfg->board_size > AZX_MAX_BOARD)
        return fail(AZX_EINVAL, "board_size %d outside [2, %d]", cfg->board_size, AZX_MAX_BOARD);
    if (cfg->n_games < 1) return fail(AZX_EINVAL, "n_games must be >= 1");
    if (cfg->search_batch_size < 1 || cfg->search_batch_size > AZX_MAX_BATCH)
        return fail(AZX_EINVAL, "search_batch_size %d outside [1, %d]", cfg->search_batch_size,
                    AZX_MAX_BATCH);
    if (cfg->simulations < 0) return fail(AZX_EINVAL, "simulations must be >= 0");
    if (cfg->evaluator < AZX_EVAL_RESNET || cfg->evaluator > AZX_EVAL_EXTERNAL)
        return fail(AZX_EINVAL, "unknown evaluator %d", cfg->evaluator);
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(AZX_EINVAL, "device %d not in [0, %d)", cfg->device, ndev);
    if ((cfg->flags & AZX_FLAG_RANDOM_REFLECT) &&
        (cfg->evaluator == AZX_EVAL_UNIFORM || cfg->evaluator == AZX_EVAL_UNIFORM_HASH))
        return fail(AZX_EINVAL, "AZX_FLAG_RANDOM_REFLECT needs a network input to reflect: the inline evaluator %s has "
                                "none (use AZX_EVAL_RESNET or AZX_EVAL_EXTERNAL)",
                    cfg->evaluator == AZX_EVAL_UNIFORM ? "AZX_EVAL_UNIFORM" : "AZX_EVAL_UNIFORM_HASH");
    if ((cfg->flags & AZX_FLAG_TOWER_F16) && cfg->evaluator != AZX_EVAL_RESNET)     // (shape, AZX_TOWER=fp32: azx_net_create)
        return fail(AZX_EINVAL, "AZX_FLAG_TOWER_F16 selects a tower kernel of the built-in network: evaluator %d is not "
                                "AZX_EVAL_RESNET", cfg->evaluator);
    if (cfg->game_index_stride < 0 || cfg->game_index_offset < 0 ||
        cfg->game_index_offset >= std::max(1, cfg->game_index_stride))
        return fail(AZX_EINVAL, "game_index_offset %d outside [0, game_index_stride %d)", cfg->game_index_offset,
                    std::max(1, cfg->game_index_stride));
    DevGuard guard(cfg->device);
    { int cur = -1; if (hipGetDevice(&cur) != hipSuccess || cur != cfg->device) return fail(AZX_EHIP, "hipSetDevice(%d) failed", cfg->device); }
    if (azx_init_geometry(cfg->device)) return fail(AZX_EHIP, "uploading the board geometry tables failed");

    azx_engine *e = new azx_engine();
    e->cfg = *cfg;
    { const char *v = getenv("AZX_MCTS_GENERIC"); e->force_generic = v && atoi(v) != 0; }
    { const char *v = getenv("AZX_NO_PERSISTENT"); e->no_persistent = v && atoi(v) != 0; }
    { const char *v = getenv("AZX_PIPELINE"); e->pipeline = !(v && atoi(v) == 0); }
    { const char *v = getenv("AZX_PIPELINE_STAGGER"); e->stagger = !(v && atoi(v) == 0); }
    HIPCHECK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    DevEngine &d = e->d;
    memset(&d, 0, sizeof d);
    d.N = cfg->board_size;
    d.ncells = d.N * d.N;
    d.G = cfg->n_games;
    d.bs = cfg->search_batch_size;
    d.slots = d.ncells <= 128 ? 2 : 3;
    d.c_puct = cfg->exploration_coef;
    d.evaluator = cfg->evaluator;
    d.flags = cfg->flags;
    d.seed = cfg->seed;
    d.uid_stride = std::max(1, cfg->game_index_stride);
    d.uid_offset = cfg->game_index_offset;
    d.slot_base = 0;
    d.pool_games = d.G;
    d.noise_alpha = (float)cfg->noise_alpha;
    d.noise_scale = 0.0;
    d.exploration_depth = cfg->exploration_depth;
    d.temperature = (float)cfg->temperature;
    d.pt_eighths = d.pt_root_eighths = 8;
    e->num_batches = cfg->simulations / cfg->search_batch_size + 1;   // mcts.py:268
    e->selects_per_search = e->num_batches * cfg->search_batch_size;
    d.selects_per_search = e->selects_per_search;
    int cap = cfg->nodes_per_game;
    // default: six moves' worth of expansions -- a sharply peaked network carries most of its tree
    // from move to move (the reference allows 10M nodes per game, search_tree.py:18)
    if (cap <= 0) cap = 6 * (e->selects_per_search + 1) * d.ncells + 1024;
    d.cap = cap;

    const size_t G = d.G, bs = d.bs, E = G * bs;
    const size_t pstride = d.ncells + (d.ncells & 1);
    int rc = AZX_OK;
#define A(ptr, count) if (!rc) rc = dev_alloc(e, &ptr, (count))
    A(d.cells, G * d.slots * 64);
    A(d.ghdr, G);
    A(d.thdr, G);
    if (!rc) rc = dev_alloc(e, &d.arena[0], G * (size_t)cap, false);
    if (cfg->flags & AZX_FLAG_NO_COMPACT) d.arena[1] = d.arena[0];
    else if (!rc) rc = dev_alloc(e, &d.arena[1], G * (size_t)cap, false);
    A(d.leaf_node, E); A(d.leaf_len, E); A(d.leaf_eval, E); A(d.leaf_link, E); A(d.leaf_cells, E);
    A(d.leaf_mask, E * 4); A(d.path, E * pstride);
    A(d.ev_board, E * AZX_CELL_STRIDE); A(d.ev_src, E); A(d.ev_flip, E);
    A(d.ev_value, E); A(d.ev_prior, E * AZX_CELL_STRIDE); A(d.n_eval, 4);   // (n_eval[1]: the second half-pool's count)
    A(d.counters, G * CTR_COUNT); A(d.q_count, 2); A(d.stat_sums, G * 8);
    A(d.resign_ctr, G * RS_COUNT);
    A(d.estop_ctr, G * ES_COUNT);
    A(d.tt_ctr, G * TT_COUNT);
    A(d.fp_ctr, G * FP_COUNT);
    A(d.gm_ctr, G * GM_COUNT);
    A(d.fpu_ctr, G * FPU_COUNT);
    A(d.pt_ctr, G * PT_COUNT);
    A(d.gm_state, G * GM_STATE_WORDS);
    A(d.gm_g, G * 2 * AZX_CELL_STRIDE);
    A(e->g_k, G); A(e->g_legal, G * d.ncells); A(e->g_nn, G);
    A(e->g_cv, G * d.ncells); A(e->g_cw, G * d.ncells); A(e->g_cp, G * d.ncells);
    A(e->g_rv, G); A(e->g_rw, G); A(e->g_sv, G);
    A(e->moveids_dev, G); A(e->slots_dev, G); A(e->nmoves_dev, G);
#undef A
    if (rc) { azx_destroy(e); return rc; }
    if (cfg->evaluator == AZX_EVAL_RESNET) {
        rc = azx_net_create(&e->net, d.N, cfg->num_blocks, cfg->base_chans, (int)E,
                            (cfg->flags & AZX_FLAG_TOWER_F16) ? 1 : 0, e->stream);
        if (rc) { g_err = azx_net_error(); azx_destroy(e); return rc; }
    }
    {   // inverse-CDF table of the device Dirichlet sampler for this engine's alpha
        float *gt = nullptr;
        rc = dev_alloc(e, &gt, AZX_GAMMA_TAB_FLOATS);
        if (rc) { azx_destroy(e); return rc; }
        std::vector<float> tab(AZX_GAMMA_TAB_FLOATS, 0.0f);
        if (cfg->noise_alpha > 0.0) azx_gamma_table(cfg->noise_alpha, tab.data());
        if (hipMemcpyAsync(gt, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, e->stream) != hipSuccess ||
            hipStreamSynchronize(e->stream) != hipSuccess) {
            azx_destroy(e);
            return fail(AZX_EHIP, "uploading the gamma sampler table failed");
        }
        e->d.gamma_tab = gt;
    }
    *out = e;
    {   // default uniform prior table: float32 1/k, the same bits as the IEEE division on device
        std::vector<float> tab(d.ncells + 1, 0.0f);
        for (int k = 1; k <= d.ncells; ++k) tab[k] = 1.0f / (float)k;
        rc = azx_set_prior_table(e, tab.data(), d.ncells + 1);
        if (rc) { azx_destroy(e); *out = nullptr; return rc; }
        e->d.prior_default = 1;
    }
    // all slots start as fresh games with uids 0..G-1
    azx_launch_reset(d, nullptr, d.G, nullptr, nullptr, 0, 1, e->stream);
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

extern "C" void azx_destroy(azx_engine *e) {
    if (!e) return;
    ENGINE_GUARD(e);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->net) azx_net_destroy(e->net);
    for (void *p : e->allocs) (void)hipFree(p);
    for (void *p : e->q_allocs) (void)hipFree(p);
    for (void *p : e->ring_allocs) (void)hipFree(p);
    for (void *p : e->book_allocs) if (p) (void)hipFree(p);
    if (e->export_board) (void)hipFree(e->export_board);
    if (e->export_prob) (void)hipFree(e->export_prob);
    if (e->ext_info_host) (void)hipHostFree(e->ext_info_host);
    for (hipEvent_t ev : e->ev_pool) (void)hipEventDestroy(ev);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    if (e->ev_stagger) (void)hipEventDestroy(e->ev_stagger);
    if (e->stream_b) { (void)hipStreamSynchronize(e->stream_b); (void)hipStreamDestroy(e->stream_b); }
    for (int i = 0; i < 8; ++i) {
        if (e->cidx_ev[i]) { (void)hipEventSynchronize(e->cidx_ev[i]); (void)hipEventDestroy(e->cidx_ev[i]); }
        if (e->cidx_host[i]) (void)hipHostFree(e->cidx_host[i]);
        if (e->cidx_dev[i]) (void)hipFree(e->cidx_dev[i]);
    }
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

extern "C" void *azx_stream(azx_engine *e) { return e ? (void *)e->stream : nullptr; }

// CU mask layout of gfx950, measured (tools/microbench/cu_mask.hip, profiles/r6_cu_mask_microbench.txt): bit b of the
// mask is XCD b % 8, shader engine (b / 8) % 4, so bits [0, 8 r) are r CUs of every XCD, dealt one per shader engine.
extern "C" int azx_reserve_cus(azx_engine *e, int cus_per_xcd, int *reserved_out) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    hipDeviceProp_t prop;
    HIPCHECK(hipGetDeviceProperties(&prop, e->cfg.device));
    const int ncu = prop.multiProcessorCount, xcds = 8, ses = 4;
    if (cus_per_xcd < 0 || cus_per_xcd * xcds >= ncu)
        return fail(AZX_EINVAL, "cus_per_xcd %d outside [0, %d)", cus_per_xcd, ncu / xcds);
    if (cus_per_xcd > 0 && ncu % (xcds * ses))
        return fail(AZX_ESTATE, "CU reservation is laid out for 8 XCDs x 4 shader engines; this device has %d CUs", ncu);
    const int per = (cus_per_xcd + ses - 1) / ses * ses;
    const int words = (ncu + 31) / 32;
    std::vector<uint32_t> mask((size_t)words, 0u);
    for (int b = 0; b < ncu; ++b)
        if (b >= per * xcds) mask[b / 32] |= 1u << (b % 32);
    HIPCHECK(hipStreamSynchronize(e->stream));
    hipStream_t fresh = nullptr;
    if (per == 0) HIPCHECK(hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking));
    else HIPCHECK(hipExtStreamCreateWithCUMask(&fresh, (uint32_t)words, mask.data()));
    hipStream_t old = e->stream;
    e->stream = fresh;
    if (e->net) azx_net_set_stream(e->net, fresh, per ? mask.data() : nullptr, per ? words : 0);
    (void)hipStreamDestroy(old);
    if (e->stream_b) {      // the second half-pool's stream is made again, on the new mask, at its next use
        (void)hipStreamSynchronize(e->stream_b);
        (void)hipStreamDestroy(e->stream_b);
        e->stream_b = nullptr;
    }
    e->cu_mask.assign(mask.begin(), per ? mask.end() : mask.begin());
    e->reserved_cus = per * xcds;
    if (!e->cidx_maxk) TRY(dev_alloc(e, &e->cidx_maxk, 4));     // (so that the trainer's thread never allocates beside a play)
    HIPCHECK(hipStreamSynchronize(e->stream));
    if (reserved_out) *reserved_out = e->reserved_cus;
    return AZX_OK;
}

// ---- pipelined play: two half-pools -----------------------------------------------------------
// The resnet play loop can run the pool as two halves, slots [0, G/2) and [G/2, G), each on its own stream: one
// half's search phases and its tower launches' ramp and tail overlap the other half's tower.  The games
// are independent (the device RNG is keyed by the global game index, each tower row depends on its own board alone),
// so the halves compute what the one-stream loop computes.
static bool use_pipeline(const azx_engine *e) {
    return e->pipeline && e->d.evaluator == AZX_EVAL_RESNET && e->d.G % 2 == 0 && e->d.G >= 1024 &&
           azx_net_rows_splittable(e->net);
}

// DevEngine over slots [base, base + n): every per-slot array offset by `base` slots, the evaluation queue the
// matching part of ev_* with its own count `n_eval`; the pool-wide harvest queue (q_*, q_count) stays shared
static DevEngine pool_view(const DevEngine &d, int base, int n, int32_t *n_eval) {
    DevEngine v = d;
    const size_t b = (size_t)base, bs = (size_t)d.bs, nc = (size_t)d.ncells, pstride = nc + (nc & 1);
    v.G = n;
    v.slot_base = d.slot_base + base;
    v.cells += b * d.slots * 64;
    v.ghdr += b;
    v.thdr += b;
    v.arena[0] += b * d.cap;
    v.arena[1] += b * d.cap;
    v.leaf_node += b * bs; v.leaf_len += b * bs; v.leaf_eval += b * bs; v.leaf_link += b * bs; v.leaf_cells += b * bs;
    v.leaf_mask += b * bs * 4;
    v.path += b * bs * pstride;
    v.ev_board += b * bs * AZX_CELL_STRIDE;
    v.ev_src += b * bs;
    v.ev_flip += b * bs;
    v.ev_value += b * bs;
    v.ev_prior += b * bs * AZX_CELL_STRIDE;
    v.n_eval = n_eval;
    if (v.noise) v.noise += b * d.n_select * d.noise_stride;
    v.counters += b * CTR_COUNT;
    v.stat_sums += b * 8;
    v.resign_ctr += b * RS_COUNT;
    v.estop_ctr += b * ES_COUNT;
    v.tt_ctr += b * TT_COUNT;
    v.fp_ctr += b * FP_COUNT;
    v.gm_ctr += b * GM_COUNT;
    v.fpu_ctr += b * FPU_COUNT;
    v.pt_ctr += b * PT_COUNT;
    v.gm_state += b * GM_STATE_WORDS;
    v.gm_g += b * 2 * AZX_CELL_STRIDE;
    if (v.row_board) v.row_board += b * nc * AZX_CELL_STRIDE;
    if (v.row_prob) v.row_prob += b * nc * AZX_CELL_STRIDE;
    if (v.row_k) v.row_k += b * nc;
    if (v.row_meta) v.row_meta += b * nc * AZX_ROW_METRICS;
    return v;
}

static int pipeline_streams(azx_engine *e) {
    if (!e->stream_b) {
        if (e->cu_mask.empty()) HIPCHECK(hipStreamCreateWithFlags(&e->stream_b, hipStreamNonBlocking));
        else HIPCHECK(hipExtStreamCreateWithCUMask(&e->stream_b, (uint32_t)e->cu_mask.size(), e->cu_mask.data()));
    }
    if (!e->ev_fork) HIPCHECK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    if (!e->ev_join) HIPCHECK(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
    if (!e->ev_stagger) HIPCHECK(hipEventCreateWithFlags(&e->ev_stagger, hipEventDisableTiming));
    if (!e->stagger_ctr) TRY(dev_alloc(e, &e->stagger_ctr, 4));     // (zeroed on the engine stream, where half A uses it)
    return AZX_OK;
}

// ---- the self-play options as the host describes them, in the order azx_kernel_info lists them and matches refuse them ----
static std::string strf(const char *fmt, ...) {
    char t[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t, sizeof t, fmt, ap);
    va_end(ap);
    return t;
}

struct OptionInfo {
    const char *field;                          // azx_kernel_info: " <field>=<text>", "off" while the option is not set
    bool (*is_set)(const azx_engine *);
    std::string (*text)(const azx_engine *);
    const char *noun;                           // a refusal: "engine <i> has <noun> set: <reason> (<clear>)",
    const char *reason;                         // ... {} standing for "match" / "tournament" in both clauses
    const char *clear;
};

static const OptionInfo SELFPLAY_OPTIONS[] = {
    {"cap", [](const azx_engine *e) { return e->opt.cap_on; },
     [](const azx_engine *e) { return strf("%.6g/%d", e->opt.cap_full_prob, e->opt.cap_fast_sims); },
     "a playout cap", "a {} records one row per moved ply", "clear it with azx_set_playout_cap(e, 1.0, 0)"},
    {"resign", [](const azx_engine *e) { return e->opt.resign_on; },
     [](const azx_engine *e) { return strf("%.6g/%d/%.6g", e->opt.resign_thr, e->opt.resign_min_ply, e->opt.resign_keep); },
     "resignation", "a {} plays every game to the end and records one row per moved ply", "clear it with azx_clear_resign"},
    {"estop", [](const azx_engine *e) { return e->opt.estop_on; },
     [](const azx_engine *) { return std::string("on"); },
     "early stop", "a {} searches every ply in full", "clear it with azx_set_early_stop(e, 0)"},
    {"targets", [](const azx_engine *e) { return e->opt.tt_on(); },
     [](const azx_engine *e) {
         return strf("%s/%.9g", e->opt.tt_rows == AZX_ROWS_VISITS ? "visits" : "reference", (double)e->opt.tt_mix);
     },
     "training targets", "a {}'s harvest records the reference's rows and the outcome",
     "clear them with azx_set_train_targets(e, AZX_ROWS_REFERENCE, 0)"},
    {"forced", [](const azx_engine *e) { return e->opt.fp_k > 0.0f; },
     [](const azx_engine *e) { return strf("%.9g/%s", (double)e->opt.fp_k, e->opt.fp_prune ? "prune" : "noprune"); },
     "forced playouts", "a {} searches and draws every ply as the reference does",
     "clear them with azx_set_forced_playouts(e, 0, 0)"},
    {"gumbel", [](const azx_engine *e) { return e->opt.gm_m != 0; },
     [](const azx_engine *e) {
         return strf("%d/%.9g/%.9g/%s", e->opt.gm_m, (double)e->opt.gm_c_visit, (double)e->opt.gm_c_scale,
                     e->opt.gm_rows ? "rows" : "norows");
     },
     "the Gumbel root search", "a {} searches and draws every ply as the reference does",
     "clear it with azx_set_gumbel(e, 0, 0, 1, 0)"},
    {"book", [](const azx_engine *e) { return e->d.bk_n > 0; },
     [](const azx_engine *e) { return std::to_string(e->d.bk_n); },
     "a self-play opening book", "a {} starts its games from its own book",
     "azx_{}_set_openings; clear the engine's with azx_set_selfplay_openings(e, 0, ...)"},
};

static std::string selfplay_option_fields(const azx_engine *e) {
    std::string out;
    for (const OptionInfo &o : SELFPLAY_OPTIONS)
        out += std::string(" ") + o.field + "=" + (o.is_set(e) ? o.text(e) : std::string("off"));
    return out;
}

// A match or tournament (`what`) takes no engine with a self-play option set: AZX_EINVAL for the first option of the
// table that any engine has, naming the first engine that has it -- by its letter of `letters`, else by its index.
static int refuse_selfplay_options(azx_engine *const *eng, int n, const char *what, const char *letters) {
    for (const OptionInfo &o : SELFPLAY_OPTIONS)
        for (int k = 0; k < n; ++k) {
            if (!o.is_set(eng[k])) continue;
            std::string clauses = std::string(o.reason) + " (" + o.clear + ")";
            for (size_t at; (at = clauses.find("{}")) != std::string::npos;) clauses.replace(at, 2, what);
            const std::string who = letters ? std::string(1, letters[k]) : std::to_string(k);
            return fail(AZX_EINVAL, "engine %s has %s set: %s", who.c_str(), o.noun, clauses.c_str());
        }
    return AZX_OK;
}

extern "C" int azx_kernel_info(azx_engine *e, char *buf, int cap) {
    if (!e || !buf || cap < 1) return fail(AZX_EINVAL, "null argument");
    const DevEngine &d = e->d;
    const int S = d.slots <= 2 ? 2 : 3;
    char tree[96], play[160];
    if (d.evaluator == AZX_EVAL_UNIFORM || d.evaluator == AZX_EVAL_UNIFORM_HASH) {
        // the FAST instantiation also needs the default prior table and device (or no) noise: decided per launch
        DevEngine probe = d;
        probe.device_noise = 1;
        const bool fast = azx_mcts_fast_path(probe, MODE_BEGIN | MODE_INLINE, e->force_generic);
        snprintf(tree, sizeof tree, "k_mcts<%d,%s>", S, fast ? "FAST (throughput mode; generic with host noise)" : "generic");
        snprintf(play, sizeof play, "%s", fast && !e->no_persistent ? (S == 2 ? "k_play<2> (persistent)" : "k_play<3> (persistent)")
                                                                       : "k_mcts + k_choose + k_advance per move");
    } else {
        // (a policy temperature in force takes the phase launches to its own instantiation: azx_launch_mcts)
        if (d.pt_eighths != 8 || d.pt_root_eighths != 8)
            snprintf(tree, sizeof tree, "k_mcts_pt<%d> (BEGIN / APPLY|SELECT / APPLY phases)", S);
        else
            snprintf(tree, sizeof tree, "k_mcts<%d,generic> (BEGIN / APPLY|SELECT / APPLY phases)", S);
        snprintf(play, sizeof play, "%s", !use_pipeline(e) ? "phases + k_choose + k_advance per move, one stream"
                                          : e->stagger     ? "phases + k_choose + k_advance per move, two half-pools on two streams half an evaluation apart (any tower)"
                                                           : "phases + k_choose + k_advance per move, two half-pools on two streams");
    }
    std::string text = std::string("tree=") + tree + "; play=" + play + "; net=" +
                       (e->net ? azx_net_kernel_info(e->net) : "none") +
                       "; switches: AZX_MCTS_GENERIC=" + (e->force_generic ? "1" : "0") +
                       " AZX_NO_PERSISTENT=" + (e->no_persistent ? "1" : "0") +
                       " AZX_PIPELINE=" + (e->pipeline ? "1" : "0") +
                       " AZX_PIPELINE_STAGGER=" + (e->stagger ? "1" : "0") +
                       " reserved_cus=" + std::to_string(e->reserved_cus) +
                       " reflect=" + ((d.flags & AZX_FLAG_RANDOM_REFLECT) ? "on" : "off") +
                       selfplay_option_fields(e) +
                       (e->ro_R > 0 ? " eval=rollout(" + std::to_string(e->ro_R) + ")" : std::string()) +
                       "; src=" AZX_SRC_SHA +      // sha256 (16 hex digits) over the kernel sources this library was built from
                       "; temp=" + (e->pt_eighths == 8 && e->pt_root_eighths == 8 ? std::string("off")     // azx_set_policy_temp
                                    : std::to_string(e->pt_eighths) + "/8," + std::to_string(e->pt_root_eighths) + "/8");
    snprintf(buf, (size_t)cap, "%s", text.c_str());
    return (int)text.size();
}

extern "C" int azx_debug_stagger(azx_engine *e, int32_t *out4) {
    if (!e || !out4) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    memset(out4, 0, 4 * sizeof(int32_t));
    if (!e->stagger_ctr) return AZX_OK;
    HIPCHECK(hipMemcpyAsync(out4, e->stagger_ctr, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

// host only: the position-tile map k_tower_f16x3_s16 would run with on this board size (tower_tiles.h)
extern "C" int azx_debug_tower_tiles(int board_size, const char *map, uint8_t *rows256, uint32_t *skip4, int32_t *light_slot) {
    if (!map || !rows256 || !skip4 || !light_slot) return fail(AZX_EINVAL, "null argument");
    if (board_size < 2 || board_size * board_size > 121)
        return fail(AZX_EINVAL, "tower tiles: board size %d outside the fused tower's 2..11", board_size);
    if (strcmp(map, "edge") && strcmp(map, "rows")) return fail(AZX_EINVAL, "tower tiles: map '%s' is neither edge nor rows", map);
    AzxTowerTiles t;
    azx_tower_tiles_build(board_size, !strcmp(map, "edge"), &t);
    memcpy(rows256, t.row, sizeof t.row);
    for (int w = 0; w < 4; ++w) skip4[w] = t.skip[w];
    *light_slot = AZX_TOWER_LIGHT_SLOT;
    return t.edge;
}

// host only: which tower and heads kernels azx_create would give a network of this shape (net_kernels.hip: net_plan)
extern "C" int azx_debug_tower_choice(int board_size, int num_blocks, int base_chans, int flags, char *buf, int cap) {
    if (!buf || cap < 1) return fail(AZX_EINVAL, "null argument");
    const int rc = azx_net_describe(board_size, num_blocks, base_chans, (flags & AZX_FLAG_TOWER_F16) ? 1 : 0, buf, cap);
    if (rc < 0) g_err = azx_net_error();
    return rc;
}

extern "C" int azx_debug_set_queue_cap(azx_engine *e, int64_t rows) {
    if (!e || rows < 0) return fail(AZX_EINVAL, "bad argument");
    e->dbg_qcap = rows;
    return AZX_OK;
}

// AZX_ERANGE when a split-f16 tower launch of this call overflowed an activation (net_kernels.hip: NetDev::sat_flag)
static int check_net_range(azx_engine *e) {
    if (!e->net) return AZX_OK;
    int rc = azx_net_check_range(e->net, e->stream);
    if (rc) g_err = azx_net_error();
    return rc;
}

extern "C" int azx_debug_weights(azx_engine *e, int which, void *out, int64_t cap, int64_t *nbytes, char *name, int name_cap) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    if (!e->net) return fail(AZX_ESTATE, "engine was not created with AZX_EVAL_RESNET");
    int rc = azx_net_debug_weights(e->net, which, out, cap, nbytes, name, name_cap);
    if (rc) g_err = azx_net_error();
    return rc;
}

extern "C" int azx_set_weights(azx_engine *e, int n_tensors, const char *const *names,
                               const void *const *ptrs, const int64_t *counts, int on_device) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    if (!e->net) return fail(AZX_ESTATE, "engine was not created with AZX_EVAL_RESNET");
    int rc = azx_net_set_weights(e->net, n_tensors, names, ptrs, counts, on_device);
    if (rc) g_err = azx_net_error();
    return rc;
}

extern "C" int azx_set_prior_table(azx_engine *e, const float *prior_by_k, int count) {
    if (!e || !prior_by_k) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    if (count < e->d.ncells + 1) return fail(AZX_EINVAL, "prior table needs %d entries", e->d.ncells + 1);
    if (!e->prior_table_dev) TRY(dev_alloc(e, &e->prior_table_dev, (size_t)e->d.ncells + 1));
    HIPCHECK(hipMemcpyAsync(e->prior_table_dev, prior_by_k, sizeof(float) * (e->d.ncells + 1),
                            hipMemcpyHostToDevice, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    e->d.prior_by_k = e->prior_table_dev;
    e->d.prior_default = 0;
    return AZX_OK;
}

extern "C" int azx_reset(azx_engine *e, const int32_t *slots, int n_slots, const int32_t *moves,
                         const int32_t *n_moves, int stride) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    DevEngine &d = e->d;
    if (!slots) n_slots = d.G;
    if (n_slots < 1 || n_slots > d.G) return fail(AZX_EINVAL, "n_slots %d outside [1, %d]", n_slots, d.G);
    if (slots) {
        for (int i = 0; i < n_slots; ++i)
            if (slots[i] < 0 || slots[i] >= d.G) return fail(AZX_EINVAL, "slot %d out of range", slots[i]);
        HIPCHECK(hipMemcpyAsync(e->slots_dev, slots, sizeof(int32_t) * n_slots, hipMemcpyHostToDevice, e->stream));
    }
    if (moves) {
        if (!n_moves || stride < 1) return fail(AZX_EINVAL, "moves given without n_moves/stride");
        const size_t need = (size_t)n_slots * stride;
        if (need > e->moves_cap) {
            TRY(dev_alloc(e, &e->moves_dev, need));
            e->moves_cap = need;
        }
        // validate on the host: the device step assumes legal moves (hex.py:173-176 asserts)
        for (int i = 0; i < n_slots; ++i) {
            if (n_moves[i] < 0 || n_moves[i] > stride) return fail(AZX_EINVAL, "n_moves[%d] out of range", i);
            std::vector<char> used(d.ncells, 0);
            for (int p = 0; p < n_moves[i]; ++p) {
                const int mv = moves[(size_t)i * stride + p];
                if (mv < 1 || mv > d.ncells || used[mv - 1]) return fail(AZX_EINVAL, "illegal move %d", mv);
                used[mv - 1] = 1;
            }
        }
        HIPCHECK(hipMemcpyAsync(e->moves_dev, moves, sizeof(int32_t) * need, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(hipMemcpyAsync(e->nmoves_dev, n_moves, sizeof(int32_t) * n_slots, hipMemcpyHostToDevice, e->stream));
    }
    azx_launch_reset(d, slots ? e->slots_dev : nullptr, n_slots, moves ? e->moves_dev : nullptr,
                     moves ? e->nmoves_dev : nullptr, stride, 1, e->stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(e->stream));
    e->phase_api = SearchCursor();
    if (e->ext_failed) {
        for (int i = 0; i < n_slots; ++i) e->ext_dirty[slots ? slots[i] : i] = 0;
        e->ext_failed = std::find(e->ext_dirty.begin(), e->ext_dirty.end(), 1) != e->ext_dirty.end();
    }
    return AZX_OK;
}

// ---- timing of the tree kernels (roofline: algorithmic bytes / measured launch time) --------
static void time_begin(azx_engine *e, char tag = 0, hipStream_t s = nullptr, int group = 0, int ref = -1) {
    if (e->ev_used + 2 > e->ev_pool.size()) {
        if (e->ev_pool.size() >= 1 << 16) return;
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
        e->ev_pool.push_back(a);
        e->ev_pool.push_back(b);
    }
    const size_t n = e->ev_pool.size() / 2, i = e->ev_used / 2;
    if (e->ev_tag.size() < n) { e->ev_tag.resize(n, 0); e->ev_weight.resize(n, 1); e->ev_group.resize(n, 0); e->ev_ref.resize(n, -1); }
    e->ev_tag[i] = tag;
    e->ev_weight[i] = 1;
    e->ev_group[i] = ref >= 0 ? group : 0;
    e->ev_ref[i] = ref;
    (void)hipEventRecord(e->ev_pool[e->ev_used], s ? s : e->stream);
}
// (on the stream time_begin recorded on: a pipelined launch is timed on its half-pool's stream)
static void time_end(azx_engine *e, int weight = 1, hipStream_t s = nullptr) {
    if (e->ev_used + 2 > e->ev_pool.size()) return;     // pool full: time_begin recorded nothing either
    (void)hipEventRecord(e->ev_pool[e->ev_used + 1], s ? s : e->stream);
    e->ev_weight[e->ev_used / 2] = weight;
    e->ev_used += 2;
}
// a reference mark on stream s for grouped launches issued after it (its pool index, -1 when the pool is full)
static int time_mark(azx_engine *e, hipStream_t s) {
    time_begin(e, 2, s);
    if (e->ev_used + 2 > e->ev_pool.size()) return -1;
    const int ref = (int)e->ev_used;
    time_end(e, 1, s);
    return ref;
}
static void time_collect(azx_engine *e, azx_play_stats *st) {
    auto book = [&](char tag, int weight, double seconds, int launches) {
        if (tag == 1) { st->net_seconds += seconds; st->net_launches += launches; }
        else {
            st->mcts_seconds += seconds;
            st->mcts_launches += weight * launches;
            st->mcts_kernel_launches += launches;
        }
    };
    std::map<int, char> groups;                                      // group id -> tag (one launch each)
    std::map<std::pair<int, char>, std::vector<std::pair<float, float>>> spans;   // (reference, tag) -> spans (ms)
    for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
        const size_t k = i / 2;
        if (e->ev_tag[k] == 2) continue;
        float ms = 0.f;
        if (!e->ev_group[k]) {
            if (hipEventElapsedTime(&ms, e->ev_pool[i], e->ev_pool[i + 1]) == hipSuccess)
                book(e->ev_tag[k], e->ev_weight[k], ms * 1e-3, 1);
            continue;
        }
        float b = 0.f, en = 0.f;
        const hipEvent_t ref = e->ev_pool[e->ev_ref[k]];
        if (hipEventElapsedTime(&b, ref, e->ev_pool[i]) != hipSuccess || hipEventElapsedTime(&en, ref, e->ev_pool[i + 1]) != hipSuccess)
            continue;
        groups[e->ev_group[k]] = e->ev_tag[k];
        spans[{e->ev_ref[k], e->ev_tag[k]}].push_back({b, en});
    }
    for (const auto &g : groups) book(g.second, 1, 0.0, 1);
    for (auto &kv : spans) {
        std::vector<std::pair<float, float>> &v = kv.second;
        std::sort(v.begin(), v.end());
        double total = 0.0;
        float lo = v[0].first, hi = v[0].second;
        for (const auto &iv : v) {
            if (iv.first > hi) { total += hi - lo; lo = iv.first; hi = iv.second; }
            else hi = std::max(hi, iv.second);
        }
        total += hi - lo;
        book(kv.first.second, 1, total * 1e-3, 0);
    }
    e->ev_used = 0;
    e->ev_groups = 0;
}

static int upload_noise(azx_engine *e, const double *noise, int n_select, int noise_stride,
                        double noise_scale) {
    DevEngine &d = e->d;
    d.noise = nullptr;
    d.device_noise = 0;
    d.noise_scale = noise_scale;
    d.n_select = n_select;
    d.noise_stride = noise_stride;
    if (noise_scale == 0.0) return AZX_OK;
    if (!noise) { d.device_noise = 1; return AZX_OK; }
    if (n_select < e->selects_per_search)
        return fail(AZX_EINVAL, "noise has %d rows, a search consumes %d", n_select, e->selects_per_search);
    const size_t need = (size_t)d.G * n_select * noise_stride;
    if (need > e->noise_cap) {
        if (e->noise_dev) {      // searches are blocking: no kernel still reads the old rows
            (void)hipFree(e->noise_dev);
            e->allocs.erase(std::remove(e->allocs.begin(), e->allocs.end(), (void *)e->noise_dev), e->allocs.end());
            e->noise_dev = nullptr;
            e->noise_cap = 0;
        }
        TRY(dev_alloc(e, &e->noise_dev, need, false));
        e->noise_cap = need;
    }
    HIPCHECK(hipMemcpyAsync(e->noise_dev, noise, sizeof(double) * need, hipMemcpyHostToDevice, e->stream));
    d.noise = e->noise_dev;
    return AZX_OK;
}

// ---- registered external evaluator (azx_set_external_evaluator) ------------------------------------------------
static bool ext_registered(const azx_engine *e) {
    return e->d.evaluator == AZX_EVAL_EXTERNAL && (e->ext_fn || e->ro_R > 0);
}

static int ext_refuse(const azx_engine *e) {
    if (!e->ext_failed) return AZX_OK;
    return fail(AZX_ESTATE, "an external evaluation failed and left searches half done: azx_reset every slot first");
}

// a failed hand-over: the slots' searches stop where they are; nothing queued is waited for by a later call
static int ext_fail(azx_engine *e, const char *fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    (void)hipStreamSynchronize(e->stream);
    const int32_t clear = AZX_EXT_NO_ERROR;
    (void)hipMemcpyAsync(e->ext.info + 2, &clear, sizeof clear, hipMemcpyHostToDevice, e->stream);
    (void)hipStreamSynchronize(e->stream);
    e->ext_info[2] = clear;
    e->phase_api = SearchCursor();
    e->ev_used = 0;                       // the timed launches of the failed call are not booked
    e->ev_groups = 0;
    e->ext_failed = true;
    std::fill(e->ext_dirty.begin(), e->ext_dirty.end(), 1);
    return fail(AZX_EEXTERNAL, "%s", buf);
}

// what k_ext_import found wrong with the first bad row since the last read (ext_info[2])
static int ext_check_rows(azx_engine *e) {
    const int32_t w = e->ext_info[2];
    if (w == AZX_EXT_NO_ERROR) return AZX_OK;
    const int row = w >> 3, what = w & 7;
    return ext_fail(e, "external evaluator: row %d of its batch %s", row,
                    (what & 1) ? "has a value that is not finite"
                    : (what & 2) ? "has a negative (or NaN) prior probability"
                                 : "has prior probabilities whose sum is not 1 within 1e-4 (mcts.py:211-213)");
}

// ext.info -> the pinned host words, enqueued on `s` (not waited for); ext_info_take after that stream was waited for
static int ext_info_enqueue(azx_engine *e, hipStream_t s) {
    HIPCHECK(hipMemcpyAsync(e->ext_info_host, e->ext.info, sizeof e->ext_info, hipMemcpyDeviceToHost, s));
    return AZX_OK;
}

static int ext_info_take(azx_engine *e) {
    memcpy(e->ext_info, e->ext_info_host, sizeof e->ext_info);
    return ext_check_rows(e);
}

static int ext_read_info(azx_engine *e) {
    TRY(ext_info_enqueue(e, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return ext_info_take(e);
}

// One evaluation point of the phase loop, where the resnet path calls azx_net_eval, in two halves.  The first needs
// no host: the pending requests are put in (slot, leaf) order and n, kmax and the previous import's error word are
// sent to the host.  The second waits for those words (the one host sync of the point), then: the rows out to the
// caller's buffers, the callback, the checked results back into ev_*.
static int ext_point_enqueue(azx_engine *e, bool timed) {
    if (timed) time_begin(e, 1);
    azx_launch_ext_order(e->d, e->ext, e->stream);
    HIPCHECK(hipGetLastError());
    return ext_info_enqueue(e, e->stream);
}

static int ext_point_finish(azx_engine *e, bool timed) {
    DevEngine &d = e->d;
    HIPCHECK(hipStreamSynchronize(e->stream));
    const int rc_info = ext_info_take(e);
    if (rc_info) return rc_info;
    const int n = e->ext_info[0], kmax = e->ext_info[1];
    if (n < 0 || n > d.G * d.bs) return ext_fail(e, "external evaluator: %d pending rows (internal error)", n);
    if (n > 0) {
        azx_launch_ext_export(d, e->ext, n, e->stream);
        HIPCHECK(hipGetLastError());
        if (e->ro_R > 0) {      // the rollout evaluator: a kernel on the same stream where the callback would run
            azx_launch_rollout_ex(e->ext.board, n, d.N, e->ro_R, e->ro_seed, e->ext.value, e->ext.prior, nullptr, nullptr,
                                  e->ro_won, e->stream);
            HIPCHECK(hipGetLastError());
            e->ro_handovers += 1;
            e->ro_rows += n;
        } else {
            const int rc = e->ext_fn(e->ext_user, n, kmax, e->ext.board, e->ext.legal, e->ext.value, e->ext.prior,
                                     (void *)e->stream);
            if (rc) return ext_fail(e, "external evaluator returned %d on a batch of %d rows", rc, n);
        }
        azx_launch_ext_import(d, e->ext, n, e->stream);
        HIPCHECK(hipGetLastError());
    }
    if (timed) time_end(e);
    return AZX_OK;
}

// Where the launches of one phase of a search (the schedule: phase_mode, above azx_engine) go: the pool or half-pool they cover, its stream, and how they are timed -- `group` and `ref`
// as time_begin takes them.  The defaults are the whole pool on the engine stream, each launch timed on its own.
struct PhaseWhere {
    const DevEngine *view;
    hipStream_t stream;
    bool timed;
    int group = 0, ref = -1;
};
static PhaseWhere whole_pool(azx_engine *e, bool timed) { return {&e->d, e->stream, timed}; }

// a tree launch with its timing pair: every k_mcts launch of a search, and the uniform evaluators' fused one
static void launch_tree(azx_engine *e, const PhaseWhere &w, int mode) {
    if (w.timed) time_begin(e, 0, w.stream, w.group, w.ref);
    azx_launch_mcts(*w.view, mode, e->num_batches, w.stream, e->force_generic);
    if (w.timed) time_end(e, 1, w.stream);
}

// the tree launch of phase `ph`; a phase that queues leaves for an evaluation starts from an empty queue
static int enqueue_tree_phase(azx_engine *e, const PhaseWhere &w, int ph) {
    const PhaseMode m = phase_mode(ph, e->num_batches);
    if (m.then_eval) HIPCHECK(hipMemsetAsync(w.view->n_eval, 0, sizeof(int32_t), w.stream));
    launch_tree(e, w, m.bits);
    return AZX_OK;
}

// the network's evaluation of the leaves a phase queued
static void enqueue_net_eval(azx_engine *e, const PhaseWhere &w) {
    if (w.timed) time_begin(e, 1, w.stream);
    azx_net_eval(e->net, *w.view, w.stream);
    if (w.timed) time_end(e, 1, w.stream);
}

// Issues the cursor's next phase on the engine stream: the tree launch and, after phases 0 .. nb, what evaluates the
// leaves it queued -- the network's launches, the first half of a registered evaluator's point, or nothing, where
// the phase API's caller evaluates.  A registered evaluator's point is finished (host sync, callback: its second half)
// at the start of the next call, so that all the host can enqueue without waiting is on the stream before it waits.
// enqueue_search runs a cursor to its end; ply_searches advances several engines' cursors in turn; the phase API
// advances the engine's own by one phase per call.
static int search_advance(azx_engine *e, SearchCursor *c) {
    const bool net = e->d.evaluator == AZX_EVAL_RESNET, point = !net && !c->by_caller;
    const PhaseWhere w = whole_pool(e, c->timed);
    if (point && c->next > 0) TRY(ext_point_finish(e, c->timed));
    const int ph = c->next++;
    if (ph == 0 && net && !azx_net_ready(e->net)) return fail(AZX_ESTATE, "azx_set_weights has not been called");
    TRY(enqueue_tree_phase(e, w, ph));
    if (!phase_mode(ph, e->num_batches).then_eval) return AZX_OK;
    if (net) enqueue_net_eval(e, w);
    return point ? ext_point_enqueue(e, c->timed) : AZX_OK;
}

// the hand-over buffers of a registered evaluator, made at the first registration and kept
static int ext_alloc(azx_engine *e) {
    if (!e->ext.info) {
        const size_t E = (size_t)e->d.G * e->d.bs, nc = (size_t)e->d.ncells;
        ExtBufs x = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        int rc = AZX_OK;
        if (!rc) rc = dev_alloc(e, &x.src2ev, E);
        if (!rc) rc = dev_alloc(e, &x.row_ev, E);
        if (!rc) rc = dev_alloc(e, &x.info, 4);
        if (!rc) rc = dev_alloc(e, &x.board, E * nc);
        if (!rc) rc = dev_alloc(e, &x.legal, E * nc);
        if (!rc) rc = dev_alloc(e, &x.value, E);
        if (!rc) rc = dev_alloc(e, &x.prior, E * nc);
        if (rc) return rc;
        if (!e->ext_info_host &&
            hipHostMalloc((void **)&e->ext_info_host, sizeof e->ext_info, hipHostMallocDefault) != hipSuccess)
            return fail(AZX_ENOMEM, "hipHostMalloc of the evaluator's info words failed");
        const int32_t init[4] = {0, 0, AZX_EXT_NO_ERROR, 0};
        HIPCHECK(hipMemcpyAsync(x.info, init, sizeof init, hipMemcpyHostToDevice, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
        e->ext = x;
        e->ext_dirty.assign((size_t)e->d.G, 0);
    }
    return AZX_OK;
}

// The policy temperature in force (azx_set_policy_temp): the rollout evaluator hands every child one table prior, and
// such rows are untouched by the rule (include/azx.h), so while it is set the launches see (8, 8).
static void pt_refresh(azx_engine *e) {
    const bool table = e->ro_R > 0;
    e->d.pt_eighths = table ? 8 : e->pt_eighths;
    e->d.pt_root_eighths = table ? 8 : e->pt_root_eighths;
}

extern "C" int azx_set_external_evaluator(azx_engine *e, azx_eval_fn fn, void *user) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    if (e->d.evaluator != AZX_EVAL_EXTERNAL)
        return fail(AZX_EINVAL, "an external evaluator needs an AZX_EVAL_EXTERNAL engine (this one has evaluator %d)",
                    e->d.evaluator);
    if (fn) TRY(ext_alloc(e));
    e->ext_fn = fn;
    e->ext_user = fn ? user : nullptr;
    if (fn) e->ro_R = 0;                 // it and azx_set_rollout_evaluator replace each other: the last call wins
    pt_refresh(e);
    return AZX_OK;
}

// ---- rollout evaluator (azx_set_rollout_evaluator; NOT the reference's behaviour) --------------------------------
extern "C" int azx_set_rollout_evaluator(azx_engine *e, int rollouts, uint64_t seed) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    if (e->d.evaluator != AZX_EVAL_EXTERNAL)
        return fail(AZX_EINVAL, "a rollout evaluator needs an AZX_EVAL_EXTERNAL engine (this one has evaluator %d)",
                    e->d.evaluator);
    if (rollouts < 0 || rollouts > AZX_ROLLOUT_MAX)
        return fail(AZX_EINVAL, "rollouts must be 0 (unregister) or in [1, %d], got %d", AZX_ROLLOUT_MAX, rollouts);
    if (rollouts > 0 && (e->d.flags & AZX_FLAG_RANDOM_REFLECT))
        return fail(AZX_EINVAL, "a rollout evaluator is a function of the position as it stands: the engine was created "
                                "with AZX_FLAG_RANDOM_REFLECT");
    if (rollouts == 0) {
        e->ro_R = 0;
        pt_refresh(e);
        return AZX_OK;
    }
    TRY(ext_alloc(e));
    if (!e->ro_won) TRY(dev_alloc(e, &e->ro_won, 1));
    HIPCHECK(hipMemsetAsync(e->ro_won, 0, sizeof *e->ro_won, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    e->ro_R = rollouts;
    e->ro_seed = seed;
    e->ro_handovers = e->ro_rows = 0;
    e->ext_fn = nullptr;
    e->ext_user = nullptr;
    pt_refresh(e);
    return AZX_OK;
}

extern "C" int azx_rollout_stats(azx_engine *e, int64_t out4[4]) {
    if (!e || !out4) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    unsigned long long won = 0;
    if (e->ro_won) {
        HIPCHECK(hipMemcpyAsync(&won, e->ro_won, sizeof won, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
    }
    out4[0] = e->ro_handovers;
    out4[1] = e->ro_rows;
    out4[2] = e->ro_rows * (int64_t)e->ro_R;
    out4[3] = (int64_t)won;
    return AZX_OK;
}

static int rollout_args(int board_size, int n, const int32_t *boards, int rollouts) {
    if (board_size < 2 || board_size > AZX_MAX_BOARD)
        return fail(AZX_EINVAL, "rollout: board size %d outside [2, %d]", board_size, AZX_MAX_BOARD);
    if (rollouts < 1 || rollouts > AZX_ROLLOUT_MAX)
        return fail(AZX_EINVAL, "rollout: rollouts %d outside [1, %d]", rollouts, AZX_ROLLOUT_MAX);
    if (n < 1) return fail(AZX_EINVAL, "rollout: %d rows", n);
    if (!boards) return fail(AZX_EINVAL, "null argument");
    const size_t total = (size_t)n * board_size * board_size;
    for (size_t i = 0; i < total; ++i)
        if (boards[i] < 0 || boards[i] > 2)
            return fail(AZX_EINVAL, "rollout: cell %zu holds %d, not 0, 1 or 2", i, boards[i]);
    return AZX_OK;
}

extern "C" int azx_rollout_value(uint64_t seed, int board_size, const int32_t *board, int rollouts, int32_t *wins,
                                 float *value) {
    if (!wins || !value) return fail(AZX_EINVAL, "null argument");
    TRY(rollout_args(board_size, 1, board, rollouts));
    const int w = azx_rollout_host(seed, board_size, board, rollouts);
    *wins = w;
    *value = (float)(2 * w - rollouts) / (float)rollouts;
    return AZX_OK;
}

// ---- self-test hook (tests): the rollout kernel alone on host boards -------------------------------------------
extern "C" int azx_selftest_rollout(int device, int board_size, int n, const int32_t *boards, int rollouts, uint64_t seed,
                                    int32_t *wins, float *value, float *prior, uint8_t *fills) {
    if (!wins || !value || !prior) return fail(AZX_EINVAL, "null argument");
    TRY(rollout_args(board_size, n, boards, rollouts));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(AZX_ENODEV, "no HIP device visible");
    DevGuard guard(device);
    const size_t cells = (size_t)board_size * board_size, rows = (size_t)n;
    const size_t nf = (size_t)(rollouts < AZX_ROLLOUT_FILLS ? rollouts : AZX_ROLLOUT_FILLS);
    int32_t *db = nullptr, *dw = nullptr;
    float *dv = nullptr, *dp = nullptr;
    uint8_t *df = nullptr;
    hipError_t err = hipMalloc(&db, rows * cells * 4);
    if (err == hipSuccess) err = hipMalloc(&dw, rows * 4);
    if (err == hipSuccess) err = hipMalloc(&dv, rows * 4);
    if (err == hipSuccess) err = hipMalloc(&dp, rows * cells * 4);
    if (err == hipSuccess && fills) err = hipMalloc(&df, rows * nf * cells);
    if (err == hipSuccess) err = hipMemcpy(db, boards, rows * cells * 4, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        azx_launch_rollout_ex(db, n, board_size, rollouts, seed, dv, dp, dw, df, nullptr, nullptr);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
    }
    if (err == hipSuccess) err = hipMemcpy(wins, dw, rows * 4, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(value, dv, rows * 4, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(prior, dp, rows * cells * 4, hipMemcpyDeviceToHost);
    if (err == hipSuccess && fills) err = hipMemcpy(fills, df, rows * nf * cells, hipMemcpyDeviceToHost);
    (void)hipFree(db); (void)hipFree(dw); (void)hipFree(dv); (void)hipFree(dp); (void)hipFree(df);    // (on every path)
    if (err != hipSuccess) return fail(AZX_EHIP, "azx_selftest_rollout: %s", hipGetErrorString(err));
    return AZX_OK;
}

// one whole search on the stream (no host sync) for the device-side evaluators; with a registered external
// evaluator the host takes part at every evaluation point and the call returns after the last one
static int enqueue_search(azx_engine *e, bool timed) {
    const int ev = e->d.evaluator;
    if (ev == AZX_EVAL_UNIFORM || ev == AZX_EVAL_UNIFORM_HASH) {
        launch_tree(e, whole_pool(e, timed), MODE_BEGIN | MODE_INLINE);     // evaluated inside the kernel: all phases in one launch
        return AZX_OK;
    }
    if (ev != AZX_EVAL_RESNET && !ext_registered(e)) return fail(AZX_ESTATE, "evaluator %d has no device pipeline", ev);
    SearchCursor c(e->num_batches, timed, false);
    while (!c.done()) TRY(search_advance(e, &c));
    return AZX_OK;
}

// how a call that searched ends: the last import's checks, or the network's range check
static int search_outcome(azx_engine *e) {
    if (ext_registered(e)) return ext_read_info(e);
    return check_net_range(e);
}

extern "C" int azx_search(azx_engine *e, const double *noise, int n_select, int noise_stride,
                          double noise_scale) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    TRY(ext_refuse(e));
    if (e->d.evaluator == AZX_EVAL_EXTERNAL && !ext_registered(e))
        return fail(AZX_ESTATE, "AZX_EVAL_EXTERNAL: drive azx_search_begin/step instead");
    TRY(upload_noise(e, noise, n_select, noise_stride, noise_scale));
    TRY(enqueue_search(e, false));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(e->stream));
    return search_outcome(e);
}

static int read_pending(azx_engine *e, int *n_pending) {
    int32_t n = 0;
    HIPCHECK(hipMemcpyAsync(&n, e->d.n_eval, sizeof n, hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    *n_pending = n;
    return e->d.evaluator == AZX_EVAL_RESNET ? check_net_range(e) : AZX_OK;
}

extern "C" int azx_search_begin(azx_engine *e, const double *noise, int n_select, int noise_stride,
                                double noise_scale, int *n_pending) {
    if (!e || !n_pending) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(ext_refuse(e));
    if (e->d.evaluator != AZX_EVAL_EXTERNAL && e->d.evaluator != AZX_EVAL_RESNET)
        return fail(AZX_ESTATE, "phase API needs AZX_EVAL_EXTERNAL (or RESNET)");
    TRY(upload_noise(e, noise, n_select, noise_stride, noise_scale));
    SearchCursor c(e->num_batches, false, true);
    TRY(search_advance(e, &c));
    HIPCHECK(hipGetLastError());
    e->phase_api = c;                   // in flight from here on
    return read_pending(e, n_pending);
}

extern "C" int azx_search_step(azx_engine *e, int *n_pending, int *done) {
    if (!e || !n_pending || !done) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    SearchCursor &c = e->phase_api;
    if (c.done()) return fail(AZX_ESTATE, "azx_search_step without azx_search_begin");
    // the host reads n_eval back after every phase, the last included: that one queues nothing and so leaves the
    // count alone, which is zeroed here
    if (!phase_mode(c.next, e->num_batches).then_eval) HIPCHECK(hipMemsetAsync(e->d.n_eval, 0, sizeof(int32_t), e->stream));
    TRY(search_advance(e, &c));
    *done = c.done() ? 1 : 0;
    HIPCHECK(hipGetLastError());
    return read_pending(e, n_pending);
}

static int flip_cell(int cell, int N) {   // hex.py:107-111 (r,c) -> (N-1-c, N-1-r)
    const int r = cell / N, c = cell % N;
    return (N - 1 - c) * N + (N - 1 - r);
}

extern "C" int azx_get_leaves(azx_engine *e, int cap, int32_t *boards, int32_t *legal_moves,
                              int32_t *slot, int32_t *k, int *n_out) {
    if (!e || !n_out) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    DevEngine &d = e->d;
    int n = 0;
    TRY(read_pending(e, &n));
    if (n > cap) return fail(AZX_EINVAL, "%d pending leaves, caller capacity %d", n, cap);
    *n_out = n;
    e->ext_order.clear();
    e->ext_cells.clear();
    if (n == 0) return AZX_OK;
    std::vector<uint8_t> hb((size_t)n * AZX_CELL_STRIDE);
    std::vector<int32_t> hsrc(n), hflip(n);
    HIPCHECK(hipMemcpyAsync(hb.data(), d.ev_board, hb.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipMemcpyAsync(hsrc.data(), d.ev_src, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipMemcpyAsync(hflip.data(), d.ev_flip, sizeof(int32_t) * n, hipMemcpyDeviceToHost, e->stream));
    const size_t E = (size_t)d.G * d.bs;
    std::vector<uint64_t> hmask(E * 4);
    HIPCHECK(hipMemcpyAsync(hmask.data(), d.leaf_mask, sizeof(uint64_t) * hmask.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return hsrc[a] < hsrc[b]; });
    e->ext_order = order;
    e->ext_cells.resize(n);
    for (int j = 0; j < n; ++j) {
        const int ev = order[j], src = hsrc[ev];
        std::vector<int> &cells = e->ext_cells[j];
        for (int c = 0; c < d.ncells; ++c)
            if ((hmask[(size_t)src * 4 + (c >> 6)] >> (c & 63)) & 1ull) cells.push_back(c);
        if (slot) slot[j] = src / d.bs;
        if (k) k[j] = (int)cells.size();
        if (boards)
            for (int c = 0; c < d.ncells; ++c)
                boards[(size_t)j * d.ncells + c] = hb[(size_t)ev * AZX_CELL_STRIDE + c];
        if (legal_moves) {
            for (int c = 0; c < d.ncells; ++c) legal_moves[(size_t)j * d.ncells + c] = 0;
            for (size_t i = 0; i < cells.size(); ++i) {
                const int t = (hflip[ev] & 1) ? flip_cell(cells[i], d.N) : cells[i];
                legal_moves[(size_t)j * d.ncells + i] = ((hflip[ev] & 2) ? d.ncells - 1 - t : t) + 1;   // bit 1: turned by 180 degrees
            }
        }
    }
    return AZX_OK;
}

extern "C" int azx_put_evals(azx_engine *e, int n, const float *value, const float *prior) {
    if (!e || (n && (!value || !prior))) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    DevEngine &d = e->d;
    if (n != (int)e->ext_order.size())
        return fail(AZX_ESTATE, "azx_put_evals(%d) does not match %zu pending leaves", n, e->ext_order.size());
    if (n == 0) return AZX_OK;
    std::vector<float> hv(n), hp((size_t)n * AZX_CELL_STRIDE, 0.0f);
    for (int j = 0; j < n; ++j) {
        const int ev = e->ext_order[j];
        hv[ev] = value[j];
        const std::vector<int> &cells = e->ext_cells[j];
        for (size_t i = 0; i < cells.size(); ++i)
            hp[(size_t)ev * AZX_CELL_STRIDE + cells[i]] = prior[(size_t)j * d.ncells + i];
    }
    HIPCHECK(hipMemcpyAsync(d.ev_value, hv.data(), sizeof(float) * n, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(hipMemcpyAsync(d.ev_prior, hp.data(), sizeof(float) * hp.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

extern "C" int azx_get_evals(azx_engine *e, int cap, float *value, float *prior, int *n_out) {
    if (!e || !n_out) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    DevEngine &d = e->d;
    const int n = (int)e->ext_order.size();
    if (n > cap) return fail(AZX_EINVAL, "%d evaluations, caller capacity %d", n, cap);
    *n_out = n;
    if (n == 0) return AZX_OK;
    std::vector<float> hv(n), hp((size_t)n * AZX_CELL_STRIDE);
    HIPCHECK(hipMemcpyAsync(hv.data(), d.ev_value, sizeof(float) * n, hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipMemcpyAsync(hp.data(), d.ev_prior, sizeof(float) * hp.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    for (int j = 0; j < n; ++j) {
        const int ev = e->ext_order[j];
        if (value) value[j] = hv[ev];
        if (prior) {
            const std::vector<int> &cells = e->ext_cells[j];
            for (int c = 0; c < d.ncells; ++c) prior[(size_t)j * d.ncells + c] = 0.0f;
            for (size_t i = 0; i < cells.size(); ++i)
                prior[(size_t)j * d.ncells + i] = hp[(size_t)ev * AZX_CELL_STRIDE + cells[i]];
        }
    }
    return AZX_OK;
}

extern "C" int azx_get_root(azx_engine *e, int32_t *k, int32_t *legal_moves, float *child_visits,
                            float *child_value, float *child_prior, float *root_visits,
                            float *root_value, int32_t *num_nodes, float *search_value) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    DevEngine &d = e->d;
    const size_t G = d.G, GC = G * d.ncells;
    HIPCHECK(hipMemsetAsync(e->g_legal, 0, sizeof(int32_t) * GC, e->stream));
    HIPCHECK(hipMemsetAsync(e->g_cv, 0, sizeof(float) * GC, e->stream));
    HIPCHECK(hipMemsetAsync(e->g_cw, 0, sizeof(float) * GC, e->stream));
    HIPCHECK(hipMemsetAsync(e->g_cp, 0, sizeof(float) * GC, e->stream));
    azx_launch_gather_root(d, e->g_k, e->g_legal, e->g_cv, e->g_cw, e->g_cp, e->g_rv, e->g_rw,
                           e->g_nn, e->g_sv, e->stream);
    HIPCHECK(hipGetLastError());
#define D2H(dst, src, bytes) if (dst) HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream))
    D2H(k, e->g_k, sizeof(int32_t) * G);
    D2H(legal_moves, e->g_legal, sizeof(int32_t) * GC);
    D2H(child_visits, e->g_cv, sizeof(float) * GC);
    D2H(child_value, e->g_cw, sizeof(float) * GC);
    D2H(child_prior, e->g_cp, sizeof(float) * GC);
    D2H(root_visits, e->g_rv, sizeof(float) * G);
    D2H(root_value, e->g_rw, sizeof(float) * G);
    D2H(num_nodes, e->g_nn, sizeof(int32_t) * G);
    D2H(search_value, e->g_sv, sizeof(float) * G);
#undef D2H
    HIPCHECK(hipStreamSynchronize(e->stream));
    if (search_value) {   // mcts.py:291
        const float denom = (float)(e->num_batches * d.bs);
        for (size_t g = 0; g < G; ++g) search_value[g] = search_value[g] / denom;
    }
    return AZX_OK;
}

extern "C" int azx_get_status(azx_engine *e, int32_t *status) {
    if (!e || !status) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    std::vector<TreeHdr> th(e->d.G);
    HIPCHECK(hipMemcpyAsync(th.data(), e->d.thdr, sizeof(TreeHdr) * th.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    for (int g = 0; g < e->d.G; ++g) status[g] = th[g].status;
    return AZX_OK;
}

extern "C" int azx_debug_slow_div(azx_engine *e, int32_t *out) {
    if (!e || !out) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    std::vector<TreeHdr> th(e->d.G);
    HIPCHECK(hipMemcpyAsync(th.data(), e->d.thdr, sizeof(TreeHdr) * th.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    for (int g = 0; g < e->d.G; ++g) out[g] = th[g].slow_div != 0;
    return AZX_OK;
}

extern "C" int azx_get_tree_nodes(azx_engine *e, int32_t *nodes) {
    if (!e || !nodes) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    std::vector<TreeHdr> th(e->d.G);
    HIPCHECK(hipMemcpyAsync(th.data(), e->d.thdr, sizeof(TreeHdr) * th.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    for (int g = 0; g < e->d.G; ++g) nodes[g] = th[g].num_nodes + th[g].dropped;
    return AZX_OK;
}

extern "C" int azx_get_games(azx_engine *e, int32_t *board, int32_t *color, int32_t *result,
                             int32_t *ply) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    DevEngine &d = e->d;
    const size_t G = d.G;
    std::vector<uint32_t> hc(G * d.slots * 64);
    std::vector<GameHdr> hh(G);
    HIPCHECK(hipMemcpyAsync(hc.data(), d.cells, sizeof(uint32_t) * hc.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipMemcpyAsync(hh.data(), d.ghdr, sizeof(GameHdr) * G, hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    for (size_t g = 0; g < G; ++g) {
        if (board)
            for (int c = 0; c < d.ncells; ++c)
                board[g * d.ncells + c] = (int32_t)(hc[g * d.slots * 64 + c] & 3u);
        if (color) color[g] = hh[g].color - 1;                                    // hex.py:56
        if (result) result[g] = hh[g].winner ? (hh[g].winner == 2 ? 1 : 3) : 0;   // hex.py:161-170
        if (ply) ply[g] = hh[g].ply;
    }
    return AZX_OK;
}

extern "C" int azx_advance(azx_engine *e, const int32_t *move_ids) {
    if (!e || !move_ids) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    DevEngine &d = e->d;
    HIPCHECK(hipMemcpyAsync(e->moveids_dev, move_ids, sizeof(int32_t) * d.G, hipMemcpyHostToDevice, e->stream));
    azx_launch_advance(d, e->moveids_dev, 0, e->stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(e->stream));
    e->phase_api = SearchCursor();
    return AZX_OK;
}

extern "C" int azx_tree_dump(azx_engine *e, int slot, int cap, int32_t *parent, int32_t *first_child,
                             int32_t *num_children, float *num_visits, float *total_value,
                             float *prior_prob, int32_t *num_nodes, int32_t *root_id) {
    if (!e || !num_nodes || !root_id) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    DevEngine &d = e->d;
    if (slot < 0 || slot >= d.G) return fail(AZX_EINVAL, "slot %d out of range", slot);
    TreeHdr th;
    HIPCHECK(hipMemcpyAsync(&th, d.thdr + slot, sizeof th, hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    *num_nodes = th.num_nodes;
    *root_id = th.root_id;
    if (th.num_nodes > cap) return fail(AZX_EINVAL, "tree has %d nodes, caller capacity %d", th.num_nodes, cap);
    std::vector<Node> nodes(th.num_nodes);
    HIPCHECK(hipMemcpyAsync(nodes.data(), d.arena[th.arena] + (size_t)slot * d.cap,
                            sizeof(Node) * nodes.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    // rebuild the reference's six arrays (search_tree.py:48-55): parent and num_children are
    // implied by the layout (children of a k-move node are k consecutive ids, each with k-1)
    const int n = th.num_nodes;
    std::vector<int32_t> par(n, -1), kk(n, -1);
    kk[0] = th.k0;
    for (int v = 0; v < n; ++v) {
        const Node &nd = nodes[v];
        int fc = -1, nc = -1;
        if (nd.link >= 0) {
            fc = nd.link;
            nc = kk[v];
            for (int j = 0; j < nc && fc + j < n; ++j) { par[fc + j] = v; kk[fc + j] = nc - 1; }
        } else if (nd.link <= -2) {
            fc = -2 - nd.link;
            nc = 0;
        }
        if (first_child) first_child[v] = fc;
        if (num_children) num_children[v] = nc;
        if (num_visits) num_visits[v] = nd.nv;
        if (total_value) total_value[v] = nd.tv;
        if (prior_prob) prior_prob[v] = nd.pp;
    }
    if (parent) for (int v = 0; v < n; ++v) parent[v] = par[v];
    return AZX_OK;
}

extern "C" int azx_forward(azx_engine *e, int B, int K, const int32_t *boards,
                           const int32_t *legal_moves, float *value, float *moves_logprob) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    if (!e->net) return fail(AZX_ESTATE, "engine was not created with AZX_EVAL_RESNET");
    int rc = azx_net_forward_host(e->net, B, K, boards, legal_moves, value, moves_logprob, e->stream);
    if (rc) g_err = azx_net_error();
    return rc ? rc : check_net_range(e);
}

extern "C" int azx_hex_replay(int device, int board_size, int n_games, const int32_t *moves,
                              const int32_t *length, int stride, int32_t *result_out,
                              int32_t *nlegal_out, uint64_t *empties_out, int32_t *final_board) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(AZX_ENODEV, "no HIP device visible: the engine has no CPU fallback");
    if (board_size < 2 || board_size > AZX_MAX_BOARD) return fail(AZX_EINVAL, "bad board_size");
    if (n_games < 1 || stride < 1 || !moves || !length) return fail(AZX_EINVAL, "bad argument");
    DevGuard guard(device);
    if (azx_init_geometry(device)) return fail(AZX_EHIP, "uploading the board geometry tables failed");
    const int ncells = board_size * board_size;
    for (int g = 0; g < n_games; ++g) {
        if (length[g] < 0 || length[g] > stride) return fail(AZX_EINVAL, "length[%d] out of range", g);
        std::vector<char> used(ncells, 0);
        for (int p = 0; p < length[g]; ++p) {
            const int mv = moves[(size_t)g * stride + p];
            if (mv < 1 || mv > ncells || used[mv - 1]) return fail(AZX_EINVAL, "illegal move %d in game %d", mv, g);
            used[mv - 1] = 1;
        }
    }
    const size_t gs = (size_t)n_games * stride;
    int32_t *dm = nullptr, *dl = nullptr, *dr = nullptr, *dn = nullptr, *df = nullptr;
    uint64_t *de = nullptr;
    HIPCHECK(hipMalloc(&dm, sizeof(int32_t) * gs));
    HIPCHECK(hipMalloc(&dl, sizeof(int32_t) * n_games));
    HIPCHECK(hipMalloc(&dr, sizeof(int32_t) * gs));
    HIPCHECK(hipMalloc(&dn, sizeof(int32_t) * gs));
    HIPCHECK(hipMalloc(&de, sizeof(uint64_t) * gs * 4));
    HIPCHECK(hipMalloc(&df, sizeof(int32_t) * (size_t)n_games * ncells));
    HIPCHECK(hipMemset(dr, 0, sizeof(int32_t) * gs));
    HIPCHECK(hipMemset(dn, 0, sizeof(int32_t) * gs));
    HIPCHECK(hipMemset(de, 0, sizeof(uint64_t) * gs * 4));
    HIPCHECK(hipMemcpy(dm, moves, sizeof(int32_t) * gs, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dl, length, sizeof(int32_t) * n_games, hipMemcpyHostToDevice));
    azx_launch_hex_replay(board_size, n_games, dm, dl, stride, dr, dn, de, df, nullptr);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
    if (result_out) HIPCHECK(hipMemcpy(result_out, dr, sizeof(int32_t) * gs, hipMemcpyDeviceToHost));
    if (nlegal_out) HIPCHECK(hipMemcpy(nlegal_out, dn, sizeof(int32_t) * gs, hipMemcpyDeviceToHost));
    if (empties_out) HIPCHECK(hipMemcpy(empties_out, de, sizeof(uint64_t) * gs * 4, hipMemcpyDeviceToHost));
    if (final_board) HIPCHECK(hipMemcpy(final_board, df, sizeof(int32_t) * (size_t)n_games * ncells, hipMemcpyDeviceToHost));
    (void)hipFree(dm); (void)hipFree(dl); (void)hipFree(dr); (void)hipFree(dn); (void)hipFree(de); (void)hipFree(df);
    return AZX_OK;
}

// ---- which slots take part in the next searches (tournaments: only the games whose turn it is) --
extern "C" int azx_set_active(azx_engine *e, const int32_t *active) {
    if (!e || !active) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    DevEngine &d = e->d;
    std::vector<int32_t> a((size_t)d.G);
    for (int g = 0; g < d.G; ++g) a[g] = active[g] ? 1 : 0;
    HIPCHECK(hipMemcpy2DAsync(&d.ghdr[0].active, sizeof(GameHdr), a.data(), sizeof(int32_t), sizeof(int32_t),
                              (size_t)d.G, hipMemcpyHostToDevice, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

// ---- throughput mode ------------------------------------------------------------------------
static int play_setup(azx_engine *e, int64_t q_rows, int ring) {
    DevEngine &d = e->d;
    e->q_rows_valid = 0;
    if (!e->play_ready) {
        const size_t rows = (size_t)d.G * d.ncells;
        TRY(dev_alloc(e, &d.row_board, rows * AZX_CELL_STRIDE));
        TRY(dev_alloc(e, &d.row_prob, rows * AZX_CELL_STRIDE));
        TRY(dev_alloc(e, &d.row_k, rows));
        TRY(dev_alloc(e, &d.row_meta, rows * AZX_ROW_METRICS));
        e->play_ready = true;
    }
    if (q_rows > e->q_alloc) {
        (void)hipStreamSynchronize(e->stream);
        for (void *p : e->q_allocs) (void)hipFree(p);
        e->q_allocs.clear();
        e->q_alloc = 0;                                  // (nothing is held should one of the allocations below fail)
        auto qa = [&](void **p, size_t bytes) -> int {
            hipError_t err = hipMalloc(p, bytes);
            if (err != hipSuccess) return fail(AZX_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
            e->q_allocs.push_back(*p);
            return AZX_OK;
        };
        TRY(qa((void **)&d.q_board, (size_t)q_rows * AZX_CELL_STRIDE));
        TRY(qa((void **)&d.q_prob, (size_t)q_rows * AZX_CELL_STRIDE * sizeof(float)));
        TRY(qa((void **)&d.q_color, (size_t)q_rows * sizeof(int32_t)));
        TRY(qa((void **)&d.q_k, (size_t)q_rows * sizeof(int32_t)));
        TRY(qa((void **)&d.q_reward, (size_t)q_rows * sizeof(float)));
        TRY(qa((void **)&d.q_uid, (size_t)q_rows * sizeof(int64_t)));
        TRY(qa((void **)&d.q_meta, (size_t)q_rows * AZX_ROW_METRICS * sizeof(float)));
        e->q_alloc = q_rows;
    }
    d.q_cap = e->q_alloc;
    d.q_ring = ring;
    HIPCHECK(hipMemsetAsync(d.q_count, 0, sizeof(unsigned long long), e->stream));
    return AZX_OK;
}

struct CounterSnap {
    unsigned long long c[CTR_COUNT];
    double s[8];
};

static int snap_counters(azx_engine *e, CounterSnap *s) {
    const size_t G = e->d.G;
    std::vector<unsigned long long> hc(G * CTR_COUNT);
    std::vector<double> hs(G * 8);
    HIPCHECK(hipMemcpyAsync(hc.data(), e->d.counters, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipMemcpyAsync(hs.data(), e->d.stat_sums, hs.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    memset(s, 0, sizeof *s);
    for (size_t g = 0; g < G; ++g) {   // per-game accumulators (no device atomics): sum here
        for (int j = 0; j < CTR_COUNT; ++j) s->c[j] += hc[g * CTR_COUNT + j];
        for (int j = 0; j < 8; ++j) s->s[j] += hs[g * 8 + j];
    }
    return AZX_OK;
}

static void fill_stats(const CounterSnap &a, const CounterSnap &b, azx_play_stats *st) {
    st->games = (int64_t)(b.c[CTR_GAMES] - a.c[CTR_GAMES]);
    st->game_errors = (int64_t)(b.c[CTR_ERRORS] - a.c[CTR_ERRORS]);
    st->plies = (int64_t)(b.c[CTR_PLIES] - a.c[CTR_PLIES]);
    st->selects = (int64_t)(b.c[CTR_SELECTS] - a.c[CTR_SELECTS]);
    st->evals = (int64_t)(b.c[CTR_EVALS] - a.c[CTR_EVALS]);
    st->sum_depth = (int64_t)(b.c[CTR_SUM_DEPTH] - a.c[CTR_SUM_DEPTH]);
    st->sum_k_interior = (int64_t)(b.c[CTR_SUM_K_INT] - a.c[CTR_SUM_K_INT]);
    st->sum_k_leaf = (int64_t)(b.c[CTR_SUM_K_LEAF] - a.c[CTR_SUM_K_LEAF]);
    st->sum_search_value = b.s[0] - a.s[0];
    st->sum_root_width = b.s[1] - a.s[1];
    st->sum_action_logprob = b.s[2] - a.s[2];
    st->sum_reward_last = b.s[3] - a.s[3];
    st->sum_game_length = b.s[4] - a.s[4];
}

// `plies` moves of the resnet play loop as two half-pools (use_pipeline): half A on the engine stream, half B on
// stream_b.  Each half's phases follow each other on its own stream only; the host issues them phase by phase,
// alternating the halves, so that one half's tower is queued while the other half runs its search phases.  Half B
// starts after half A's first tree launch (everything queued on the engine stream before it included), about 0.15 ms
// behind: left alone, the halves' towers then start and end together phase after phase (two queues share the block
// slots about equally), and so do their tail rounds, heads and tree launches.
// The stagger (default; AZX_PIPELINE_STAGGER=0 leaves the start as above): in every move, half B's phase-1 evaluation
// waits until the first `split` rows -- half -- of half A's phase-1 evaluation are done.  Phase 1's is a move's first
// evaluation with a full batch of leaves (phase 0 evaluates fresh roots only: at most one row per game, none for a root
// kept from the last move).  Half A's is issued as two launches, rows [0, split) and [split, rows), with the event
// between them; every other phase is one launch per half.  The halves' towers then run about half a phase period
// apart: one half's tail round, heads and tree launch fall into the middle of the other half's tower,
// which has thousands of blocks waiting.  A half that is already further behind does not wait at all.
// The engine stream waits for half B at the end.
static int enqueue_plies_pipelined(azx_engine *e, int64_t plies) {
    TRY(pipeline_streams(e));
    if (!azx_net_ready(e->net)) return fail(AZX_ESTATE, "azx_set_weights has not been called");
    const DevEngine &d = e->d;
    const int half = d.G / 2, rows = half * d.bs;
    const DevEngine hv[2] = {pool_view(d, 0, half, d.n_eval), pool_view(d, half, half, d.n_eval + 1)};
    const hipStream_t hs[2] = {e->stream, e->stream_b};
    const int nb = e->num_batches;
    const int split = rows / 2 / AZX_NET_ROW_ALIGN * AZX_NET_ROW_ALIGN;     // whole blocks of every tower and heads kernel
    const bool stagger = e->stagger && split > 0;
    // the launch statistics count one phase's two half-pool launches as one launch of the whole pool
    const int ref = time_mark(e, hs[0]);
    for (int64_t p = 0; p < plies; ++p) {
        // every phase's tree launch, followed by the half's network evaluation or, after the last, by the move
        for (int ph = 0; ph <= nb + 1; ++ph) {
            const bool then_eval = phase_mode(ph, nb).then_eval;
            const int g_tree = ++e->ev_groups, g_net = then_eval ? ++e->ev_groups : 0;
            for (int h = 0; h < 2; ++h) {
                TRY(enqueue_tree_phase(e, {&hv[h], hs[h], true, g_tree, ref}, ph));
                if (!then_eval) {
                    azx_launch_choose(hv[h], hs[h]);
                    azx_launch_advance(hv[h], nullptr, 1, hs[h]);
                    continue;
                }
                if (p == 0 && ph == 0 && h == 0) {
                    HIPCHECK(hipEventRecord(e->ev_fork, hs[0]));
                    HIPCHECK(hipStreamWaitEvent(hs[1], e->ev_fork, 0));
                }
                const bool cut = stagger && ph == 1;
                if (cut && h == 1) HIPCHECK(hipStreamWaitEvent(hs[1], e->ev_stagger, 0));   // (recorded just below, for h == 0)
                time_begin(e, 1, hs[h], g_net, ref);
                azx_net_eval_rows(e->net, hv[h], h * rows, cut && h == 0 ? split : rows, hs[h]);
                time_end(e, 1, hs[h]);
                if (cut && h == 0) {
                    HIPCHECK(hipEventRecord(e->ev_stagger, hs[0]));
                    time_begin(e, 1, hs[h], g_net, ref);        // (the same group: the phase still counts as one launch)
                    azx_net_eval_rows_behind(e->net, hv[h], h * rows, split, rows, e->stagger_ctr, hs[h]);
                    time_end(e, 1, hs[h]);
                }
            }
        }
    }
    HIPCHECK(hipEventRecord(e->ev_join, hs[1]));
    HIPCHECK(hipStreamWaitEvent(hs[0], e->ev_join, 0));
    return AZX_OK;
}

// `want` plies on the engine's stream(s), by the first way of three that applies.  The uniform-evaluator path plays
// the moves in persistent launches (k_play), at most `chunk_cap` moves each; its time is booked per move like the
// per-move launches'.  Otherwise the two half-pools or per-move launches play the rest, at most `else_plies` of it.
// *enqueued: how many plies are on the stream.
static int enqueue_plies(azx_engine *e, int64_t want, int chunk_cap, int64_t else_plies, int64_t *enqueued) {
    int64_t p = 0;
    while (p < want) {
        const int n = (int)std::min<int64_t>(chunk_cap, want - p);
        time_begin(e);
        if (!azx_launch_play(e->d, e->num_batches, n, e->stream, !e->force_generic && !e->no_persistent)) break;
        time_end(e, n);                     // (a begin event without its end is simply overwritten by the next one)
        p += n;
    }
    if (p < want) {
        const int64_t rest = std::min(else_plies, want - p);
        if (use_pipeline(e)) TRY(enqueue_plies_pipelined(e, rest));
        else for (int64_t i = 0; i < rest; ++i) {
            TRY(enqueue_search(e, true));
            azx_launch_choose(e->d, e->stream);
            azx_launch_advance(e->d, nullptr, 1, e->stream);
        }
        p += rest;
    }
    *enqueued = p;
    return AZX_OK;
}

// One throughput self-play call from the first thing it puts on the device to its stats.  The scope hands the launches
// the engine's self-play options; the two events take the call's wall time on the engine stream and are released on
// every way out, an early error return included.  The caller sets the harvest queue up (play_setup) between the
// construction and begin().
struct PlayRun {
    azx_engine *e;
    SelfplayScope scope;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    CounterSnap before;
    explicit PlayRun(azx_engine *e_) : e(e_), scope(e_) {}
    ~PlayRun() { for (hipEvent_t ev : {t0, t1}) if (ev) (void)hipEventDestroy(ev); }

    int begin() {
        TRY(upload_noise(e, nullptr, 0, 0, e->cfg.noise_scale));
        TRY(snap_counters(e, &before));
        HIPCHECK(hipEventCreate(&t0));
        HIPCHECK(hipEventCreate(&t1));
        HIPCHECK(hipEventRecord(t0, e->stream));
        // slots parked by an earlier azx_play* call rejoin: games that finished while the queue was full hand their
        // rows over first (a ring queue always has room)
        azx_launch_advance(e->d, nullptr, 2, e->stream);
        return AZX_OK;
    }

    // `positions`: the rows the caller counted, or -1 for the rows the games' counters saw
    int finish(azx_play_stats *stats, int64_t positions) {
        HIPCHECK(hipEventRecord(t1, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
        float ms = 0.f;
        HIPCHECK(hipEventElapsedTime(&ms, t0, t1));
        CounterSnap after;
        TRY(snap_counters(e, &after));
        fill_stats(before, after, stats);
        stats->positions = positions >= 0 ? positions : (int64_t)(after.c[CTR_ROWS] - before.c[CTR_ROWS]);
        stats->seconds = ms * 1e-3;
        time_collect(e, stats);
        return search_outcome(e);
    }
};

extern "C" int azx_play_steps(azx_engine *e, int64_t plies, azx_play_stats *stats) {
    if (!e || !stats) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(ext_refuse(e));
    if (e->d.evaluator == AZX_EVAL_EXTERNAL && !ext_registered(e))
        return fail(AZX_ESTATE, "play mode needs a device evaluator");
    memset(stats, 0, sizeof *stats);
    PlayRun run(e);
    TRY(play_setup(e, std::max<int64_t>(e->q_alloc, 1 << 16), 1));
    TRY(run.begin());
    const int PLAY_CHUNK = 256;
    int64_t done = 0;
    TRY(enqueue_plies(e, plies, PLAY_CHUNK, plies, &done));
    HIPCHECK(hipGetLastError());
    return run.finish(stats, -1);
}

// play whole games into the harvest queue until it holds >= min_positions rows
static int play_until(azx_engine *e, int64_t min_positions, int64_t max_plies, azx_play_stats *stats,
                      unsigned long long *rows_out) {
    DevEngine &d = e->d;
    memset(stats, 0, sizeof *stats);
    PlayRun run(e);
    const int64_t worst = min_positions + (int64_t)d.G * d.ncells;
    TRY(play_setup(e, worst, 0));
    if (e->dbg_qcap > 0)                                // tests (azx_debug_set_queue_cap): a queue too small, so that slots get parked
        d.q_cap = std::max<int64_t>(1, std::min<int64_t>(d.q_cap, e->dbg_qcap));
    TRY(run.begin());
    unsigned long long rows = 0;
    for (int64_t p = 0; (max_plies <= 0 || p < max_plies) && (int64_t)rows < min_positions;) {
        // with the uniform evaluator a few moves per persistent launch (k_play) between looks at the
        // queue; Player.read may return more than it was asked for anyway (whole games only)
        // (at most 2N - 1 moves, the shortest possible game: a slot then finishes at most one game
        // per launch and the queue bound min_positions + n_games * cells still holds); else one move per look
        const int64_t most = std::min<int64_t>(8, 2 * d.N - 1);
        const int chunk = (int)std::min<int64_t>(most, max_plies > 0 ? max_plies - p : most);
        int64_t done = 0;
        TRY(enqueue_plies(e, chunk, chunk, 1, &done));
        p += done;
        HIPCHECK(hipMemcpyAsync(&rows, d.q_count, sizeof rows, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
        // a bounded queue (azx_debug_set_queue_cap) below min_positions parks every slot sooner or later: with
        // no slot left to play, return what the queue holds instead of spinning
        if (e->dbg_qcap > 0 && (p & 7) == 0) {
            std::vector<GameHdr> hh((size_t)d.G);
            HIPCHECK(hipMemcpyAsync(hh.data(), d.ghdr, sizeof(GameHdr) * hh.size(), hipMemcpyDeviceToHost, e->stream));
            HIPCHECK(hipStreamSynchronize(e->stream));
            bool any = false;
            for (const GameHdr &h : hh) any = any || h.active;
            if (!any) break;
        }
    }
    TRY(run.finish(stats, (int64_t)rows));
    *rows_out = rows;
    e->q_rows_valid = (int64_t)rows;
    return AZX_OK;
}

// rows [first, first + n) of the harvest queue to the host in azx_play's layout (any pointer may be null): widen /
// densify on the device (k_rows_export), then one copy per output array
static int rows_read(azx_engine *e, int64_t first, int64_t n_rows, int32_t *board, int32_t *color, int32_t *nlegal,
                     float *moves_prob, float *reward, int64_t *game_uid) {
    if (n_rows == 0) return AZX_OK;
    DevEngine &d = e->d;
    const size_t n = (size_t)n_rows, f = (size_t)first;
    if (board || moves_prob) {
        const size_t need = n * d.ncells;
        if (need > e->export_cap) {
            (void)hipStreamSynchronize(e->stream);
            if (e->export_board) (void)hipFree(e->export_board);
            if (e->export_prob) (void)hipFree(e->export_prob);
            e->export_board = nullptr; e->export_prob = nullptr; e->export_cap = 0;
            if (hipMalloc((void **)&e->export_board, need * sizeof(int32_t)) != hipSuccess ||
                hipMalloc((void **)&e->export_prob, need * sizeof(float)) != hipSuccess)
                return fail(AZX_ENOMEM, "hipMalloc of the export staging (%zu rows) failed", n);
            e->export_cap = need;
        }
        azx_launch_rows_export(d.q_board + f * AZX_CELL_STRIDE, d.q_prob + f * AZX_CELL_STRIDE, (long long)n, d.ncells,
                               e->export_board, e->export_prob, e->stream);
        HIPCHECK(hipGetLastError());
        if (board) HIPCHECK(hipMemcpyAsync(board, e->export_board, need * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        if (moves_prob) HIPCHECK(hipMemcpyAsync(moves_prob, e->export_prob, need * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    }
    if (color) HIPCHECK(hipMemcpyAsync(color, d.q_color + f, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (nlegal) HIPCHECK(hipMemcpyAsync(nlegal, d.q_k + f, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (reward) HIPCHECK(hipMemcpyAsync(reward, d.q_reward + f, n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (game_uid) HIPCHECK(hipMemcpyAsync(game_uid, d.q_uid + f, n * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

extern "C" int azx_play(azx_engine *e, int64_t min_positions, int64_t max_plies, int64_t cap,
                        int32_t *board, int32_t *color, int32_t *nlegal, float *moves_prob,
                        float *reward, int64_t *game_uid, azx_play_stats *stats) {
    if (!e || !stats) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(ext_refuse(e));
    if (e->d.evaluator == AZX_EVAL_EXTERNAL && !ext_registered(e))
        return fail(AZX_ESTATE, "play mode needs a device evaluator");
    DevEngine &d = e->d;
    const int64_t worst = min_positions + (int64_t)d.G * d.ncells;
    if (cap < worst)
        return fail(AZX_EINVAL, "cap %lld < min_positions + n_games*cells = %lld (whole games only)",
                    (long long)cap, (long long)worst);
    unsigned long long rows = 0;
    TRY(play_until(e, min_positions, max_plies, stats, &rows));
    return rows_read(e, 0, (int64_t)rows, board, color, nlegal, moves_prob, reward, game_uid);
}

extern "C" int azx_play_device(azx_engine *e, int64_t min_positions, int64_t max_plies, int64_t *rows_out,
                               azx_play_stats *stats) {
    if (!e || !stats || !rows_out) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(ext_refuse(e));
    if (e->d.evaluator == AZX_EVAL_EXTERNAL && !ext_registered(e))
        return fail(AZX_ESTATE, "play mode needs a device evaluator");
    unsigned long long rows = 0;
    TRY(play_until(e, min_positions, max_plies, stats, &rows));
    *rows_out = (int64_t)rows;
    return AZX_OK;
}

extern "C" int azx_play_row_metrics(azx_engine *e, int64_t cap, float *metrics, int64_t *n_out) {
    if (!e || !metrics || !n_out) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    const int64_t n = e->q_rows_valid;
    if (n > cap) return fail(AZX_EINVAL, "%lld rows queued, caller capacity %lld", (long long)n, (long long)cap);
    *n_out = n;
    if (n == 0) return AZX_OK;
    HIPCHECK(hipMemcpyAsync(metrics, e->d.q_meta, (size_t)n * AZX_ROW_METRICS * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

extern "C" int azx_rows_read(azx_engine *e, int64_t first, int64_t n, int32_t *board, int32_t *color, int32_t *nlegal,
                             float *moves_prob, float *reward, int64_t *game_uid) {
    if (!e) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    if (first < 0 || n < 0 || first + n > e->q_rows_valid)
        return fail(AZX_EINVAL, "rows [%lld, %lld) outside the %lld rows queued", (long long)first,
                    (long long)(first + n), (long long)e->q_rows_valid);
    return rows_read(e, first, n, board, color, nlegal, moves_prob, reward, game_uid);
}

extern "C" int azx_rows_pack(azx_engine *e, int64_t first, int64_t n, void *records_dev) {
    if (!e || (n > 0 && !records_dev)) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    if (first < 0 || n < 0 || first + n > e->q_rows_valid)
        return fail(AZX_EINVAL, "rows [%lld, %lld) outside the %lld rows queued", (long long)first,
                    (long long)(first + n), (long long)e->q_rows_valid);
    if (n == 0) return AZX_OK;
    DevEngine &d = e->d;
    const ReplayRows src = {d.q_board, d.q_prob, d.q_color, d.q_k, d.q_reward};
    azx_launch_rows_pack(src, (const long long *)d.q_uid, first, n, d.ncells, (uint8_t *)records_dev, e->stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

extern "C" int azx_replay_put_records(azx_engine *e, int64_t n, const void *records_dev) {
    if (!e || (n > 0 && !records_dev)) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    if (e->ring_cap == 0) return fail(AZX_ESTATE, "no replay ring: call azx_replay_create first");
    if (n < 0) return fail(AZX_EINVAL, "n must be >= 0");
    if (n == 0) return AZX_OK;
    azx_launch_records_put((const uint8_t *)records_dev, e->ring, n, e->ring_cap, e->ring_write, e->d.ncells, e->stream);
    HIPCHECK(hipGetLastError());
    e->ring_write = (e->ring_write + n) % e->ring_cap;
    e->ring_size = std::min<int64_t>(e->ring_cap, e->ring_size + n);
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

extern "C" int azx_replay_put_records_async(azx_engine *e, int64_t n, const void *records_dev, void *hip_stream) {
    if (!e || (n > 0 && !records_dev)) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    if (e->ring_cap == 0) return fail(AZX_ESTATE, "no replay ring: call azx_replay_create first");
    if (n < 0) return fail(AZX_EINVAL, "n must be >= 0");
    if (n == 0) return AZX_OK;
    // only ring state and the caller's stream: nothing the play thread (azx_play_device on e->stream) touches
    azx_launch_records_put((const uint8_t *)records_dev, e->ring, n, e->ring_cap, e->ring_write, e->d.ncells, (hipStream_t)hip_stream);
    HIPCHECK(hipGetLastError());
    e->ring_write = (e->ring_write + n) % e->ring_cap;
    e->ring_size = std::min<int64_t>(e->ring_cap, e->ring_size + n);
    return AZX_OK;
}

// ---- device-resident replay ring: ReplayBuffer.put FIFO (replay_buffer.py:134-149) and the
// prep.batch_replays collate (prep.py:24-39) without leaving HBM ---------------------------------
extern "C" int azx_replay_create(azx_engine *e, int64_t capacity) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    if (capacity < 1) return fail(AZX_EINVAL, "capacity must be >= 1");
    (void)hipStreamSynchronize(e->stream);
    for (void *p : e->ring_allocs) (void)hipFree(p);
    e->ring_allocs.clear();
    e->ring_cap = e->ring_size = e->ring_write = 0;
    e->ring_idx = nullptr;
    e->ring_idx_cap = 0;
    auto ra = [&](void **p, size_t bytes) -> int {
        hipError_t err = hipMalloc(p, bytes);
        if (err != hipSuccess) return fail(AZX_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
        e->ring_allocs.push_back(*p);
        return AZX_OK;
    };
    TRY(ra((void **)&e->ring.board, (size_t)capacity * AZX_CELL_STRIDE));
    TRY(ra((void **)&e->ring.prob, (size_t)capacity * AZX_CELL_STRIDE * sizeof(float)));
    TRY(ra((void **)&e->ring.color, (size_t)capacity * sizeof(int32_t)));
    TRY(ra((void **)&e->ring.k, (size_t)capacity * sizeof(int32_t)));
    TRY(ra((void **)&e->ring.reward, (size_t)capacity * sizeof(float)));
    TRY(ra((void **)&e->ring_maxk, sizeof(int32_t)));
    e->ring_cap = capacity;
    return AZX_OK;
}

extern "C" int azx_replay_state(azx_engine *e, int64_t *capacity, int64_t *size, int64_t *write_idx) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    if (capacity) *capacity = e->ring_cap;
    if (size) *size = e->ring_size;
    if (write_idx) *write_idx = e->ring_write;
    return AZX_OK;
}

extern "C" int azx_replay_set_state(azx_engine *e, int64_t size, int64_t write_idx) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    if (e->ring_cap == 0) return fail(AZX_ESTATE, "no replay ring: call azx_replay_create first");
    if (size < 0 || size > e->ring_cap || write_idx < 0 || write_idx >= e->ring_cap)
        return fail(AZX_EINVAL, "size/write_idx outside the ring");
    e->ring_size = size;
    e->ring_write = write_idx;
    return AZX_OK;
}

// rows [0, n) of `src` enter the ring in order, oldest rows overwritten first
static int ring_put(azx_engine *e, const ReplayRows &src, int64_t n) {
    azx_launch_replay_put(src, e->ring, n, e->ring_cap, e->ring_write, e->stream);
    HIPCHECK(hipGetLastError());
    e->ring_write = (e->ring_write + n) % e->ring_cap;
    e->ring_size = std::min<int64_t>(e->ring_cap, e->ring_size + n);
    return AZX_OK;
}

extern "C" int azx_replay_put(azx_engine *e, int64_t n, const int32_t *board, const int32_t *color,
                              const int32_t *nlegal, const float *moves_prob, const float *reward) {
    if (!e || !board || !color || !nlegal || !moves_prob || !reward) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    if (e->ring_cap == 0) return fail(AZX_ESTATE, "no replay ring: call azx_replay_create first");
    if (n < 0) return fail(AZX_EINVAL, "n must be >= 0");
    if (n == 0) return AZX_OK;
    DevEngine &d = e->d;
    // stage through the harvest queue buffers (same row format)
    TRY(play_setup(e, n, 0));
    std::vector<uint8_t> hb((size_t)n * AZX_CELL_STRIDE, 0);
    std::vector<float> hp((size_t)n * AZX_CELL_STRIDE, 0.0f);
    for (int64_t r = 0; r < n; ++r) {
        if (nlegal[r] < 0 || nlegal[r] > d.ncells) return fail(AZX_EINVAL, "row %lld: nlegal out of range", (long long)r);
        for (int c = 0; c < d.ncells; ++c) {
            const int32_t v = board[r * d.ncells + c];
            if (v < 0 || v > 2) return fail(AZX_EINVAL, "row %lld: cell value %d", (long long)r, v);
            hb[r * AZX_CELL_STRIDE + c] = (uint8_t)v;
        }
        for (int c = 0; c < nlegal[r]; ++c) hp[r * AZX_CELL_STRIDE + c] = moves_prob[r * d.ncells + c];
    }
    HIPCHECK(hipMemcpyAsync(d.q_board, hb.data(), hb.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHECK(hipMemcpyAsync(d.q_prob, hp.data(), hp.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHECK(hipMemcpyAsync(d.q_color, color, n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHECK(hipMemcpyAsync(d.q_k, nlegal, n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHECK(hipMemcpyAsync(d.q_reward, reward, n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    const ReplayRows src = {d.q_board, d.q_prob, d.q_color, d.q_k, d.q_reward};
    TRY(ring_put(e, src, n));
    HIPCHECK(hipStreamSynchronize(e->stream));   // the host staging vectors die here
    return AZX_OK;
}

extern "C" int azx_replay_fill(azx_engine *e, int64_t min_positions, int64_t max_plies,
                               int64_t *rows_out, azx_play_stats *stats) {
    if (!e || !stats) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    if (e->ring_cap == 0) return fail(AZX_ESTATE, "no replay ring: call azx_replay_create first");
    TRY(ext_refuse(e));
    if (e->d.evaluator == AZX_EVAL_EXTERNAL && !ext_registered(e))
        return fail(AZX_ESTATE, "play mode needs a device evaluator");
    unsigned long long rows = 0;
    TRY(play_until(e, min_positions, max_plies, stats, &rows));
    DevEngine &d = e->d;
    const ReplayRows src = {d.q_board, d.q_prob, d.q_color, d.q_k, d.q_reward};
    if (rows) TRY(ring_put(e, src, (int64_t)rows));
    HIPCHECK(hipStreamSynchronize(e->stream));
    if (rows_out) *rows_out = (int64_t)rows;
    return AZX_OK;
}

// azx_replay_set_reflect: the key of this collate's row bits -- (seed, collates since the seed was set), nothing of
// the ring -- and the count moves on, for the blocking and the enqueued collate alike
static unsigned long long reflect_key(azx_engine *e) {
    if (!e->ring_reflect) return 0ull;
    return azx_mix64(azx_mix64(e->ring_reflect_seed ^ 0x5245464C45435421ull) + e->ring_reflect_count++);
}

extern "C" int azx_replay_collate(azx_engine *e, int64_t batch, const int64_t *indices, int64_t *color_dev,
                                  int32_t *legal_moves_dev, int64_t *result_dev, int32_t *board_dev,
                                  float *moves_prob_dev, float *reward_dev, int32_t *max_k_out) {
    if (!e || !indices || !color_dev || !legal_moves_dev || !result_dev || !board_dev || !moves_prob_dev ||
        !reward_dev || !max_k_out)
        return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    if (e->ring_cap == 0) return fail(AZX_ESTATE, "no replay ring: call azx_replay_create first");
    if (batch < 1 || batch > (1 << 24)) return fail(AZX_EINVAL, "batch outside [1, 2^24]");
    for (int64_t b = 0; b < batch; ++b)
        if (indices[b] < 0 || indices[b] >= e->ring_size)
            return fail(AZX_EINVAL, "index %lld outside the %lld rows held", (long long)indices[b], (long long)e->ring_size);
    if (batch > e->ring_idx_cap) {
        void *p = nullptr;
        hipError_t err = hipMalloc(&p, (size_t)batch * sizeof(long long));
        if (err != hipSuccess) return fail(AZX_ENOMEM, "hipMalloc failed: %s", hipGetErrorString(err));
        if (e->ring_idx) {                 // blocking calls: no kernel still reads the old index buffer
            (void)hipFree(e->ring_idx);
            e->ring_allocs.erase(std::remove(e->ring_allocs.begin(), e->ring_allocs.end(), (void *)e->ring_idx),
                                 e->ring_allocs.end());
        }
        e->ring_allocs.push_back(p);
        e->ring_idx = (long long *)p;
        e->ring_idx_cap = batch;
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "index width");
    HIPCHECK(hipMemcpyAsync(e->ring_idx, indices, (size_t)batch * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
    HIPCHECK(hipMemsetAsync(e->ring_maxk, 0, sizeof(int32_t), e->stream));
    azx_launch_replay_collate(e->ring, e->ring_idx, (int)batch, e->d.ncells, (long long *)color_dev,
                              legal_moves_dev, (long long *)result_dev, board_dev, moves_prob_dev, reward_dev,
                              e->ring_maxk, e->ring_mover_view ? e->d.N : 0, e->ring_reflect ? 1 : 0,
                              reflect_key(e), e->stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(max_k_out, e->ring_maxk, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

// The same collate, enqueued on the CALLER's stream and not synchronised (no max_k: the consumer takes full-width
// rows): for a trainer whose step runs on that stream (azx_train_step) -- the host queues collate + step and moves on.
extern "C" int azx_replay_set_mover_view(azx_engine *e, int on) {
    if (!e) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    e->ring_mover_view = on != 0;
    return AZX_OK;
}

extern "C" int azx_replay_set_reflect(azx_engine *e, int on, uint64_t seed) {
    if (!e) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    e->ring_reflect = on != 0;
    e->ring_reflect_seed = seed;
    e->ring_reflect_count = 0;
    return AZX_OK;
}

// The sampled indices are staged through a small ring of pinned buffers; a slot is re-used only after the collate that
// read it has run (one event per slot).  The caller orders ring WRITES (azx_replay_fill / put, which are blocking calls
// on the engine's stream) after these reads by synchronising its stream before a refill.
extern "C" int azx_replay_collate_async(azx_engine *e, int64_t batch, const int64_t *indices, int64_t *color_dev,
                                        int32_t *legal_moves_dev, int64_t *result_dev, int32_t *board_dev,
                                        float *moves_prob_dev, float *reward_dev, void *hip_stream) {
    if (!e || !indices || !color_dev || !legal_moves_dev || !result_dev || !board_dev || !moves_prob_dev || !reward_dev)
        return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    if (e->ring_cap == 0) return fail(AZX_ESTATE, "no replay ring: call azx_replay_create first");
    if (batch < 1 || batch > (1 << 20)) return fail(AZX_EINVAL, "batch outside [1, 2^20]");
    for (int64_t b = 0; b < batch; ++b)
        if (indices[b] < 0 || indices[b] >= e->ring_size)
            return fail(AZX_EINVAL, "index %lld outside the %lld rows held", (long long)indices[b], (long long)e->ring_size);
    hipStream_t st = (hipStream_t)hip_stream;
    if (batch > e->cidx_cap) {
        for (int i = 0; i < 8; ++i) {
            if (e->cidx_ev[i]) HIPCHECK(hipEventSynchronize(e->cidx_ev[i]));
            if (e->cidx_host[i]) (void)hipHostFree(e->cidx_host[i]);
            if (e->cidx_dev[i]) (void)hipFree(e->cidx_dev[i]);
            e->cidx_host[i] = e->cidx_dev[i] = nullptr;
            if (hipHostMalloc((void **)&e->cidx_host[i], (size_t)batch * sizeof(long long)) != hipSuccess ||
                hipMalloc((void **)&e->cidx_dev[i], (size_t)batch * sizeof(long long)) != hipSuccess)
                return fail(AZX_ENOMEM, "allocating the collate index ring failed");
            if (!e->cidx_ev[i]) HIPCHECK(hipEventCreateWithFlags(&e->cidx_ev[i], hipEventDisableTiming));
        }
        if (!e->cidx_maxk) TRY(dev_alloc(e, &e->cidx_maxk, 4));
        e->cidx_cap = batch;
    }
    const int slot = (int)(e->cidx_next++ % 8);
    HIPCHECK(hipEventSynchronize(e->cidx_ev[slot]));          // returns at once for a slot never used
    memcpy(e->cidx_host[slot], indices, (size_t)batch * sizeof(int64_t));
    HIPCHECK(hipMemcpyAsync(e->cidx_dev[slot], e->cidx_host[slot], (size_t)batch * sizeof(int64_t), hipMemcpyHostToDevice, st));
    azx_launch_replay_collate(e->ring, e->cidx_dev[slot], (int)batch, e->d.ncells, (long long *)color_dev,
                              legal_moves_dev, (long long *)result_dev, board_dev, moves_prob_dev, reward_dev,
                              e->cidx_maxk, e->ring_mover_view ? e->d.N : 0, e->ring_reflect ? 1 : 0,
                              reflect_key(e), st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipEventRecord(e->cidx_ev[slot], st));
    return AZX_OK;
}

// ---- float32 arithmetic self-test hook (tests): IEEE sqrt/divide and no FMA contraction ----
extern "C" int azx_selftest_arith(int device, int n, const float *a, const float *b, float *sq,
                                  float *dv, float *mul) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(AZX_ENODEV, "no HIP device visible");
    DevGuard guard(device);
    float *da, *db, *ds, *dd, *dm;
    HIPCHECK(hipMalloc(&da, n * 4)); HIPCHECK(hipMalloc(&db, n * 4)); HIPCHECK(hipMalloc(&ds, n * 4));
    HIPCHECK(hipMalloc(&dd, n * 4)); HIPCHECK(hipMalloc(&dm, n * 4));
    HIPCHECK(hipMemcpy(da, a, n * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(db, b, n * 4, hipMemcpyHostToDevice));
    azx_launch_arith(da, db, ds, dd, dm, n, nullptr);
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(sq, ds, n * 4, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(dv, dd, n * 4, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(mul, dm, n * 4, hipMemcpyDeviceToHost));
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(ds); (void)hipFree(dd); (void)hipFree(dm);
    return AZX_OK;
}

// ---- self-test hook (tests): the search kernel's unscaled divide and sqrt table ----------------
extern "C" int azx_selftest_divide(int device, int n, const float *num, const float *den, float *quot,
                                   float *sqrt_tab) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(AZX_ENODEV, "no HIP device visible");
    if (n < 1 || !num || !den || !quot || !sqrt_tab) return fail(AZX_EINVAL, "bad argument");
    DevGuard guard(device);
    if (azx_init_geometry(device)) return fail(AZX_EHIP, "uploading the constant tables failed");
    float *da, *db, *dq, *dr;
    HIPCHECK(hipMalloc(&da, n * 4)); HIPCHECK(hipMalloc(&db, n * 4));
    HIPCHECK(hipMalloc(&dq, n * 4)); HIPCHECK(hipMalloc(&dr, n * 4));
    HIPCHECK(hipMemcpy(da, num, n * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(db, den, n * 4, hipMemcpyHostToDevice));
    azx_launch_divide_test(da, db, dq, dr, n, nullptr);
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(quot, dq, n * 4, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(sqrt_tab, dr, n * 4, hipMemcpyDeviceToHost));
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dq); (void)hipFree(dr);
    return AZX_OK;
}

// ---- device Dirichlet self-test hook (tests): n_rows draws of Dirichlet(alpha * 1_k) -------------
extern "C" int azx_selftest_dirichlet(int device, double alpha, int k, int n_rows, uint32_t seed, float *out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(AZX_ENODEV, "no HIP device visible");
    if (k < 1 || k > 128 || n_rows < 1 || !out) return fail(AZX_EINVAL, "bad argument");
    DevGuard guard(device);
    float *d = nullptr;
    HIPCHECK(hipMalloc(&d, sizeof(float) * (size_t)k * n_rows));
    if (!(alpha > 0.0)) return fail(AZX_EINVAL, "alpha must be positive");
    std::vector<float> tab(AZX_GAMMA_TAB_FLOATS);
    azx_gamma_table(alpha, tab.data());
    float *dt = nullptr;
    HIPCHECK(hipMalloc(&dt, tab.size() * sizeof(float)));
    HIPCHECK(hipMemcpy(dt, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    azx_launch_noise_test((float)alpha, dt, k, n_rows, seed, d, nullptr);
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(out, d, sizeof(float) * (size_t)k * n_rows, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    (void)hipFree(dt);
    return AZX_OK;
}

extern "C" int azx_debug_choose(azx_engine *e, int32_t *move_id, float *moves_prob) {
    if (!e || !move_id || !moves_prob) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    DevEngine &d = e->d;
    TRY(play_setup(e, std::max<int64_t>(e->q_alloc, 1 << 10), 1));
    std::vector<GameHdr> before(d.G), after(d.G);
    HIPCHECK(hipMemcpyAsync(before.data(), d.ghdr, sizeof(GameHdr) * d.G, hipMemcpyDeviceToHost, e->stream));
    azx_launch_choose(d, e->stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(after.data(), d.ghdr, sizeof(GameHdr) * d.G, hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    std::vector<float> row(AZX_CELL_STRIDE);
    for (int g = 0; g < d.G; ++g) {
        const bool drew = after[g].n_rows == before[g].n_rows + 1;
        move_id[g] = drew ? after[g].move_id : -1;
        float *out = moves_prob + (size_t)g * d.ncells;
        if (!drew) { std::fill(out, out + d.ncells, 0.0f); continue; }
        HIPCHECK(hipMemcpyAsync(row.data(), d.row_prob + ((size_t)g * d.ncells + before[g].n_rows) * AZX_CELL_STRIDE,
                                sizeof(float) * AZX_CELL_STRIDE, hipMemcpyDeviceToHost, e->stream));
        HIPCHECK(hipStreamSynchronize(e->stream));
        std::copy(row.begin(), row.begin() + d.ncells, out);
    }
    return AZX_OK;
}

// ---- the options' statistics: [G][count] accumulators per game (no device atomics), summed over the games here ----
static int sum_game_counters(azx_engine *e, const unsigned long long *ctr, int count, int64_t *out, int n_out) {
    const size_t G = e->d.G;
    std::vector<unsigned long long> hc(G * count);
    HIPCHECK(hipMemcpyAsync(hc.data(), ctr, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    std::fill(out, out + n_out, (int64_t)0);
    for (size_t g = 0; g < G; ++g)
        for (int j = 0; j < count && j < n_out; ++j) out[j] += (int64_t)hc[g * count + j];
    return AZX_OK;
}

// ... and zeroed, with the stream waited for, at the top of the option's setter
static int zero_game_counters(azx_engine *e, unsigned long long *ctr, int count) {
    HIPCHECK(hipMemsetAsync(ctr, 0, (size_t)e->d.G * count * sizeof(unsigned long long), e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

// ---- playout cap randomisation (include/azx.h; NOT the reference's behaviour) ---------------
extern "C" int azx_playout_cap_is_full(uint64_t seed, int64_t uid, int ply, double full_prob) {
    if (!(full_prob > 0.0 && full_prob <= 1.0)) return fail(AZX_EINVAL, "full_prob %g outside (0, 1]", full_prob);
    if (ply < 0) return fail(AZX_EINVAL, "ply %d is negative", ply);
    return azx_cap_is_full(seed, uid, ply, azx_cap_threshold_m1(full_prob)) ? 1 : 0;
}

extern "C" int azx_set_playout_cap(azx_engine *e, double full_prob, int fast_simulations) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    if (!(full_prob > 0.0 && full_prob <= 1.0))
        return fail(AZX_EINVAL, "playout cap: full_prob %g outside (0, 1]", full_prob);
    const bool named_clear = full_prob == 1.0 && fast_simulations == 0;
    if (!named_clear && (fast_simulations < 1 || fast_simulations > e->cfg.simulations))
        return fail(AZX_EINVAL, "playout cap: fast_simulations %d outside [1, simulations = %d] (0 with full_prob 1 clears the cap)",
                    fast_simulations, e->cfg.simulations);
    ENGINE_GUARD(e);
    CounterSnap now;
    TRY(snap_counters(e, &now));
    e->opt.cap_on = !(named_clear || (full_prob == 1.0 && fast_simulations == e->cfg.simulations));
    e->opt.cap_full_prob = e->opt.cap_on ? full_prob : 1.0;
    e->opt.cap_fast_sims = e->opt.cap_on ? fast_simulations : 0;
    e->cap_base[0] = now.c[CTR_CAP_FULL];
    e->cap_base[1] = now.c[CTR_CAP_FAST];
    e->cap_base[2] = now.c[CTR_CAP_EMPTY];
    return AZX_OK;
}

extern "C" int azx_playout_cap_stats(azx_engine *e, int64_t out4[4]) {
    if (!e || !out4) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    CounterSnap now;
    TRY(snap_counters(e, &now));
    out4[0] = (int64_t)(now.c[CTR_CAP_FULL] - e->cap_base[0]);
    out4[1] = (int64_t)(now.c[CTR_CAP_FAST] - e->cap_base[1]);
    out4[2] = (int64_t)(now.c[CTR_CAP_EMPTY] - e->cap_base[2]);
    out4[3] = 0;
    return AZX_OK;
}

// ---- resignation for throughput self-play (include/azx.h; NOT the reference's behaviour) ------
static const char *resign_keep_problem(double keep_prob) {
    return (std::isfinite(keep_prob) && keep_prob >= 0.0 && keep_prob <= 1.0) ? nullptr : "keep_prob outside [0, 1]";
}

extern "C" int azx_resign_is_exempt(uint64_t seed, int64_t uid, double keep_prob) {
    if (resign_keep_problem(keep_prob)) return fail(AZX_EINVAL, "resign: keep_prob %g outside [0, 1]", keep_prob);
    if (keep_prob == 0.0) return 0;
    return azx_resign_exempt(seed, uid, AZX_RESIGN_DRAW_EXEMPT, azx_resign_threshold_m1(keep_prob)) ? 1 : 0;
}

// the games in progress leave the statistics, which start again from zero
static int resign_restart_stats(azx_engine *e) {
    azx_launch_resign_mark(e->d, e->stream);
    HIPCHECK(hipGetLastError());
    return zero_game_counters(e, e->d.resign_ctr, RS_COUNT);
}

extern "C" int azx_set_resign(azx_engine *e, double threshold, int min_ply, double keep_prob) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    if (!(std::isfinite(threshold) && threshold >= -1.0 && threshold <= 1.0))
        return fail(AZX_EINVAL, "resign: threshold %g outside [-1, 1]", threshold);
    if (min_ply < 0) return fail(AZX_EINVAL, "resign: min_ply %d is negative", min_ply);
    if (resign_keep_problem(keep_prob)) return fail(AZX_EINVAL, "resign: keep_prob %g outside [0, 1]", keep_prob);
    ENGINE_GUARD(e);
    TRY(resign_restart_stats(e));
    e->opt.resign_on = true;
    e->opt.resign_thr = threshold;
    e->opt.resign_min_ply = min_ply;
    e->opt.resign_keep = keep_prob;
    return AZX_OK;
}

extern "C" int azx_clear_resign(azx_engine *e) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    ENGINE_GUARD(e);
    e->opt.resign_on = false;
    e->opt.resign_thr = -1.0;
    e->opt.resign_min_ply = 0;
    e->opt.resign_keep = 0.0;
    return AZX_OK;
}

extern "C" int azx_resign_stats(azx_engine *e, int64_t out8[8]) {
    if (!e || !out8) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(sum_game_counters(e, e->d.resign_ctr, RS_COUNT, out8, 8));
    out8[7] = 0;                        // (reserved)
    return AZX_OK;
}

// ---- early stop for throughput self-play (include/azx.h; NOT the reference's behaviour) ------
extern "C" int azx_set_early_stop(azx_engine *e, int on) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    if (on != 0 && on != 1) return fail(AZX_EINVAL, "early stop: on must be 0 or 1, got %d", on);
    if (on != 0 && e->opt.gm_m != 0)
        return fail(AZX_EINVAL, "early stop: the engine has the Gumbel root search set, which does not play the PUCT visit "
                                "leader (clear it with azx_set_gumbel(e, 0, 0, 1, 0))");
    ENGINE_GUARD(e);
    TRY(zero_game_counters(e, e->d.estop_ctr, ES_COUNT));
    e->opt.estop_on = on != 0;
    return AZX_OK;
}

extern "C" int azx_early_stop_stats(azx_engine *e, int64_t out4[4]) {
    if (!e || !out4) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(sum_game_counters(e, e->d.estop_ctr, ES_COUNT, out4, 4));
    out4[3] = 0;                        // (reserved)
    return AZX_OK;
}

// ---- training targets of the recorded rows (include/azx.h; NOT the reference's behaviour) ------
extern "C" int azx_set_train_targets(azx_engine *e, int policy_rows, float value_mix) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    if (policy_rows != AZX_ROWS_REFERENCE && policy_rows != AZX_ROWS_VISITS)
        return fail(AZX_EINVAL, "train targets: policy_rows must be AZX_ROWS_REFERENCE (0) or AZX_ROWS_VISITS (1), got %d", policy_rows);
    if (!(value_mix >= 0.0f && value_mix <= 1.0f))      // NaN fails both comparisons
        return fail(AZX_EINVAL, "train targets: value_mix must be in [0, 1], got %g", (double)value_mix);
    ENGINE_GUARD(e);
    TRY(zero_game_counters(e, e->d.tt_ctr, TT_COUNT));
    e->opt.tt_rows = policy_rows;
    e->opt.tt_mix = value_mix;
    return AZX_OK;
}

extern "C" int azx_get_train_targets(azx_engine *e, int *policy_rows, float *value_mix) {
    if (!e || !policy_rows || !value_mix) return fail(AZX_EINVAL, "null argument");
    *policy_rows = e->opt.tt_rows;
    *value_mix = e->opt.tt_mix;
    return AZX_OK;
}

extern "C" int azx_train_targets_stats(azx_engine *e, int64_t out4[4]) {
    if (!e || !out4) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(sum_game_counters(e, e->d.tt_ctr, TT_COUNT, out4, 4));
    out4[3] = 0;                        // (reserved)
    return AZX_OK;
}

// ---- forced playouts and policy target pruning (include/azx.h; NOT the reference's behaviour) ------
extern "C" int azx_set_forced_playouts(azx_engine *e, float k, int prune) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    if (!(k >= 0.0f && k <= 64.0f))                     // NaN fails both comparisons
        return fail(AZX_EINVAL, "forced playouts: k must be in [0, 64], got %g", (double)k);
    if (prune != 0 && prune != 1) return fail(AZX_EINVAL, "forced playouts: prune must be 0 or 1, got %d", prune);
    if (k == 0.0f && prune == 1)
        return fail(AZX_EINVAL, "forced playouts: pruning needs forcing (k > 0): the prune gives back at most the forced quota");
    if (k != 0.0f && e->opt.gm_m != 0)
        return fail(AZX_EINVAL, "forced playouts: the engine has the Gumbel root search set, whose root selects are not "
                                "PUCT's (clear it with azx_set_gumbel(e, 0, 0, 1, 0))");
    ENGINE_GUARD(e);
    TRY(zero_game_counters(e, e->d.fp_ctr, FP_COUNT));
    e->opt.fp_k = k == 0.0f ? 0.0f : k;                     // (-0.0f is off too)
    e->opt.fp_prune = prune;
    return AZX_OK;
}

extern "C" int azx_get_forced_playouts(azx_engine *e, float *k, int *prune) {
    if (!e || !k || !prune) return fail(AZX_EINVAL, "null argument");
    *k = e->opt.fp_k;
    *prune = e->opt.fp_prune;
    return AZX_OK;
}

extern "C" int azx_forced_playouts_stats(azx_engine *e, int64_t out4[4]) {
    if (!e || !out4) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(sum_game_counters(e, e->d.fp_ctr, FP_COUNT, out4, 4));
    return AZX_OK;
}

// ---- Gumbel root search with sequential halving (include/azx.h; NOT the reference's behaviour) ------
extern "C" int azx_set_gumbel(azx_engine *e, int m, float c_visit, float c_scale, int improved_rows) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    if (m != 0 && (m < 2 || m > 64)) return fail(AZX_EINVAL, "gumbel: m must be 0 (off) or in [2, 64], got %d", m);
    if (m != 0) {
        if (!(c_visit >= 0.0f && c_visit <= 1.0e4f))     // NaN fails both comparisons
            return fail(AZX_EINVAL, "gumbel: c_visit must be in [0, 1e4], got %g", (double)c_visit);
        if (!(c_scale > 0.0f && c_scale <= 100.0f))
            return fail(AZX_EINVAL, "gumbel: c_scale must be in (0, 100], got %g", (double)c_scale);
        if (improved_rows != 0 && improved_rows != 1)
            return fail(AZX_EINVAL, "gumbel: improved_rows must be 0 or 1, got %d", improved_rows);
        if (e->opt.fp_k > 0.0f)
            return fail(AZX_EINVAL, "gumbel: the engine has forced playouts set, a rule about PUCT's root selects "
                                    "(clear them with azx_set_forced_playouts(e, 0, 0))");
        if (e->opt.estop_on)
            return fail(AZX_EINVAL, "gumbel: the engine has early stop set, a rule about the PUCT visit leader "
                                    "(clear it with azx_set_early_stop(e, 0))");
    }
    ENGINE_GUARD(e);
    HIPCHECK(hipMemsetAsync(e->d.gm_state, 0, (size_t)e->d.G * GM_STATE_WORDS * sizeof(uint64_t), e->stream));
    TRY(zero_game_counters(e, e->d.gm_ctr, GM_COUNT));
    e->opt.gm_m = m;
    e->opt.gm_c_visit = m ? c_visit + 0.0f : 0.0f;
    e->opt.gm_c_scale = m ? c_scale : 0.0f;
    e->opt.gm_rows = m ? improved_rows : 0;
    return AZX_OK;
}

extern "C" int azx_get_gumbel(azx_engine *e, int *m, float *c_visit, float *c_scale, int *improved_rows) {
    if (!e || !m || !c_visit || !c_scale || !improved_rows) return fail(AZX_EINVAL, "null argument");
    *m = e->opt.gm_m;
    *c_visit = e->opt.gm_c_visit;
    *c_scale = e->opt.gm_c_scale;
    *improved_rows = e->opt.gm_rows;
    return AZX_OK;
}

extern "C" int azx_gumbel_stats(azx_engine *e, int64_t out4[4]) {
    if (!e || !out4) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(sum_game_counters(e, e->d.gm_ctr, GM_COUNT, out4, 4));
    return AZX_OK;
}

extern "C" int azx_gumbel_state(azx_engine *e, uint64_t *candidates, uint64_t *survivors) {
    if (!e || !candidates || !survivors) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    const size_t G = e->d.G;
    std::vector<uint64_t> hs(G * GM_STATE_WORDS);
    HIPCHECK(hipMemcpyAsync(hs.data(), e->d.gm_state, hs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    for (size_t g = 0; g < G; ++g)
        for (int s = 0; s < 3; ++s) {
            candidates[g * 3 + s] = hs[g * GM_STATE_WORDS + GM_CAND + s];
            survivors[g * 3 + s] = hs[g * GM_STATE_WORDS + GM_SURV + s];
        }
    return AZX_OK;
}

extern "C" int azx_gumbel_variate(uint64_t seed, int64_t uid, int ply, int child, double *g) {
    if (!g) return fail(AZX_EINVAL, "null argument");
    if (ply < 0) return fail(AZX_EINVAL, "ply %d is negative", ply);
    if (child < 0 || child >= AZX_CELL_STRIDE) return fail(AZX_EINVAL, "child %d outside [0, %d)", child, AZX_CELL_STRIDE);
    *g = azx_gumbel_of_word_host(azx_gumbel_word(seed, uid, ply, child));
    return AZX_OK;
}

// ---- self-test hook (tests): the device's Gumbel variates of raw Philox words ----------------
extern "C" int azx_selftest_gumbel(int device, int n, const uint32_t *words, float *g_out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(AZX_ENODEV, "no HIP device visible");
    if (n < 1 || !words || !g_out) return fail(AZX_EINVAL, "bad argument");
    DevGuard guard(device);
    uint32_t *dw = nullptr;
    float *dg = nullptr;
    hipError_t err = hipMalloc(&dw, (size_t)n * 4);
    if (err == hipSuccess) err = hipMalloc(&dg, (size_t)n * 4);
    if (err == hipSuccess) err = hipMemcpy(dw, words, (size_t)n * 4, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        azx_launch_gumbel_test(dw, dg, n, nullptr);
        err = hipDeviceSynchronize();
    }
    if (err == hipSuccess) err = hipMemcpy(g_out, dg, (size_t)n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(dw); (void)hipFree(dg);                       // (on every path)
    if (err != hipSuccess) return fail(AZX_EHIP, "azx_selftest_gumbel: %s", hipGetErrorString(err));
    return AZX_OK;
}

// ---- first-play urgency (include/azx.h; NOT the reference's behaviour) ------
// A property of the engine's search: it lives in e->d, in every launch, and is not one of SELFPLAY_OPTIONS.
static int fpu_check(int mode, float value, float reduction, float root_reduction) {
    if (mode != AZX_FPU_OFF && mode != AZX_FPU_ABSOLUTE && mode != AZX_FPU_REDUCTION)
        return fail(AZX_EINVAL, "fpu: mode must be AZX_FPU_OFF (0), AZX_FPU_ABSOLUTE (1) or AZX_FPU_REDUCTION (2), got %d", mode);
    if (mode == AZX_FPU_OFF) return AZX_OK;
    if (!(value >= -1.0f && value <= 1.0f))                 // NaN fails both comparisons
        return fail(AZX_EINVAL, "fpu: value must be in [-1, 1], got %g", (double)value);
    if (!(reduction >= 0.0f && reduction <= 3.0e38f))
        return fail(AZX_EINVAL, "fpu: reduction must be finite and >= 0, got %g", (double)reduction);
    if (!(root_reduction >= 0.0f && root_reduction <= 3.0e38f))
        return fail(AZX_EINVAL, "fpu: root_reduction must be finite and >= 0, got %g", (double)root_reduction);
    return AZX_OK;
}

extern "C" int azx_set_fpu(azx_engine *e, int mode, float value, float reduction, float root_reduction) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    TRY(fpu_check(mode, value, reduction, root_reduction));
    if (!e->phase_api.done())
        return fail(AZX_ESTATE, "fpu: a phase-API search is in flight (finish it with azx_search_step first)");
    ENGINE_GUARD(e);
    TRY(zero_game_counters(e, e->d.fpu_ctr, FPU_COUNT));
    const bool on = mode != AZX_FPU_OFF;
    e->d.fpu_mode = mode;
    e->d.fpu_value = on ? value + 0.0f : 0.0f;
    e->d.fpu_red = on ? reduction + 0.0f : 0.0f;
    e->d.fpu_root_red = on ? root_reduction + 0.0f : 0.0f;
    return AZX_OK;
}

extern "C" int azx_get_fpu(azx_engine *e, int *mode, float *value, float *reduction, float *root_reduction) {
    if (!e || !mode || !value || !reduction || !root_reduction) return fail(AZX_EINVAL, "null argument");
    *mode = e->d.fpu_mode;
    *value = e->d.fpu_value;
    *reduction = e->d.fpu_red;
    *root_reduction = e->d.fpu_root_red;
    return AZX_OK;
}

extern "C" int azx_fpu_stats(azx_engine *e, int64_t out4[4]) {
    if (!e || !out4) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(sum_game_counters(e, e->d.fpu_ctr, FPU_COUNT, out4, 4));
    out4[3] = 0;                        // (not computed: include/azx.h)
    return AZX_OK;
}

// the definition on the host for one node: score_actions + np.argmax (mcts.py:119-136, :112) op by op in float32, the
// unvisited children's Q from fpu.h
extern "C" int azx_fpu_score(int mode, float value, float reduction, float root_reduction, int is_root, int k, float nv_p,
                             float tv_p, const float *nv, const float *tv, const float *prior, float c_puct,
                             int32_t *child_out) {
#pragma clang fp contract(off)
    if (k < 1 || !nv || !tv || !prior || !child_out) return fail(AZX_EINVAL, "fpu score: bad argument");
    TRY(fpu_check(mode, value, reduction, root_reduction));
    double sum = 0.0;                                       // integers: exact in any order
    uint32_t M = 0u;
    for (int j = 0; j < k; ++j) {
        sum += (double)nv[j];
        if (nv[j] > 0.0f) M += azx_fpu_mass_word(prior[j]);
    }
    const float sq = sqrtf((float)sum);
    float fpu = 0.0f;
    if (mode != AZX_FPU_OFF) fpu = azx_fpu_q(mode, value, is_root ? root_reduction : reduction, nv_p, tv_p, M);
    int best = 0;
    float best_score = 0.0f;
    for (int j = 0; j < k; ++j) {
        const float gap = sq / (1.0f + nv[j]);
        const float U = (c_puct * prior[j]) * gap;
        float Q = (-tv[j]) / fmaxf(nv[j], 1.0f);
        if (mode != AZX_FPU_OFF && nv[j] == 0.0f) Q = fpu;
        const float score = Q + U;
        if (j == 0 || score > best_score) { best = j; best_score = score; }
    }
    *child_out = best;
    return AZX_OK;
}

// ---- policy temperature of the search's priors (include/azx.h; NOT the reference's behaviour) ------
// Like first-play urgency a property of the engine's search: it lives in e->d, in every launch, and is not one of
// SELFPLAY_OPTIONS.
static int pt_check(int eighths, int root_eighths) {
    if (eighths < 1 || eighths > 8)
        return fail(AZX_EINVAL, "policy temperature: eighths must be in 1..8 (8 is off), got %d", eighths);
    if (root_eighths < 1 || root_eighths > 8)
        return fail(AZX_EINVAL, "policy temperature: root_eighths must be in 1..8 (8 is off), got %d", root_eighths);
    return AZX_OK;
}

extern "C" int azx_set_policy_temp(azx_engine *e, int eighths, int root_eighths) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    TRY(pt_check(eighths, root_eighths));
    if (!e->phase_api.done())
        return fail(AZX_ESTATE, "policy temperature: a phase-API search is in flight (finish it with azx_search_step first)");
    ENGINE_GUARD(e);
    TRY(zero_game_counters(e, e->d.pt_ctr, PT_COUNT));
    e->pt_eighths = eighths;
    e->pt_root_eighths = root_eighths;
    pt_refresh(e);
    return AZX_OK;
}

extern "C" int azx_get_policy_temp(azx_engine *e, int *eighths, int *root_eighths) {
    if (!e || !eighths || !root_eighths) return fail(AZX_EINVAL, "null argument");
    *eighths = e->pt_eighths;
    *root_eighths = e->pt_root_eighths;
    return AZX_OK;
}

extern "C" int azx_policy_temp_stats(azx_engine *e, int64_t out4[4]) {
    if (!e || !out4) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    TRY(sum_game_counters(e, e->d.pt_ctr, PT_COUNT, out4, 4));
    out4[3] = 0;
    return AZX_OK;
}

// the definition on the host for one row, from the text the kernels compile (policy_temp.h)
extern "C" int azx_policy_temp_row(int eighths, int k, const float *p_in, float *p_out, int *tempered) {
#pragma clang fp contract(off)
    if (k < 1 || k > AZX_CELL_STRIDE || !p_in || !p_out || !tempered)
        return fail(AZX_EINVAL, "policy temperature row: k must be in 1..%d and the pointers non-null", AZX_CELL_STRIDE);
    if (eighths < 1 || eighths > 8)
        return fail(AZX_EINVAL, "policy temperature: eighths must be in 1..8 (8 is off), got %d", eighths);
    *tempered = 0;
    bool bad = eighths == 8;
    for (int j = 0; j < k && !bad; ++j) bad = azx_pt_bad(p_in[j]);
    uint32_t Z = 0u;
    if (!bad) {
        for (int j = 0; j < k; ++j) Z += azx_pt_word(azx_pt_q(p_in[j], eighths));
        bad = Z == 0u;
    }
    if (bad) {
        if (p_out != p_in) memmove(p_out, p_in, sizeof(float) * (size_t)k);
        return AZX_OK;
    }
    const float Zf = azx_pt_zf(Z);
    for (int j = 0; j < k; ++j) p_out[j] = azx_pt_q(p_in[j], eighths) / Zf;
    *tempered = 1;
    return AZX_OK;
}

extern "C" int azx_resign_value(azx_engine *e, float *v) {
    if (!e || !v) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    azx_launch_resign_value(e->d, e->g_sv, e->stream);      // (g_sv: azx_get_root's per-slot float scratch)
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(v, e->g_sv, (size_t)e->d.G * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

extern "C" int azx_debug_counters_raw(azx_engine *e, uint64_t *out, int64_t n_games) {
    if (!e || !out) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    if (n_games != e->d.G) return fail(AZX_EINVAL, "n_games must equal the engine's game count");
    HIPCHECK(hipMemcpyAsync(out, e->d.counters, (size_t)n_games * CTR_COUNT * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

extern "C" int azx_debug_counters(azx_engine *e, uint64_t *out16) {
    if (!e || !out16) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    CounterSnap snap;
    TRY(snap_counters(e, &snap));
    for (int j = 0; j < CTR_COUNT; ++j) out16[j] = snap.c[j];
    return AZX_OK;
}

// ---- opening books of matches and tournaments: the host-side check (no device call) ---------------------------
// Colour of the winner after `tile` was played, or 0: the mover's group around the tile is flood-filled and wins when
// it spans rows 0 .. N-1 (colour 1) or columns 0 .. N-1 (colour 2) -- hex.py:204-231 over the :190-195 neighbourhood.
static int hex_host_winner(const std::vector<int8_t> &board, int N, int tile) {
    static const int dr[6] = {-1, -1, 0, 0, 1, 1}, dc[6] = {0, 1, -1, 1, -1, 0};
    const int color = board[(size_t)tile];
    std::vector<char> seen(board.size(), 0);
    std::vector<int> border(1, tile);
    seen[(size_t)tile] = 1;
    int lo = N, hi = -1;
    while (!border.empty()) {
        const int t = border.back();
        border.pop_back();
        const int r = t / N, c = t - r * N, i = color == 1 ? r : c;
        lo = std::min(lo, i);
        hi = std::max(hi, i);
        if (lo == 0 && hi == N - 1) return color;
        for (int d = 0; d < 6; ++d) {
            const int rr = r + dr[d], cc = c + dc[d];
            if (rr < 0 || rr >= N || cc < 0 || cc >= N) continue;
            const int nb = rr * N + cc;
            if (seen[(size_t)nb] || board[(size_t)nb] != color) continue;
            seen[(size_t)nb] = 1;
            border.push_back(nb);
        }
    }
    return 0;
}

// the arguments every opening-book entry point refuses before it looks at the table
static int openings_args(int n_openings, int stride, const int16_t *moves, const int32_t *lengths) {
    if (n_openings < 0 || n_openings > (1 << 20))
        return fail(AZX_EINVAL, "n_openings %d outside [0, %d]", n_openings, 1 << 20);
    if (stride < 0) return fail(AZX_EINVAL, "stride %d must be >= 0", stride);
    if (n_openings > 0 && (!moves || !lengths)) return fail(AZX_EINVAL, "null opening table with n_openings = %d", n_openings);
    return AZX_OK;
}

extern "C" int azx_openings_check(int board_size, int n_openings, int stride, const int16_t *moves,
                                  const int32_t *lengths, int32_t *bad_opening, int32_t *bad_ply) {
    if (board_size < 2 || board_size > AZX_MAX_BOARD)
        return fail(AZX_EINVAL, "board_size %d outside [2, %d]", board_size, AZX_MAX_BOARD);
    TRY(openings_args(n_openings, stride, moves, lengths));
    const int N = board_size, ncells = N * N;
    std::vector<int8_t> board((size_t)ncells);
    auto refuse = [&](int o, int p) {
        if (bad_opening) *bad_opening = o;
        if (bad_ply) *bad_ply = p;
        return AZX_EINVAL;
    };
    for (int o = 0; o < n_openings; ++o) {
        const int len = lengths[o];
        if (len < 0 || len > stride) {
            (void)fail(AZX_EINVAL, "opening %d: length %d outside [0, stride %d]", o, len, stride);
            return refuse(o, -1);
        }
        std::fill(board.begin(), board.end(), (int8_t)0);
        for (int p = 0; p < len; ++p) {
            const int mv = moves[(size_t)o * stride + p];
            if (mv < 1 || mv > ncells) {
                (void)fail(AZX_EINVAL, "opening %d, ply %d: move %d outside [1, %d] (tile + 1 on a %dx%d board)", o, p, mv,
                           ncells, N, N);
                return refuse(o, p);
            }
            if (board[(size_t)mv - 1]) {
                (void)fail(AZX_EINVAL, "opening %d, ply %d: tile %d is played twice", o, p, mv - 1);
                return refuse(o, p);
            }
            board[(size_t)mv - 1] = (int8_t)(1 + (p & 1));
            if (hex_host_winner(board, N, mv - 1)) {
                (void)fail(AZX_EINVAL, "opening %d, ply %d: move %d decides the game for colour %d (an opening must leave "
                           "the game undecided)", o, p, mv, 1 + (p & 1));
                return refuse(o, p);
            }
        }
    }
    return AZX_OK;
}

// the checked book on the device, replacing `*book` (the handle's); n_openings == 0 clears it.  Blocking copies:
// no play call of the handle is running (they block), so the old tables are free to go.
static int book_set(MatchBook *book, int board_size, int n_openings, int stride, const int16_t *moves,
                    const int32_t *lengths) {
    TRY(azx_openings_check(board_size, n_openings, stride, moves, lengths, nullptr, nullptr));
    MatchBook nb = {nullptr, nullptr, 0, 0};
    if (n_openings > 0) {
        int16_t *dm = nullptr;
        int32_t *dl = nullptr;
        const size_t mbytes = sizeof(int16_t) * (size_t)n_openings * (size_t)stride;
        hipError_t err = hipMalloc((void **)&dm, std::max<size_t>(mbytes, 16));
        if (err == hipSuccess) err = hipMalloc((void **)&dl, sizeof(int32_t) * (size_t)n_openings);
        if (err == hipSuccess && mbytes) err = hipMemcpy(dm, moves, mbytes, hipMemcpyHostToDevice);
        if (err == hipSuccess) err = hipMemcpy(dl, lengths, sizeof(int32_t) * (size_t)n_openings, hipMemcpyHostToDevice);
        if (err != hipSuccess) {
            if (dm) (void)hipFree(dm);
            if (dl) (void)hipFree(dl);
            return fail(AZX_ENOMEM, "copying a book of %d openings to the device failed: %s", n_openings, hipGetErrorString(err));
        }
        nb = MatchBook{dm, dl, n_openings, stride};
    }
    if (book->moves) (void)hipFree(const_cast<int16_t *>(book->moves));
    if (book->len) (void)hipFree(const_cast<int32_t *>(book->len));
    *book = nb;
    return AZX_OK;
}

// ---- self-play opening book (include/azx.h; NOT the reference's behaviour) ------------------------------------
extern "C" int azx_selfplay_opening_word(uint64_t seed, int64_t uid, uint32_t *word) {
    if (!word) return fail(AZX_EINVAL, "null argument");
    *word = azx_book_word(seed, uid);
    return AZX_OK;
}

extern "C" int azx_selfplay_openings_bounds(int n_openings, const double *weights, uint64_t *ub) {
    if (!ub) return fail(AZX_EINVAL, "null argument");
    if (n_openings < 1 || n_openings > (1 << 20))
        return fail(AZX_EINVAL, "selfplay openings: n_openings %d outside [1, %d]", n_openings, 1 << 20);
    int bad = -1;
    if (const char *why = azx_book_bounds(n_openings, weights, ub, &bad)) {
        if (bad >= 0) return fail(AZX_EINVAL, "selfplay openings: weight %d (%g) %s", bad, weights[bad], why);
        return fail(AZX_EINVAL, "selfplay openings: the weights' %s", why[0] == 'a' ? "values are all zero" : why);
    }
    return AZX_OK;
}

extern "C" int azx_set_selfplay_openings(azx_engine *e, int n_openings, int stride, const int16_t *moves,
                                         const int32_t *lengths, const double *weights) {
    if (!e) return fail(AZX_EINVAL, "null engine");
    TRY(openings_args(n_openings, stride, moves, lengths));
    TRY(azx_openings_check(e->d.N, n_openings, stride, moves, lengths, nullptr, nullptr));
    std::vector<uint64_t> ub((size_t)n_openings);
    if (n_openings > 0) TRY(azx_selfplay_openings_bounds(n_openings, weights, ub.data()));
    ENGINE_GUARD(e);
    // no play call of the engine is running (they block): the old tables are free to go once the new ones stand
    HIPCHECK(hipStreamSynchronize(e->stream));
    if (e->stream_b) HIPCHECK(hipStreamSynchronize(e->stream_b));
    void *na[4] = {nullptr, nullptr, nullptr, nullptr};
    if (n_openings > 0) {
        const size_t n = (size_t)n_openings;
        const size_t bytes[4] = {std::max<size_t>(sizeof(int16_t) * n * (size_t)stride, 16), sizeof(int32_t) * n,
                                 sizeof(uint64_t) * n, sizeof(unsigned long long) * n * BK_COUNT};
        const void *src[4] = {moves, lengths, ub.data(), nullptr};
        hipError_t err = hipSuccess;
        for (int i = 0; i < 4 && err == hipSuccess; ++i) {
            err = hipMalloc(&na[i], bytes[i]);
            if (err != hipSuccess) break;
            if (i == 0 && stride == 0) err = hipMemset(na[i], 0, bytes[i]);
            else if (src[i]) err = hipMemcpy(na[i], src[i], i == 0 ? sizeof(int16_t) * n * (size_t)stride : bytes[i], hipMemcpyHostToDevice);
            else err = hipMemset(na[i], 0, bytes[i]);
        }
        if (err != hipSuccess) {
            for (void *p : na) if (p) (void)hipFree(p);
            return fail(AZX_ENOMEM, "copying a book of %d openings to the device failed: %s", n_openings, hipGetErrorString(err));
        }
    }
    for (int i = 0; i < 4; ++i) {
        if (e->book_allocs[i]) (void)hipFree(e->book_allocs[i]);
        e->book_allocs[i] = na[i];
    }
    DevEngine &d = e->d;
    d.bk_n = n_openings;
    d.bk_stride = n_openings > 0 ? stride : 0;
    d.bk_moves = (const int16_t *)na[0];
    d.bk_len = (const int32_t *)na[1];
    d.bk_ub = (const uint64_t *)na[2];
    d.bk_ctr = (unsigned long long *)na[3];
    // the games that have not begun follow the new book (or, cleared, the empty board) from where they stand
    azx_launch_book_seat(d, e->stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(e->stream));
    return AZX_OK;
}

extern "C" int azx_selfplay_openings_slots(azx_engine *e, int32_t *opening) {
    if (!e || !opening) return fail(AZX_EINVAL, "null argument");
    ENGINE_GUARD(e);
    std::vector<GameHdr> hdr((size_t)e->d.G);
    HIPCHECK(hipMemcpyAsync(hdr.data(), e->d.ghdr, hdr.size() * sizeof(GameHdr), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    for (size_t g = 0; g < hdr.size(); ++g) opening[g] = e->d.bk_n > 0 ? hdr[g].book : -1;
    return AZX_OK;
}

extern "C" int azx_selfplay_openings_stats(azx_engine *e, int64_t cap, int64_t *out) {
    if (!e || (cap > 0 && !out)) return fail(AZX_EINVAL, "null argument");
    const int64_t n = e->d.bk_n;
    if (cap < n) return fail(AZX_EINVAL, "selfplay openings: room for %lld openings, the book has %lld", (long long)cap, (long long)n);
    if (n == 0) return 0;
    ENGINE_GUARD(e);
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "tally width");
    HIPCHECK(hipMemcpyAsync(out, e->d.bk_ctr, (size_t)n * BK_COUNT * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHECK(hipStreamSynchronize(e->stream));
    return (int)n;
}

// ---- matches between two engines on the device (match_kernels.hip) -------------------------------------------
// evaluation.worker + play_game (evaluation.py:60-80, play_game.py:27-52) for a whole pool of games: slot g of
// engine a and slot g of engine b hold the two agents' trees of one game.  Per ply the host enqueues
//   k_match_turn                      (a's stream)  whose turn it is -> GameHdr.active in both engines
//   a's search + move draw            (a's stream)  |  b's search + move draw  (b's stream, forked / joined by events)
//   k_match_step                      (a's stream)  hand-over, game step in both engines, settle, refill
// and reads back ONE word, the number of games decided.  An engine with a registered external evaluator cannot be
// enqueued whole: the host takes part at each of its evaluation points.  Its search is then a cursor (SearchCursor)
// that the ply advances point by point, after everything that needs no host is on the streams and in turn with the
// other engine's cursor when both are external (ply_searches).
//
// A tournament (further down) is P such matches side by side in the same ply loop.  What the two handles share is a
// PlyLoop, and everything the host does around the two kernel families is written once, over it: the handle's shared
// state, the setters, the prologue and epilogue of a play call and the ply loop itself.  A handle adds what is its
// own: the device state of its kernel family (MatchDev / TourDev) and the result buffers behind it.
struct PlyLoop {
    std::vector<azx_engine *> eng;               // a match: {a, b}.  Engine 0's stream carries the turn and step kernels
    const char *noun = "match";                  // the handle in messages: "match" or "tournament"
    const char *letters = nullptr;               // the engines in messages: "ab" for a match, null = by index
    bool interleave = true;                      // AZX_MATCH_INTERLEAVE=0 (a match only): each engine's whole search in turn
    unsigned long long *host_word = nullptr;     // pinned: the per-ply read-back
    hipEvent_t ev_fork = nullptr, t0 = nullptr, t1 = nullptr;
    std::vector<hipEvent_t> ev_join;             // [K - 1]: engine k's stream back into engine 0's
    std::vector<SearchCursor> cur;                 // [K]: the external engines' searches of the current ply
    int sink = -1;                               // *_set_harvest: the engine whose harvest queue takes the won games' rows
    int first_mode = -1;                         // *_set_first_mover
    int64_t rows_last = 0;                       // rows the last play call harvested
    MatchBook book = {nullptr, nullptr, 0, 0};   // *_set_openings: device tables the handle owns (n == 0: none)

    std::string name(int k) const { return letters ? std::string(1, letters[k]) : std::to_string(k); }
};

static const char *match_engine_problem(const azx_engine *e) {
    if (e->d.evaluator == AZX_EVAL_EXTERNAL && !ext_registered(e))
        return "is an AZX_EVAL_EXTERNAL engine with no evaluator registered (azx_set_external_evaluator)";
    if (e->d.evaluator == AZX_EVAL_RESNET && !azx_net_ready(e->net)) return "has no weights (azx_set_weights)";
    return nullptr;
}

// the shared state of a new handle, after the handle's own allocations (`err`: how those went) in one chain: whatever
// fails, the caller destroys the partly built handle and returns AZX_ENOMEM
static hipError_t loop_create(PlyLoop &L, hipError_t err, azx_engine *const *engines, int K, const char *noun,
                              const char *letters) {
    L.eng.assign(engines, engines + K);
    L.noun = noun;
    L.letters = letters;
    L.ev_join.assign((size_t)K - 1, nullptr);
    L.cur.assign((size_t)K, SearchCursor());
    if (err == hipSuccess) err = hipHostMalloc((void **)&L.host_word, sizeof(unsigned long long), hipHostMallocDefault);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&L.ev_fork, hipEventDisableTiming);
    for (hipEvent_t &ev : L.ev_join)
        if (err == hipSuccess) err = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (err == hipSuccess) err = hipEventCreate(&L.t0);
    if (err == hipSuccess) err = hipEventCreate(&L.t1);
    return err;
}

// frees the device buffers `own` of a handle and its shared state (the caller holds the device and deletes the handle)
static void loop_destroy(PlyLoop &L, std::initializer_list<const void *> own) {
    for (const void *p : own)
        if (p) (void)hipFree(const_cast<void *>(p));
    for (const void *p : {(const void *)L.book.moves, (const void *)L.book.len})
        if (p) (void)hipFree(const_cast<void *>(p));
    if (L.host_word) (void)hipHostFree(L.host_word);
    for (hipEvent_t ev : {L.ev_fork, L.t0, L.t1})
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : L.ev_join)
        if (ev) (void)hipEventDestroy(ev);
}

// the bodies of azx_{match,tournament}_set_first_mover / _set_openings / _rows (L: null for a null handle, which
// `noun` names in the message)
static int loop_set_first_mover(PlyLoop *L, const char *noun, int mode) {
    if (mode < -1 || mode > 1) return fail(AZX_EINVAL, "first mover mode %d: -1 (agent u & 1), 0 or 1", mode);
    if (!L) return fail(AZX_EINVAL, "null %s", noun);
    L->first_mode = mode;
    return AZX_OK;
}

static int loop_set_openings(PlyLoop *L, const char *noun, int n_openings, int stride, const int16_t *moves,
                             const int32_t *lengths) {
    if (!L) return fail(AZX_EINVAL, "null %s", noun);
    TRY(openings_args(n_openings, stride, moves, lengths));
    ENGINE_GUARD(L->eng[0]);
    return book_set(&L->book, L->eng[0]->d.N, n_openings, stride, moves, lengths);
}

static int loop_rows(const PlyLoop *L, int64_t *rows_out) {
    if (!L || !rows_out) return fail(AZX_EINVAL, "null argument");
    *rows_out = L->rows_last;
    return AZX_OK;
}

struct azx_match {
    PlyLoop loop;
    MatchDev m = {nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, -1};
    int16_t *moves_buf = nullptr;
    int64_t out_cap = 0, len_cap = 0, moves_cap = 0;     // elements the outcome, length and moves buffers hold
};

extern "C" void azx_match_destroy(azx_match *m) {
    if (!m) return;
    DevGuard guard(m->loop.eng[0]->cfg.device);
    loop_destroy(m->loop, {m->m.slot_game, m->m.ctr, m->m.outcome, m->m.length, m->moves_buf});
    delete m;
}

extern "C" int azx_match_create(azx_engine *a, azx_engine *b, azx_match **out) {
    if (!a || !b || !out) return fail(AZX_EINVAL, "null argument");
    if (a == b) return fail(AZX_EINVAL, "a match needs two engines: every agent owns its search tree (a == b)");
    if (a->cfg.device != b->cfg.device)
        return fail(AZX_EINVAL, "the engines are on different devices (%d and %d)", a->cfg.device, b->cfg.device);
    if (a->d.N != b->d.N) return fail(AZX_EINVAL, "the engines' board sizes differ (%d and %d)", a->d.N, b->d.N);
    if (a->d.G != b->d.G) return fail(AZX_EINVAL, "the engines' n_games differ (%d and %d)", a->d.G, b->d.G);
    if (const char *why = match_engine_problem(a)) return fail(AZX_EINVAL, "engine a %s", why);
    if (const char *why = match_engine_problem(b)) return fail(AZX_EINVAL, "engine b %s", why);
    DevGuard guard(a->cfg.device);
    azx_match *m = new azx_match();
    azx_engine *const both[2] = {a, b};
    hipError_t err = hipMalloc((void **)&m->m.slot_game, sizeof(int64_t) * (size_t)a->d.G);
    if (err == hipSuccess) err = hipMalloc((void **)&m->m.ctr, sizeof(unsigned long long) * MCTR_COUNT);
    err = loop_create(m->loop, err, both, 2, "match", "ab");
    { const char *v = getenv("AZX_MATCH_INTERLEAVE"); m->loop.interleave = !(v && atoi(v) == 0); }
    if (err != hipSuccess) {
        azx_match_destroy(m);
        return fail(AZX_ENOMEM, "allocating the match state failed: %s", hipGetErrorString(err));
    }
    *out = m;
    return AZX_OK;
}

extern "C" int azx_match_set_harvest(azx_match *m, int on) {
    if (!m) return fail(AZX_EINVAL, "null match");
    m->loop.sink = on ? 0 : -1;                          // won games' replay rows go to a's harvest queue
    return AZX_OK;
}

extern "C" int azx_match_set_first_mover(azx_match *m, int mode) {
    return loop_set_first_mover(m ? &m->loop : nullptr, "match", mode);
}
extern "C" int azx_match_set_openings(azx_match *m, int n_openings, int stride, const int16_t *moves,
                                      const int32_t *lengths) {
    return loop_set_openings(m ? &m->loop : nullptr, "match", n_openings, stride, moves, lengths);
}
extern "C" int azx_match_rows(azx_match *m, int64_t *rows_out) { return loop_rows(m ? &m->loop : nullptr, rows_out); }

// the harvest queue of a harvesting match / tournament: no ring, room for every game at its longest (`cells` plies)
static int harvest_setup(azx_engine *sink, int64_t n_games) {
    const int64_t rows = n_games * sink->d.ncells;
    const size_t row_bytes = AZX_CELL_STRIDE + AZX_CELL_STRIDE * sizeof(float) + 2 * sizeof(int32_t) + sizeof(float) +
                             sizeof(int64_t) + AZX_ROW_METRICS * sizeof(float);
    const int rc = play_setup(sink, rows, 0);
    if (rc == AZX_ENOMEM)
        return fail(AZX_ENOMEM, "the harvest queue of %lld games needs %lld rows = %zu bytes of device memory: %s",
                    (long long)n_games, (long long)rows, (size_t)rows * row_bytes, std::string(g_err).c_str());
    if (rc) return rc;
    if (sink->dbg_qcap > 0)                              // tests (azx_debug_set_queue_cap): a queue too small
        sink->d.q_cap = std::max<int64_t>(1, std::min<int64_t>(sink->d.q_cap, sink->dbg_qcap));
    return AZX_OK;
}

// a device buffer of at least `count` elements (grown, never shrunk; the contents are not kept)
template <typename T>
static int loop_grow(const PlyLoop &L, T **p, int64_t *cap, int64_t count, const char *what) {
    if (count <= *cap) return AZX_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    if (hipMalloc((void **)p, sizeof(T) * (size_t)count) != hipSuccess)
        return fail(AZX_ENOMEM, "hipMalloc of the %s's %s (%lld) failed", L.noun, what, (long long)count);
    *cap = count;
    return AZX_OK;
}

// a failure inside a ply: nothing any engine has queued is left running, and the message says whose engine it was
static int loop_fail(const PlyLoop &L, int k, int rc) {
    for (azx_engine *e : L.eng) (void)hipStreamSynchronize(e->stream);
    if (rc == AZX_EEXTERNAL) g_err = "engine " + L.name(k) + ": " + g_err;
    return rc;
}
#define LOOP_TRY(k, expr)                           \
    do {                                            \
        int _rc = (expr);                           \
        if (_rc) return loop_fail(L, (k), _rc);     \
    } while (0)

// Every engine's search and move draw of one ply, each on its engine's stream (all forked from engine 0's).
// Interleaved: first what needs no host -- the whole search and draw of every device-evaluated engine -- then the
// external engines' cursors in turn, so that each engine's next tree phase is on its stream before the host waits
// for another engine's evaluation point.  Plain order: each engine's whole search in turn.  The streams' contents,
// and so the games, are the same either way.
static int ply_searches(PlyLoop &L) {
    const int K = (int)L.eng.size();
    for (int k = 0; k < K; ++k)
        if (!L.interleave || !ext_registered(L.eng[k])) {
            LOOP_TRY(k, enqueue_search(L.eng[k], false));
            azx_launch_choose(L.eng[k]->d, L.eng[k]->stream);
        }
    if (!L.interleave) return AZX_OK;
    for (int k = 0; k < K; ++k) {
        L.cur[k] = ext_registered(L.eng[k]) ? SearchCursor(L.eng[k]->num_batches, false, false) : SearchCursor();
        if (!L.cur[k].done()) LOOP_TRY(k, search_advance(L.eng[k], &L.cur[k]));
    }
    for (bool busy = true; busy;) {
        busy = false;
        for (int k = 0; k < K; ++k)
            if (!L.cur[k].done()) {
                LOOP_TRY(k, search_advance(L.eng[k], &L.cur[k]));
                busy = true;
            }
    }
    for (int k = 0; k < K; ++k)
        if (ext_registered(L.eng[k])) azx_launch_choose(L.eng[k]->d, L.eng[k]->stream);
    return AZX_OK;
}

// What a play call does before anything of its own reaches the device (the caller holds the device): the refusals,
// `n_stats` stats blocks zeroed, and every engine's row area and noise.  The move draw records a replay row per draw
// (choose_body), so the row area must exist: a game draws at most ceil(cells / 2) times per engine and n_rows restarts
// with every game; the sink's is its harvest queue instead.
static int loop_begin(PlyLoop &L, int64_t n_games, azx_match_stats *stats, int n_stats) {
    const int K = (int)L.eng.size();
    TRY(refuse_selfplay_options(L.eng.data(), K, L.noun, L.letters));
    for (int k = 0; k < K; ++k)
        if (const char *why = match_engine_problem(L.eng[k])) return fail(AZX_ESTATE, "engine %s %s", L.name(k).c_str(), why);
    for (azx_engine *e : L.eng) TRY(ext_refuse(e));
    if (stats) memset(stats, 0, sizeof *stats * (size_t)n_stats);
    L.rows_last = 0;
    for (int k = 0; k < K; ++k) {
        azx_engine *e = L.eng[k];
        if (k == L.sink) TRY(harvest_setup(e, n_games));
        else TRY(play_setup(e, std::max<int64_t>(e->q_alloc, 1 << 10), 1));
        TRY(upload_noise(e, nullptr, 0, 0, e->cfg.noise_scale));
    }
    return AZX_OK;
}

// The ply loop, from the handle's games in their slots (the caller has synchronised engine 0's stream after its init
// kernels) until `*decided_dev` says all n_games are decided.  Per ply: turn() on engine 0's stream, the other
// streams forked from it, every engine's search and draw, the streams joined, step(), and ONE word read back.
template <typename Turn, typename Step>
static int loop_play(PlyLoop &L, const unsigned long long *decided_dev, int64_t n_games, int64_t max_plies,
                     const Turn &turn, const Step &step) {
    const int K = (int)L.eng.size();
    const hipStream_t s0 = L.eng[0]->stream;
    HIPCHECK(hipEventRecord(L.t0, s0));
    for (int64_t plies = 0;; ++plies) {
        if (plies > max_plies)
            return fail(AZX_ESTATE, "%s: %lld plies without deciding all %lld games (internal error)", L.noun,
                        (long long)plies, (long long)n_games);
        turn();
        HIPCHECK(hipEventRecord(L.ev_fork, s0));
        for (int k = 1; k < K; ++k) HIPCHECK(hipStreamWaitEvent(L.eng[k]->stream, L.ev_fork, 0));
        TRY(ply_searches(L));
        for (int k = 1; k < K; ++k) {
            HIPCHECK(hipEventRecord(L.ev_join[k - 1], L.eng[k]->stream));
            HIPCHECK(hipStreamWaitEvent(s0, L.ev_join[k - 1], 0));
        }
        step();
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(L.host_word, decided_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, s0));
        // the error word of each external search's last import rides on the same read-back (every stream has joined)
        for (azx_engine *e : L.eng)
            if (ext_registered(e)) TRY(ext_info_enqueue(e, s0));
        HIPCHECK(hipStreamSynchronize(s0));
        for (int k = 0; k < K; ++k)
            if (ext_registered(L.eng[k])) LOOP_TRY(k, ext_info_take(L.eng[k]));
        if (*L.host_word >= (unsigned long long)n_games) break;
    }
    HIPCHECK(hipEventRecord(L.t1, s0));
    return AZX_OK;
}

static void fill_match_stats(const unsigned long long *ctr, float ms, azx_match_stats *st) {
    st->games = (int64_t)ctr[MCTR_DECIDED];
    st->wins[0] = (int64_t)ctr[MCTR_WINS0];
    st->wins[1] = (int64_t)ctr[MCTR_WINS1];
    st->first_player_wins = (int64_t)ctr[MCTR_FIRST_WINS];
    st->voided = (int64_t)ctr[MCTR_VOIDED];
    st->plies = (int64_t)ctr[MCTR_PLIES];
    st->seconds = ms * 1e-3;
}

// the device side of a finished play call's results: P counter blocks (one per pair; a match has one) and the records
struct LoopResults {
    const unsigned long long *ctr;
    const int8_t *outcome;
    const int16_t *length;
    const int16_t *moves;
};

// What a play call does after its ply loop: the results to the caller's arrays, every engine left as azx_reset leaves
// it (fresh games, all active, its own uid numbering), the stats of the P blocks, and the checks that come last.
static int loop_finish(PlyLoop &L, const LoopResults &dev, int P, int64_t n_games, int8_t *outcome, int16_t *length,
                       int16_t *moves, azx_match_stats *stats) {
    azx_engine *sink = L.sink >= 0 ? L.eng[(size_t)L.sink] : nullptr;
    const hipStream_t s0 = L.eng[0]->stream;
    const size_t ncells = (size_t)L.eng[0]->d.ncells;
    std::vector<unsigned long long> ctr((size_t)P * MCTR_COUNT);
    unsigned long long rows = 0, lost = 0;
    HIPCHECK(hipMemcpyAsync(ctr.data(), dev.ctr, sizeof(unsigned long long) * ctr.size(), hipMemcpyDeviceToHost, s0));
    if (sink) HIPCHECK(hipMemcpyAsync(&rows, sink->d.q_count, sizeof rows, hipMemcpyDeviceToHost, s0));
    if (outcome) HIPCHECK(hipMemcpyAsync(outcome, dev.outcome, (size_t)n_games, hipMemcpyDeviceToHost, s0));
    if (length) HIPCHECK(hipMemcpyAsync(length, dev.length, sizeof(int16_t) * (size_t)n_games, hipMemcpyDeviceToHost, s0));
    if (moves) HIPCHECK(hipMemcpyAsync(moves, dev.moves, sizeof(int16_t) * (size_t)n_games * ncells, hipMemcpyDeviceToHost, s0));
    for (azx_engine *e : L.eng) azx_launch_reset(e->d, nullptr, e->d.G, nullptr, nullptr, 0, 1, s0);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s0));
    if (stats) {
        float ms = 0.f;
        HIPCHECK(hipEventElapsedTime(&ms, L.t0, L.t1));
        for (int s = 0; s < P; ++s) fill_match_stats(ctr.data() + (size_t)s * MCTR_COUNT, ms, stats + s);
    }
    for (int s = 0; s < P; ++s) lost += ctr[(size_t)s * MCTR_COUNT + MCTR_ROWS_LOST];
    if (lost)
        return fail(AZX_ESTATE, "%s: %llu replay rows of finished games did not fit the harvest queue of %lld rows "
                    "or did not add up to their games (internal error)", L.noun, lost, (long long)(sink ? sink->d.q_cap : 0));
    if (sink) {                                          // the rows stay readable until the sink's next play call
        L.rows_last = (int64_t)rows;
        sink->q_rows_valid = (int64_t)rows;
    }
    for (azx_engine *e : L.eng) TRY(check_net_range(e));
    return AZX_OK;
}

extern "C" int azx_match_play(azx_match *m, int64_t first_game, int64_t n_games, int8_t *outcome, int16_t *length,
                              int16_t *moves, azx_match_stats *stats) {
    if (!m) return fail(AZX_EINVAL, "null match");
    if (first_game < 0 || n_games < 1) return fail(AZX_EINVAL, "first_game must be >= 0 and n_games >= 1");
    PlyLoop &L = m->loop;
    azx_engine *a = L.eng[0], *b = L.eng[1];
    ENGINE_GUARD(a);
    TRY(loop_begin(L, n_games, stats, 1));
    const int G = a->d.G, ncells = a->d.ncells;
    const hipStream_t sa = a->stream;
    TRY(loop_grow(L, &m->m.outcome, &m->out_cap, n_games, "outcomes"));
    TRY(loop_grow(L, &m->m.length, &m->len_cap, n_games, "lengths"));
    if (moves) TRY(loop_grow(L, &m->moves_buf, &m->moves_cap, n_games * ncells, "move records"));
    MatchDev M = m->m;
    M.first_game = first_game;
    M.n_games = n_games;
    M.harvest = L.sink >= 0 ? 1 : 0;
    M.first_mode = L.first_mode;
    M.book = L.book;
    M.moves = moves ? m->moves_buf : nullptr;
    if (M.moves) HIPCHECK(hipMemsetAsync(M.moves, 0, sizeof(int16_t) * (size_t)n_games * ncells, sa));
    unsigned long long ctr0[MCTR_COUNT] = {0};
    ctr0[MCTR_NEXT] = (unsigned long long)std::min<int64_t>(G, n_games);
    HIPCHECK(hipMemcpyAsync(M.ctr, ctr0, sizeof ctr0, hipMemcpyHostToDevice, sa));
    // fresh games in every slot of both engines (no generation is used up: the uids are the match's)
    azx_launch_reset(a->d, nullptr, G, nullptr, nullptr, 0, 0, sa);
    azx_launch_reset(b->d, nullptr, G, nullptr, nullptr, 0, 0, sa);
    azx_launch_match_init(a->d, b->d, M, sa);
    if (M.book.n > 0) azx_launch_match_open(a->d, b->d, M, sa);      // the slots' first games from their openings
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(sa));                  // (ctr0 is on this frame)

    // every game ends within `cells` plies and a slot plays its games back to back
    const int64_t max_plies = ((n_games + G - 1) / G + 1) * (int64_t)(ncells + 1);
    TRY(loop_play(L, M.ctr + MCTR_DECIDED, n_games, max_plies, [&] { azx_launch_match_turn(a->d, b->d, M, sa); },
                  [&] { azx_launch_match_step(a->d, b->d, M, sa); }));
    return loop_finish(L, LoopResults{M.ctr, M.outcome, M.length, M.moves}, 1, n_games, outcome, length, moves, stats);
}

// ---- tournaments: P matches side by side in one ply loop, sharing K engines (match_kernels.hip) ----------------
// evaluation.evaluate hands every round's pairs to its pool at once (evaluation.py:29-58); here every pair gets
// `tables_per_pair` tables, a table being slot sa of the pair's first engine and slot sb of its second (an engine's
// pool is partitioned among its opponents, so no engine holds a slot for a pair it is not part of).  Per ply:
//   k_tour_turn                    (engine 0's stream)   whose turn it is at every table -> GameHdr.active
//   engine k's search + move draw  (engine k's stream)   over the active slots of ALL its pairs; forked / joined by events
//   k_tour_step                    (engine 0's stream)   hand-over, game step in both slots, settle per pair, refill
// and ONE word read back: the games decided over all pairs.  Game numbering is the round robin's: round r of pair s is
// game first_game + s * rounds + r, with that uid in both engines, so a pair plays exactly the games of
// azx_match_play(first_game + s * rounds, rounds) between its two engines.
struct azx_tournament {
    PlyLoop loop;
    TourDev t = {};
    DevEngine *eng_dev = nullptr;                // [K]
    TourTable *tab_dev = nullptr;
    int64_t tab_cap = 0, game_cap = 0, ctr_cap = 0, out_cap = 0, len_cap = 0, moves_cap = 0;   // elements held
};

extern "C" void azx_tournament_destroy(azx_tournament *t) {
    if (!t) return;
    DevGuard guard(t->loop.eng[0]->cfg.device);
    loop_destroy(t->loop, {t->eng_dev, t->tab_dev, t->t.tab_game, t->t.ctr, t->t.outcome, t->t.length, t->t.moves});
    delete t;
}

extern "C" int azx_tournament_create(azx_engine *const *engines, int n_engines, azx_tournament **out) {
    if (!engines || !out) return fail(AZX_EINVAL, "null argument");
    if (n_engines < 2) return fail(AZX_EINVAL, "a tournament needs at least two engines (n_engines = %d)", n_engines);
    for (int i = 0; i < n_engines; ++i) {
        azx_engine *e = engines[i];
        if (!e) return fail(AZX_EINVAL, "engine %d is null", i);
        for (int j = 0; j < i; ++j)
            if (engines[j] == e)
                return fail(AZX_EINVAL, "engines %d and %d are the same engine: every agent owns its search tree", j, i);
        if (e->cfg.device != engines[0]->cfg.device)
            return fail(AZX_EINVAL, "engines 0 and %d are on different devices (%d and %d)", i, engines[0]->cfg.device,
                        e->cfg.device);
        if (e->d.N != engines[0]->d.N)
            return fail(AZX_EINVAL, "the board sizes of engines 0 and %d differ (%d and %d)", i, engines[0]->d.N, e->d.N);
        if (const char *why = match_engine_problem(e)) return fail(AZX_EINVAL, "engine %d %s", i, why);
    }
    DevGuard guard(engines[0]->cfg.device);
    azx_tournament *t = new azx_tournament();
    hipError_t err = hipMalloc((void **)&t->eng_dev, sizeof(DevEngine) * (size_t)n_engines);
    err = loop_create(t->loop, err, engines, n_engines, "tournament", nullptr);
    if (err != hipSuccess) {
        azx_tournament_destroy(t);
        return fail(AZX_ENOMEM, "allocating the tournament state failed: %s", hipGetErrorString(err));
    }
    *out = t;
    return AZX_OK;
}

extern "C" int azx_tournament_set_harvest(azx_tournament *t, int sink_engine) {
    if (!t) return fail(AZX_EINVAL, "null tournament");
    const int K = (int)t->loop.eng.size();
    if (sink_engine < -1 || sink_engine >= K)
        return fail(AZX_EINVAL, "sink engine %d: -1 (off) or an engine index below %d", sink_engine, K);
    t->loop.sink = sink_engine;
    return AZX_OK;
}

extern "C" int azx_tournament_set_first_mover(azx_tournament *t, int mode) {
    return loop_set_first_mover(t ? &t->loop : nullptr, "tournament", mode);
}
extern "C" int azx_tournament_set_openings(azx_tournament *t, int n_openings, int stride, const int16_t *moves,
                                           const int32_t *lengths) {
    return loop_set_openings(t ? &t->loop : nullptr, "tournament", n_openings, stride, moves, lengths);
}
extern "C" int azx_tournament_rows(azx_tournament *t, int64_t *rows_out) { return loop_rows(t ? &t->loop : nullptr, rows_out); }

extern "C" int azx_tournament_play(azx_tournament *t, int n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                                   int64_t first_game, int64_t rounds, int32_t tables_per_pair, int8_t *outcome,
                                   int16_t *length, int16_t *moves, azx_match_stats *stats) {
    if (!t) return fail(AZX_EINVAL, "null tournament");
    if (!pair_a || !pair_b || n_pairs < 1) return fail(AZX_EINVAL, "a tournament needs at least one pair (pair_a, pair_b, n_pairs)");
    if (first_game < 0 || rounds < 1 || tables_per_pair < 1)
        return fail(AZX_EINVAL, "first_game must be >= 0, rounds >= 1 and tables_per_pair >= 1");
    PlyLoop &L = t->loop;
    const int K = (int)L.eng.size(), P = n_pairs, T = tables_per_pair;
    // ---- the static slot layout: engine i's pool is partitioned among its opponents, in pair order ----
    std::vector<int> deg((size_t)K, 0);
    std::vector<TourTable> tab((size_t)P * T);
    for (int s = 0; s < P; ++s) {
        const int a = pair_a[s], b = pair_b[s];
        if (a < 0 || a >= K || b < 0 || b >= K)
            return fail(AZX_EINVAL, "pair %d = (%d, %d): engine index out of range (%d engines)", s, a, b, K);
        if (a == b) return fail(AZX_EINVAL, "pair %d = (%d, %d): an engine cannot play itself (a == b)", s, a, b);
        for (int r = 0; r < s; ++r)
            if ((pair_a[r] == a && pair_b[r] == b) || (pair_a[r] == b && pair_b[r] == a))
                return fail(AZX_EINVAL, "pair %d = (%d, %d) repeats pair %d = (%d, %d)", s, a, b, r, pair_a[r], pair_b[r]);
        for (int l = 0; l < T; ++l)
            tab[(size_t)s * T + l] = TourTable{a, deg[a] * T + l, b, deg[b] * T + l, s, l};
        deg[a] += 1;
        deg[b] += 1;
    }
    int max_g = 0;
    for (int k = 0; k < K; ++k) {
        if ((int64_t)deg[k] * T > L.eng[k]->d.G)
            return fail(AZX_EINVAL, "engine %d has n_games = %d slots, its %d pairs at %d tables each need %lld", k,
                        L.eng[k]->d.G, deg[k], T, (long long)deg[k] * T);
        max_g = std::max(max_g, L.eng[k]->d.G);
    }
    const int64_t n_games = (int64_t)P * rounds, n_tables = (int64_t)P * T;
    if (n_tables > (1 << 24)) return fail(AZX_EINVAL, "%lld tables are more than a tournament takes", (long long)n_tables);
    azx_engine *e0 = L.eng[0];
    ENGINE_GUARD(e0);
    TRY(loop_begin(L, n_games, stats, P));
    const int ncells = e0->d.ncells;
    const hipStream_t s0 = e0->stream;
    TRY(loop_grow(L, &t->tab_dev, &t->tab_cap, n_tables, "tables"));
    TRY(loop_grow(L, &t->t.tab_game, &t->game_cap, n_tables, "table games"));
    TRY(loop_grow(L, &t->t.ctr, &t->ctr_cap, (int64_t)(P + 1) * MCTR_COUNT, "counters"));
    TRY(loop_grow(L, &t->t.outcome, &t->out_cap, n_games, "outcomes"));
    TRY(loop_grow(L, &t->t.length, &t->len_cap, n_games, "lengths"));
    if (moves) TRY(loop_grow(L, &t->t.moves, &t->moves_cap, n_games * ncells, "move records"));
    TourDev D = t->t;
    D.eng = t->eng_dev;
    D.tab = t->tab_dev;
    D.n_engines = K;
    D.n_pairs = P;
    D.n_tables = (int32_t)n_tables;
    D.max_g = max_g;
    D.first_game = first_game;
    D.rounds = rounds;
    D.moves = moves ? t->t.moves : nullptr;
    D.sink = L.sink;
    D.first_mode = L.first_mode;
    D.book = L.book;
    std::vector<DevEngine> devs;
    for (azx_engine *e : L.eng) devs.push_back(e->d);
    std::vector<unsigned long long> ctr0((size_t)(P + 1) * MCTR_COUNT, 0ull);
    for (int s = 0; s < P; ++s) ctr0[(size_t)s * MCTR_COUNT + MCTR_NEXT] = (unsigned long long)std::min<int64_t>(T, rounds);
    HIPCHECK(hipMemcpyAsync(t->eng_dev, devs.data(), sizeof(DevEngine) * (size_t)K, hipMemcpyHostToDevice, s0));
    HIPCHECK(hipMemcpyAsync(t->tab_dev, tab.data(), sizeof(TourTable) * tab.size(), hipMemcpyHostToDevice, s0));
    HIPCHECK(hipMemcpyAsync(D.ctr, ctr0.data(), sizeof(unsigned long long) * ctr0.size(), hipMemcpyHostToDevice, s0));
    if (D.moves) HIPCHECK(hipMemsetAsync(D.moves, 0, sizeof(int16_t) * (size_t)n_games * ncells, s0));
    // fresh games in every slot of every engine (no generation is used up: the uids are the tournament's)
    for (azx_engine *e : L.eng) azx_launch_reset(e->d, nullptr, e->d.G, nullptr, nullptr, 0, 0, s0);
    azx_launch_tour_init(D, s0);
    if (D.book.n > 0) azx_launch_tour_open(D, e0->d.slots, s0);      // the tables' first games from their openings
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s0));                  // (the uploads are from this frame)

    // every game ends within `cells` plies and a table plays its pair's games back to back; the block after the
    // pairs' counts the games decided over all pairs
    const int64_t max_plies = ((rounds + T - 1) / T + 1) * (int64_t)(ncells + 1);
    TRY(loop_play(L, D.ctr + (size_t)P * MCTR_COUNT + MCTR_DECIDED, n_games, max_plies, [&] { azx_launch_tour_turn(D, s0); },
                  [&] { azx_launch_tour_step(D, e0->d.slots, s0); }));
    return loop_finish(L, LoopResults{D.ctr, D.outcome, D.length, D.moves}, P, n_games, outcome, length, moves, stats);
}

// ---- native training step (train_kernels.hip) ----------------------------------------------------------------
struct azx_trainer {
    AzxTrain *t = nullptr;
    int device = 0;
};

#define TRAIN_GUARD(h) DevGuard _dev_guard((h)->device)
static int trn_rc(int rc) {
    if (rc) g_err = azx_trn_error();
    return rc;
}

extern "C" int azx_train_create(const azx_train_config *cfg, azx_trainer **out) {
    if (!cfg || !out) return fail(AZX_EINVAL, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(AZX_ENODEV, "no HIP device visible: the training step is HIP-only (no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(AZX_EINVAL, "device %d out of range (%d visible)", cfg->device, ndev);
    DevGuard guard(cfg->device);
    azx_trainer *h = new azx_trainer();
    h->device = cfg->device;
    int rc = azx_trn_create(&h->t, cfg->board_size, cfg->num_blocks, cfg->base_chans, cfg->batch_size, cfg->device);
    if (rc) { delete h; return trn_rc(rc); }
    *out = h;
    return AZX_OK;
}

extern "C" void azx_train_destroy(azx_trainer *h) {
    if (!h) return;
    { TRAIN_GUARD(h); azx_trn_destroy(h->t); }
    delete h;
}

extern "C" int azx_train_bind(azx_trainer *h, int n, const char *const *names, void *const *tensors,
                              const int64_t *counts, void *const *momentum) {
    if (!h || !names || !tensors || !counts) return fail(AZX_EINVAL, "null argument");
    TRAIN_GUARD(h);
    return trn_rc(azx_trn_bind(h->t, n, names, tensors, counts, momentum));
}

extern "C" int azx_train_inputs(azx_trainer *h, int32_t **board, int32_t **legal_moves, float **moves_prob, float **reward) {
    if (!h) return fail(AZX_EINVAL, "null argument");
    return trn_rc(azx_trn_inputs(h->t, board, legal_moves, moves_prob, reward));
}

extern "C" int azx_train_outputs(azx_trainer *h, float **loss3, float **value, float **moves_logprob) {
    if (!h) return fail(AZX_EINVAL, "null argument");
    return trn_rc(azx_trn_outputs(h->t, loss3, value, moves_logprob));
}

extern "C" int azx_train_step(azx_trainer *h, float lr, float momentum, float weight_decay, void *hip_stream) {
    if (!h) return fail(AZX_EINVAL, "null argument");
    TRAIN_GUARD(h);
    return trn_rc(azx_trn_step(h->t, lr, momentum, weight_decay, (hipStream_t)hip_stream));
}

extern "C" int azx_train_debug(azx_trainer *h, const char *name, void *out, int64_t cap, int64_t *nbytes) {
    if (!h || !name || !nbytes) return fail(AZX_EINVAL, "null argument");
    TRAIN_GUARD(h);
    return trn_rc(azx_trn_debug(h->t, name, out, cap, nbytes));
}
