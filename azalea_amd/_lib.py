"""ctypes binding of libazx_hip.so (include/azx.h).

The HIP engine is the product: if the shared object is missing or no MI355X is visible the
calls fail loudly -- there is deliberately no CPU fallback (and nothing here imports oracle/).
"""
import ctypes as C
import logging
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libazx_hip.so")

MAX_BOARD = 13
CELL_STRIDE = 192
MAX_BATCH = 16
ROW_METRICS = 8          # AZX_ROW_METRICS


def record_bytes(cells):
    """AZX_RECORD_BYTES (include/azx.h): one fixed-size replay record."""
    return (16 + 5 * cells + 15) // 16 * 16

EVAL_RESNET, EVAL_UNIFORM, EVAL_UNIFORM_HASH, EVAL_EXTERNAL = 0, 1, 2, 3
FLAG_NO_COMPACT = 1
FLAG_RANDOM_REFLECT = 2  # AZX_FLAG_RANDOM_REFLECT: evaluation requests randomly turned by 180 degrees (opt-in)
FLAG_TOWER_F16 = 4       # AZX_FLAG_TOWER_F16: the plain-f16 tower, one MFMA per product (opt-in, outside every parity claim)
EEXTERNAL = -7           # AZX_EEXTERNAL: the registered external evaluator failed or produced a bad row


class AzxError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("board_size", C.c_int32), ("n_games", C.c_int32), ("simulations", C.c_int32),
                ("search_batch_size", C.c_int32), ("exploration_coef", C.c_float),
                ("exploration_depth", C.c_int32), ("noise_alpha", C.c_double),
                ("noise_scale", C.c_double), ("temperature", C.c_double),
                ("evaluator", C.c_int32), ("num_blocks", C.c_int32), ("base_chans", C.c_int32),
                ("nodes_per_game", C.c_int32), ("flags", C.c_int32), ("device", C.c_int32),
                ("seed", C.c_uint64), ("game_index_stride", C.c_int32), ("game_index_offset", C.c_int32)]


class PlayStats(C.Structure):
    _fields_ = [("positions", C.c_int64), ("games", C.c_int64), ("game_errors", C.c_int64),
                ("plies", C.c_int64), ("selects", C.c_int64), ("evals", C.c_int64),
                ("sum_depth", C.c_int64), ("sum_k_interior", C.c_int64),
                ("sum_k_leaf", C.c_int64), ("sum_search_value", C.c_double),
                ("sum_root_width", C.c_double), ("sum_action_logprob", C.c_double),
                ("sum_reward_last", C.c_double), ("seconds", C.c_double),
                ("mcts_seconds", C.c_double), ("mcts_launches", C.c_int64),
                ("net_seconds", C.c_double), ("net_launches", C.c_int64),
                ("mcts_kernel_launches", C.c_int64), ("sum_game_length", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class MatchStats(C.Structure):
    """azx_match_stats (include/azx.h)."""
    _fields_ = [("games", C.c_int64), ("wins", C.c_int64 * 2), ("first_player_wins", C.c_int64),
                ("voided", C.c_int64), ("plies", C.c_int64), ("seconds", C.c_double)]

    def as_dict(self):
        return dict(games=self.games, wins=[self.wins[0], self.wins[1]], first_player_wins=self.first_player_wins,
                    voided=self.voided, plies=self.plies, seconds=self.seconds)


_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_u64p = C.POINTER(C.c_uint64)
_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)
_vp = C.c_void_p

# azx_eval_fn (include/azx.h): user, n, kmax, board_dev, legal_moves_dev, value_dev, prior_dev, hip_stream
EVAL_FN = C.CFUNCTYPE(C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp)

# every symbol include/azx.h declares: (restype, argtypes)
SYMBOLS = {
    "azx_last_error": (C.c_char_p, []),
    "azx_version": (C.c_int, []),
    "azx_create": (C.c_int, [C.POINTER(Config), C.POINTER(_vp)]),
    "azx_destroy": (None, [_vp]),
    "azx_set_weights": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(_vp), _i64p, C.c_int]),
    "azx_debug_weights": (C.c_int, [_vp, C.c_int, _vp, C.c_int64, _i64p, C.c_char_p, C.c_int]),
    "azx_set_prior_table": (C.c_int, [_vp, _f32p, C.c_int]),
    "azx_reset": (C.c_int, [_vp, _i32p, C.c_int, _i32p, _i32p, C.c_int]),
    "azx_set_active": (C.c_int, [_vp, _i32p]),
    "azx_search": (C.c_int, [_vp, _f64p, C.c_int, C.c_int, C.c_double]),
    "azx_search_begin": (C.c_int, [_vp, _f64p, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int)]),
    "azx_search_step": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "azx_get_leaves": (C.c_int, [_vp, C.c_int, _i32p, _i32p, _i32p, _i32p, C.POINTER(C.c_int)]),
    "azx_put_evals": (C.c_int, [_vp, C.c_int, _f32p, _f32p]),
    "azx_get_evals": (C.c_int, [_vp, C.c_int, _f32p, _f32p, C.POINTER(C.c_int)]),
    "azx_get_root": (C.c_int, [_vp, _i32p, _i32p, _f32p, _f32p, _f32p, _f32p, _f32p, _i32p, _f32p]),
    "azx_get_status": (C.c_int, [_vp, _i32p]),
    "azx_get_tree_nodes": (C.c_int, [_vp, _i32p]),
    "azx_get_games": (C.c_int, [_vp, _i32p, _i32p, _i32p, _i32p]),
    "azx_advance": (C.c_int, [_vp, _i32p]),
    "azx_tree_dump": (C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _i32p, _f32p, _f32p, _f32p, _i32p, _i32p]),
    "azx_forward": (C.c_int, [_vp, C.c_int, C.c_int, _i32p, _i32p, _f32p, _f32p]),
    "azx_hex_replay": (C.c_int, [C.c_int, C.c_int, C.c_int, _i32p, _i32p, C.c_int, _i32p, _i32p, _u64p, _i32p]),
    "azx_play": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, _i32p, _i32p, _i32p, _f32p, _f32p, _i64p, C.POINTER(PlayStats)]),
    "azx_play_row_metrics": (C.c_int, [_vp, C.c_int64, _f32p, _i64p]),
    "azx_play_steps": (C.c_int, [_vp, C.c_int64, C.POINTER(PlayStats)]),
    "azx_replay_create": (C.c_int, [_vp, C.c_int64]),
    "azx_replay_state": (C.c_int, [_vp, _i64p, _i64p, _i64p]),
    "azx_replay_set_state": (C.c_int, [_vp, C.c_int64, C.c_int64]),
    "azx_replay_put": (C.c_int, [_vp, C.c_int64, _i32p, _i32p, _i32p, _f32p, _f32p]),
    "azx_replay_fill": (C.c_int, [_vp, C.c_int64, C.c_int64, _i64p, C.POINTER(PlayStats)]),
    "azx_play_device": (C.c_int, [_vp, C.c_int64, C.c_int64, _i64p, C.POINTER(PlayStats)]),
    "azx_rows_pack": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp]),
    "azx_replay_put_records": (C.c_int, [_vp, C.c_int64, _vp]),
    "azx_replay_put_records_async": (C.c_int, [_vp, C.c_int64, _vp, _vp]),
    "azx_reserve_cus": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    "azx_replay_collate": (C.c_int, [_vp, C.c_int64, _i64p, _vp, _vp, _vp, _vp, _vp, _vp, _i32p]),
    "azx_replay_collate_async": (C.c_int, [_vp, C.c_int64, _i64p, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "azx_replay_set_mover_view": (C.c_int, [_vp, C.c_int]),
    "azx_replay_set_reflect": (C.c_int, [_vp, C.c_int, C.c_uint64]),
    "azx_selftest_arith": (C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p, _f32p]),
    "azx_selftest_divide": (C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, _f32p]),
    "azx_selftest_dirichlet": (C.c_int, [C.c_int, C.c_double, C.c_int, C.c_int, C.c_uint32, _f32p]),
    "azx_debug_choose": (C.c_int, [_vp, _i32p, _f32p]),
    "azx_debug_counters": (C.c_int, [_vp, _u64p]),
    "azx_debug_counters_raw": (C.c_int, [_vp, _u64p, C.c_int64]),
    "azx_debug_slow_div": (C.c_int, [_vp, _i32p]),
    "azx_kernel_info": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "azx_debug_set_queue_cap": (C.c_int, [_vp, C.c_int64]),
    "azx_debug_stagger": (C.c_int, [_vp, _i32p]),
    "azx_debug_tower_tiles": (C.c_int, [C.c_int, C.c_char_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), _i32p]),
    "azx_debug_tower_choice": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]),
    "azx_stream": (_vp, [_vp]),
    "azx_set_external_evaluator": (C.c_int, [_vp, _vp, _vp]),   # fn passed as a pointer (NULL = unregister)
    "azx_match_create": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "azx_match_destroy": (None, [_vp]),
    "azx_match_play": (C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_int8), C.POINTER(C.c_int16),
                                 C.POINTER(C.c_int16), C.POINTER(MatchStats)]),
    "azx_tournament_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.POINTER(_vp)]),
    "azx_tournament_destroy": (None, [_vp]),
    "azx_tournament_play": (C.c_int, [_vp, C.c_int, _i32p, _i32p, C.c_int64, C.c_int64, C.c_int32,
                                      C.POINTER(C.c_int8), C.POINTER(C.c_int16), C.POINTER(C.c_int16),
                                      C.POINTER(MatchStats)]),
    # replay rows from matches / tournaments (additions within revision 7)
    "azx_match_set_harvest": (C.c_int, [_vp, C.c_int]),
    "azx_match_set_first_mover": (C.c_int, [_vp, C.c_int]),
    "azx_match_rows": (C.c_int, [_vp, _i64p]),
    "azx_tournament_set_harvest": (C.c_int, [_vp, C.c_int]),
    "azx_tournament_set_first_mover": (C.c_int, [_vp, C.c_int]),
    "azx_tournament_rows": (C.c_int, [_vp, _i64p]),
    "azx_rows_read": (C.c_int, [_vp, C.c_int64, C.c_int64, _i32p, _i32p, _i32p, _f32p, _f32p, _i64p]),
    # opening books of matches / tournaments (additions within revision 7)
    "azx_openings_check": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int16), _i32p, _i32p, _i32p]),
    "azx_match_set_openings": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int16), _i32p]),
    "azx_tournament_set_openings": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int16), _i32p]),
    # weighted opening book of device self-play (additions within revision 7; NOT the reference's behaviour)
    "azx_set_selfplay_openings": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int16), _i32p, C.POINTER(C.c_double)]),
    "azx_selfplay_opening_word": (C.c_int, [C.c_uint64, C.c_int64, C.POINTER(C.c_uint32)]),
    "azx_selfplay_openings_bounds": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "azx_selfplay_openings_slots": (C.c_int, [_vp, _i32p]),
    "azx_selfplay_openings_stats": (C.c_int, [_vp, C.c_int64, _i64p]),
    # playout cap randomisation of throughput self-play (additions within revision 7; NOT the reference's behaviour)
    "azx_set_playout_cap": (C.c_int, [_vp, C.c_double, C.c_int]),
    "azx_playout_cap_is_full": (C.c_int, [C.c_uint64, C.c_int64, C.c_int, C.c_double]),
    "azx_playout_cap_stats": (C.c_int, [_vp, _i64p]),
    # resignation for throughput self-play (additions within revision 7; NOT the reference's behaviour)
    "azx_set_resign": (C.c_int, [_vp, C.c_double, C.c_int, C.c_double]),
    "azx_clear_resign": (C.c_int, [_vp]),
    "azx_resign_is_exempt": (C.c_int, [C.c_uint64, C.c_int64, C.c_double]),
    "azx_resign_stats": (C.c_int, [_vp, _i64p]),
    "azx_resign_value": (C.c_int, [_vp, C.POINTER(C.c_float)]),
    # early stop of decided searches in throughput self-play (additions within revision 7; NOT the reference's behaviour)
    "azx_set_early_stop": (C.c_int, [_vp, C.c_int]),
    "azx_early_stop_stats": (C.c_int, [_vp, _i64p]),
    # training targets of the recorded rows: visit-share rows, z/q-blended rewards (additions within revision 7; NOT the
    # reference's behaviour)
    "azx_set_train_targets": (C.c_int, [_vp, C.c_int, C.c_float]),
    "azx_get_train_targets": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "azx_train_targets_stats": (C.c_int, [_vp, _i64p]),
    # forced playouts at the root and policy target pruning (additions within revision 7; NOT the reference's behaviour)
    "azx_set_forced_playouts": (C.c_int, [_vp, C.c_float, C.c_int]),
    "azx_get_forced_playouts": (C.c_int, [_vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "azx_forced_playouts_stats": (C.c_int, [_vp, _i64p]),
    # Gumbel root search with sequential halving (additions within revision 7; NOT the reference's behaviour)
    "azx_set_gumbel": (C.c_int, [_vp, C.c_int, C.c_float, C.c_float, C.c_int]),
    "azx_get_gumbel": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "azx_gumbel_stats": (C.c_int, [_vp, _i64p]),
    "azx_gumbel_variate": (C.c_int, [C.c_uint64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "azx_selftest_gumbel": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_uint32), _f32p]),
    "azx_gumbel_state": (C.c_int, [_vp, _u64p, _u64p]),
    # rollout evaluator: a network-free MCTS opponent (additions within revision 7; NOT the reference's behaviour)
    "azx_set_rollout_evaluator": (C.c_int, [_vp, C.c_int, C.c_uint64]),
    "azx_rollout_value": (C.c_int, [C.c_uint64, C.c_int, _i32p, C.c_int, _i32p, _f32p]),
    "azx_selftest_rollout": (C.c_int, [C.c_int, C.c_int, C.c_int, _i32p, C.c_int, C.c_uint64, _i32p, _f32p, _f32p,
                                       C.POINTER(C.c_uint8)]),
    "azx_rollout_stats": (C.c_int, [_vp, _i64p]),
    # first-play urgency of the PUCT search (additions within revision 7; NOT the reference's behaviour)
    "azx_set_fpu": (C.c_int, [_vp, C.c_int, C.c_float, C.c_float, C.c_float]),
    "azx_get_fpu": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "azx_fpu_stats": (C.c_int, [_vp, _i64p]),
    "azx_fpu_score": (C.c_int, [C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float,
                                _f32p, _f32p, _f32p, C.c_float, _i32p]),
    # policy temperature of the search's priors (additions within revision 7; NOT the reference's behaviour)
    "azx_set_policy_temp": (C.c_int, [_vp, C.c_int, C.c_int]),
    "azx_get_policy_temp": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "azx_policy_temp_stats": (C.c_int, [_vp, _i64p]),
    "azx_policy_temp_row": (C.c_int, [C.c_int, C.c_int, _f32p, _f32p, C.POINTER(C.c_int)]),
}

class TrainConfig(C.Structure):
    _fields_ = [("board_size", C.c_int32), ("num_blocks", C.c_int32), ("base_chans", C.c_int32),
                ("batch_size", C.c_int32), ("device", C.c_int32)]


_pp = C.POINTER(_vp)
SYMBOLS.update({
    "azx_train_create": (C.c_int, [C.POINTER(TrainConfig), C.POINTER(_vp)]),
    "azx_train_destroy": (None, [_vp]),
    "azx_train_bind": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_char_p), _pp, _i64p, _pp]),
    "azx_train_inputs": (C.c_int, [_vp, _pp, _pp, _pp, _pp]),
    "azx_train_outputs": (C.c_int, [_vp, _pp, _pp, _pp]),
    "azx_train_step": (C.c_int, [_vp, C.c_float, C.c_float, C.c_float, _vp]),
    "azx_train_debug": (C.c_int, [_vp, C.c_char_p, _vp, C.c_int64, _i64p]),
})

# entry points that a library may lack without lib() refusing it.  Empty for the package itself: a tool that loads an
# older build in this package's place (tools/lib_bench.py) names the later additions here before the first lib().
OPTIONAL = set()

_lib = None


def build(force=False):
    """Compile libazx_hip.so for gfx950 with hipcc (azalea_amd/csrc/Makefile)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc")]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    """Load the HIP engine; raises if it has not been built (no fallback path exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AzxError(
                "azalea_amd/libazx_hip.so is missing: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C azalea_amd/csrc`. "
                "The engine is HIP-only; there is no CPU fallback.")
        # PyTorch-ROCm ships its own HIP / HSA runtime.  If this library (linked against /opt/rocm's) brings the GPU up
        # first, a later first use of torch.cuda in the same process fails with "No HIP GPUs are available" -- and
        # every Policy holds its weights in torch tensors.  So where torch is installed and sees a GPU, its runtime is
        # initialised before ours is loaded; the order then no longer depends on what the caller touched first.
        # (AZX_NO_TORCH_PREINIT=1 skips this for consumers of the bare C API that never touch torch.)
        if not os.environ.get("AZX_NO_TORCH_PREINIT"):
            try:
                import torch
                if torch.cuda.is_available():
                    torch.cuda.init()
            except (ImportError, RuntimeError) as exc:      # no torch / no usable GPU: the engine reports AZX_ENODEV where it matters
                logging.getLogger(__name__).debug("torch pre-initialisation skipped: %r", exc)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            if name in OPTIONAL and not hasattr(L, name):
                continue
            fn = getattr(L, name)   # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise AzxError("azx error %d: %s" % (rc, lib().azx_last_error().decode(errors="replace")))
