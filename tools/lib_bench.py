"""Diagnostic: run bench.py's resnet workload against an alternative build of the library (tools only)."""
import sys, os, runpy
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from azalea_amd import _lib
_lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), sys.argv[1])
# an older build lacks the entry points added since (callers detect those by symbol: include/azx.h)
_lib.OPTIONAL.update(["azx_debug_stagger"])
_lib.OPTIONAL.update(["azx_match_set_harvest", "azx_match_set_first_mover", "azx_match_rows", "azx_tournament_set_harvest",
                      "azx_tournament_set_first_mover", "azx_tournament_rows", "azx_rows_read"])
_lib.OPTIONAL.update(["azx_replay_set_reflect"])
_lib.OPTIONAL.update(["azx_openings_check", "azx_match_set_openings", "azx_tournament_set_openings"])
_lib.OPTIONAL.update(["azx_set_playout_cap", "azx_playout_cap_is_full", "azx_playout_cap_stats"])
_lib.OPTIONAL.update(["azx_set_resign", "azx_clear_resign", "azx_resign_is_exempt", "azx_resign_stats", "azx_resign_value"])
_lib.OPTIONAL.update(["azx_set_early_stop", "azx_early_stop_stats"])
_lib.OPTIONAL.update(["azx_set_train_targets", "azx_get_train_targets", "azx_train_targets_stats"])
_lib.OPTIONAL.update(["azx_debug_tower_tiles"])
_lib.OPTIONAL.update(["azx_set_forced_playouts", "azx_get_forced_playouts", "azx_forced_playouts_stats"])
_lib.OPTIONAL.update(["azx_set_selfplay_openings", "azx_selfplay_opening_word", "azx_selfplay_openings_bounds",
                      "azx_selfplay_openings_slots", "azx_selfplay_openings_stats"])
_lib.OPTIONAL.update(["azx_set_gumbel", "azx_get_gumbel", "azx_gumbel_stats", "azx_gumbel_variate", "azx_selftest_gumbel",
                      "azx_gumbel_state"])
_lib.OPTIONAL.update(["azx_set_rollout_evaluator", "azx_rollout_value", "azx_selftest_rollout", "azx_rollout_stats"])
_lib.OPTIONAL.update(["azx_debug_tower_choice"])
_lib.OPTIONAL.update(["azx_set_fpu", "azx_get_fpu", "azx_fpu_stats", "azx_fpu_score"])
_lib.OPTIONAL.update(["azx_set_policy_temp", "azx_get_policy_temp", "azx_policy_temp_stats", "azx_policy_temp_row"])
sys.argv = ["bench.py"] + sys.argv[2:]
runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"), run_name="__main__")
