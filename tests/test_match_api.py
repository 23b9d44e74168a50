"""The match entry points (azx_match_*: evaluation games between two engines on the device) at the C boundary and
the argument checks of evaluation.evaluate_throughput -- everything that can be held without a GPU.  The games
themselves are tests/test_gpu_match.py's."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from option_api_stubs import _Agent  # noqa: E402,F401
MATCH_SYMBOLS = ("azx_match_create", "azx_match_destroy", "azx_match_play")


def header():
    return open(os.path.join(ROOT, "include", "azx.h")).read()


def test_header_declares_the_match_entry_points_and_the_library_exports_them():
    from azalea_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(azx_[a-z_0-9]+)\s*\(", code))
    for name in MATCH_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r"\}\s*azx_match_stats\s*;", code) and "typedef struct azx_match azx_match;" in code


def test_abi_revision_is_unchanged():
    """The match calls are an addition within revision 7: callers detect them by symbol."""
    from azalea_amd import _lib
    assert _lib.lib().azx_version() == 7


def test_match_stats_matches_the_header(tmp_path):
    from azalea_amd import _lib
    fields = [f for f, _ in _lib.MatchStats._fields_]
    assert fields == ["games", "wins", "first_player_wins", "voided", "plies", "seconds"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "azx.h"', 'int main(void) {',
             'printf("azx_match_stats %zu\\n", sizeof(azx_match_stats));']
    for f in fields:
        lines.append('printf("%s %%zu\\n", offsetof(azx_match_stats, %s));' % (f, f))
    lines.append('printf("wins_len %zu\\n", sizeof(((azx_match_stats *)0)->wins) / sizeof(int64_t));')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["azx_match_stats"]) == C.sizeof(_lib.MatchStats)
    assert int(got["wins_len"]) == 2
    for f in fields:
        assert int(got[f]) == getattr(_lib.MatchStats, f).offset, f


def test_match_create_rejects_null_engines():
    from azalea_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.azx_match_create(None, None, C.byref(h)) == -1          # AZX_EINVAL
    assert not h.value
    assert L.azx_last_error()
    assert L.azx_match_play(None, 0, 1, None, None, None, None) == -1
    L.azx_match_destroy(None)                                        # a null match is ignored


def test_evaluate_throughput_rejects_agents_without_a_device_network():
    """The same check evaluate_batched makes, before anything touches a GPU: the random mover has no Policy, and a
    Policy around a duck-typed network has no HexNetwork for the engine to run."""
    import torch
    from azalea_amd import evaluation
    from azalea_amd.policy import Policy
    from azalea_amd.random_policy import RandomPolicy

    class Duck(torch.nn.Module):
        def run(self, batch):
            raise AssertionError("never evaluated")

    duck = Policy()
    duck.net = Duck()
    good = Policy()
    good.initialize(dict(device="cpu", network="HexNetwork", board_size=5, num_blocks=1, base_chans=32,
                         simulations=10, search_batch_size=2, exploration_coef=0.5, exploration_depth=3,
                         exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0))
    for bad in (_Agent(RandomPolicy()), _Agent(duck), _Agent(None)):
        with pytest.raises(TypeError):
            evaluation.evaluate_throughput([_Agent(good), bad], 4)
        with pytest.raises(TypeError):
            evaluation.evaluate_throughput([bad, _Agent(good)], 4)


def test_oracle_match_comparison_sees_a_match_played_with_one_agents_settings(tmp_path):
    """Power of the distribution test of tests/test_gpu_match.py, oracle against oracle (case A: 60 against 10
    simulations): a match in which BOTH agents search with agent 0's settings -- the obvious way to mix the two
    engines up -- is rejected on the win rate and on the game lengths, while two honest samples on disjoint seeds
    agree."""
    import game_stats as gs
    import oracle_match_games as omg
    base = dict(batch=10, c=0.5, depth=6, alpha=0.3, eps=0.0, temp=1.0)
    cfgs = [dict(base, sims=60), dict(base, sims=10)]
    games = 4096
    a = omg.sample(7, cfgs, games, 0)
    b = omg.sample(7, cfgs, games, 1000000)
    same = omg.compare(a, b)
    print("oracle vs oracle:", same)
    assert min(same.values()) > min(gs.P_MIN, 0.05 / len(same)), same
    assert 0.6 < a["agent0_wins"].mean() < 0.8               # the stronger searcher wins
    w = omg.sample(7, [cfgs[0], cfgs[0]], games, 2000000)
    wrong = omg.compare(a, w)
    print("against equal settings:", wrong)
    assert wrong["agent0_wins"] < 1e-30 and wrong["length"] < 1e-30, wrong
