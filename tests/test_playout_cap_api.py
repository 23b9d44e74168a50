"""Playout cap randomisation of device self-play, as far as it can be held without a GPU: the C ABI's three entry points
(declared, bound), the per-ply draw on the host (azx_playout_cap_is_full: the function the kernels use), and the
refusals of Player and train, which come before any engine is made.  The games are tests/test_gpu_playout_cap.py's."""
import ctypes as C
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from option_api_stubs import _Agent, _RandomAgent, _cpu_policy, no_engines  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("azx_set_playout_cap", "azx_playout_cap_is_full", "azx_playout_cap_stats")
EINVAL = -1


def header():
    return open(os.path.join(ROOT, "include", "azx.h")).read()


def L():
    from azalea_amd import _lib
    return _lib.lib()


def test_the_header_declares_the_three_symbols_and_the_binding_requires_them():
    from azalea_amd import _lib
    text = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    assert L().azx_version() == 7
    assert EINVAL == int(re.search(r"AZX_EINVAL\s*=\s*(-?\d+)", text).group(1))
    # azx_config and azx_play_stats are unchanged: the cap is set beside them
    assert len(_lib.Config._fields_) == 18 and len(_lib.PlayStats._fields_) == 20


def test_the_header_states_the_definition_and_that_it_is_not_the_reference():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    sec = text[text.index("Playout cap randomisation"):text.index("int azx_set_playout_cap(")]
    assert "NOT the reference's behaviour" in sec and "off by default" in sec
    assert "azx_version stays 7" in sec and "dlsym azx_set_playout_cap" in sec
    assert "fast_simulations / search_batch_size + 1" in sec and "NO Dirichlet noise" in sec and "NO replay row" in sec
    assert "ceil(full_prob * 2^32)" in sec
    assert "(1.0, 0)" in sec and "leaves the previous setting in place" in sec
    assert "same kernels and returns the same bytes" in sec
    assert "not measured" in sec


def test_the_python_surface():
    from azalea_amd import engine, policy_trainer
    from azalea_amd.parallel_player import Player
    for name in ("set_playout_cap", "clear_playout_cap", "playout_cap_stats"):
        assert callable(getattr(engine.Engine, name)), name
    assert list(inspect.signature(engine.playout_cap_is_full).parameters) == ["seed", "uid", "ply", "full_prob"]
    p = inspect.signature(Player.__init__).parameters["playout_cap"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert "NOT the reference's behaviour" in Player.__init__.__doc__
    assert 'config["playout_cap"]' in policy_trainer.train.__doc__ and "not measured" in policy_trainer.train.__doc__


# ---- the draw -----------------------------------------------------------------------------------------------------
def draws(seed, uids, plies, p):
    f = L().azx_playout_cap_is_full
    return np.array([[f(seed, int(u), int(q), p) for q in plies] for u in uids], np.int64)


def test_the_draw_is_deterministic_and_a_function_of_seed_uid_and_ply():
    from azalea_amd import engine
    a = draws(12345, range(200), range(25), 0.5)
    assert np.array_equal(a, draws(12345, range(200), range(25), 0.5))
    assert set(np.unique(a)) == {0, 1}
    # every argument matters
    assert not np.array_equal(a, draws(12346 + (1 << 40), range(200), range(25), 0.5))
    assert not np.array_equal(a[:100], a[100:])
    assert not np.array_equal(a[:, :12], a[:, 12:24])
    # the key is seed + uid, as for every other stream of a game (game_rng)
    assert np.array_equal(draws(1000, range(50, 60), range(25), 0.5), draws(1050, range(10), range(25), 0.5))
    # the Python wrapper is the same function
    assert [engine.playout_cap_is_full(12345, 7, q, 0.5) for q in range(25)] == [bool(x) for x in a[7]]
    # the bit is a threshold on one word: a ply that is full at p stays full at every larger p
    lo, hi = draws(99, range(300), range(10), 0.25), draws(99, range(300), range(10), 0.6)
    assert (hi >= lo).all() and hi.sum() > lo.sum()


def test_full_prob_one_is_always_full_and_the_smallest_is_almost_never():
    assert draws(7, range(500), range(40), 1.0).all()
    assert draws(0xFFFFFFFFFFFFFFFF, [0, 1, -1, 2 ** 62], [0, 1, 168], 1.0).all()
    assert draws(7, range(500), range(40), 5e-324).sum() == 0          # one word in 2^32 is full


def test_a_bad_full_prob_or_ply_is_refused():
    from azalea_amd import engine
    f = L().azx_playout_cap_is_full
    for p in (0.0, -0.25, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")):
        assert f(1, 2, 3, p) == EINVAL, p
        assert b"full_prob" in L().azx_last_error(), p
        with pytest.raises(ValueError, match="full_prob"):
            engine.playout_cap_is_full(1, 2, 3, p)
    assert f(1, 2, -1, 0.5) == EINVAL and b"ply" in L().azx_last_error()
    assert f(1, 2, 3, 0.5) in (0, 1) and f(1, 2, 3, 1.0) == 1


def test_the_share_of_full_plies_is_the_probability_on_each_ply_parity():
    """20 000 (uid, ply) pairs at p = 0.25: the share of 1s within four binomial standard deviations of 0.25, over
    all pairs and over the even and the odd plies alone (the draw must not favour one colour's moves)."""
    p = 0.25
    a = draws(20261019, range(1000), range(20), p)
    assert a.size == 20000
    for part in (a, a[:, 0::2], a[:, 1::2]):
        sd = math.sqrt(p * (1 - p) / part.size)
        assert abs(part.mean() - p) <= 4 * sd, (part.size, part.mean(), sd)
    # and per ply, over another 20 000 games of one seed: no ply of a game is special (40 tests at four deviations)
    b = draws(5, range(20000), [0, 1], p)
    for q in (0, 1):
        assert abs(b[:, q].mean() - p) <= 4 * math.sqrt(p * (1 - p) / 20000), (q, b[:, q].mean())
    # successive plies of a game are independent draws: P(both full) = p^2 within four deviations
    # (disjoint pairs of plies, so that the pairs are independent trials)
    both = a[:, 0::2] & a[:, 1::2]
    assert abs(both.mean() - p * p) <= 4 * math.sqrt(p * p * (1 - p * p) / both.size), both.mean()


# ---- Player and train: the refusal comes before anything touches a GPU (the stubs of tests/option_api_stubs.py) ---
def test_player_takes_a_cap_for_device_self_play_and_refuses_it_elsewhere(no_engines):
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    assert Player(None, [a]).playout_cap is None
    assert Player(None, [a], playout_cap=(0.25, 4)).playout_cap == (0.25, 4)
    assert Player(None, [a], playout_cap={"full_prob": 1, "fast_simulations": 10}).playout_cap == (1.0, 10)
    # agents that play on the host: two agents, a random mover
    for agents in ([a, b], [_RandomAgent()]):
        with pytest.raises(ValueError, match="playout_cap needs the games to run in a device engine"):
            Player(None, agents, playout_cap=(0.5, 4))
    # a device match records one row per moved ply (the match's own requirements are checked first, as for openings)
    with pytest.raises(ValueError):
        Player(None, [a, b], device_match=True, playout_cap=(0.5, 4))
    # values
    for cap, word in (((0.0, 4), "full_prob"), ((1.5, 4), "full_prob"), ((float("nan"), 4), "full_prob"),
                      ((0.5, 0), "fast_simulations"), ((0.5, 11), "fast_simulations 11 above the policy's simulations 10"),
                      ((0.5, 2.5), "must be"), ((0.5,), "must be"), ("half", "must be"),
                      ({"full_prob": 0.5}, "must be"), ({"full_prob": 0.5, "fast_simulations": 4, "x": 1}, "must be")):
        with pytest.raises(ValueError, match=word):
            Player(None, [a], playout_cap=cap)


def test_device_match_refuses_a_cap_by_name(no_engines, monkeypatch):
    """With the match's own requirements met (stubbed: they need networks on a GPU), the cap is what is refused."""
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    monkeypatch.setattr(Player, "_match_policies", lambda self: [a.policy, b.policy])
    assert Player(None, [a, b], device_match=True).playout_cap is None
    with pytest.raises(ValueError, match="playout_cap is a self-play option"):
        Player(None, [a, b], device_match=True, playout_cap=(0.5, 4))


def test_train_refuses_a_bad_cap_before_it_builds_anything(no_engines, tmp_path, monkeypatch):
    from azalea_amd import policy_trainer

    def refuse(*a, **kw):
        raise AssertionError("train went on after a bad config['playout_cap']")
    monkeypatch.setattr(policy_trainer, "initialize_replay_buffer", refuse)
    monkeypatch.setattr(policy_trainer, "Player", refuse)
    policy = _cpu_policy()
    base = dict(seed=1, device="cpu", game="azalea_amd.game.hex.HexGame", board_size=5)
    for cap, word in (({"full_prob": 0.0, "fast_simulations": 4}, "full_prob"),
                      ({"full_prob": 0.5, "fast_simulations": 0}, "fast_simulations"),
                      ({"full_prob": 0.5, "fast_simulations": 11}, "fast_simulations 11 above simulations 10"),
                      ({"full_prob": 0.5}, "must be"), ({"p": 0.5, "fast_simulations": 4}, "must be")):
        with pytest.raises(ValueError, match=word):
            policy_trainer.train(policy, dict(base, playout_cap=cap), str(tmp_path / "run"))
    assert not (tmp_path / "run").exists()
