"""Resignation of device self-play with no-resign calibration games, as far as it can be held without a GPU: the C ABI's
five entry points (declared, bound), the per-game exemption draw on the host (azx_resign_is_exempt: the function the
kernels use), and the refusals of Player and train, which come before any engine is made.  The games are
tests/test_gpu_resign.py's."""
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
NEW_SYMBOLS = ("azx_set_resign", "azx_clear_resign", "azx_resign_is_exempt", "azx_resign_stats", "azx_resign_value")
EINVAL = -1


def header():
    return open(os.path.join(ROOT, "include", "azx.h")).read()


def L():
    from azalea_amd import _lib
    return _lib.lib()


def test_the_header_declares_the_five_symbols_and_the_binding_requires_them():
    from azalea_amd import _lib
    text = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    assert L().azx_version() == 7
    assert EINVAL == int(re.search(r"AZX_EINVAL\s*=\s*(-?\d+)", text).group(1))
    # azx_config and azx_play_stats are unchanged: resignation is set beside them
    assert len(_lib.Config._fields_) == 18 and len(_lib.PlayStats._fields_) == 20
    # the benchmark's loader of older libraries treats the five as optional
    tool = open(os.path.join(ROOT, "tools", "lib_bench.py")).read()
    for name in NEW_SYMBOLS:
        assert '"%s"' % name in tool, name


def test_the_header_states_the_definition_and_that_it_is_not_the_reference():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    sec = text[text.index("Resignation for throughput self-play"):text.index("int azx_resign_value(")]
    assert "NOT the reference's behaviour" in sec and "off by default" in sec
    assert "azx_version stays 7" in sec and "dlsym azx_set_resign" in sec
    assert "root.total_value / root.num_visits" in sec and "ONE float32 IEEE division" in sec
    assert "positive is good for the mover" in sec
    assert "ceil(keep_prob * 2^32) - 1" in sec
    assert "leaves the previous setting in place" in sec
    assert "same kernels and returns the same bytes" in sec
    assert "NOT measured" in sec
    # the five declarations sit in (or right after) that section, before the next one
    tail = text[text.index("int azx_set_resign("):]
    for name in NEW_SYMBOLS:
        assert tail.index("int %s(" % name) < tail.index("float32 arithmetic self-test"), name


def test_the_python_surface():
    from azalea_amd import engine, policy_trainer
    from azalea_amd.parallel_player import Player
    for name in ("set_resign", "clear_resign", "resign_stats", "resign_values"):
        assert callable(getattr(engine.Engine, name)), name
    sig = inspect.signature(engine.Engine.set_resign).parameters
    assert list(sig) == ["self", "threshold", "min_ply", "keep_prob"]
    assert sig["min_ply"].default == 0 and sig["keep_prob"].default == 0.1
    assert list(inspect.signature(engine.resign_is_exempt).parameters) == ["seed", "uid", "keep_prob"]
    assert engine.Engine.RESIGN_STATS == ("resigned", "played_out", "exempt", "exempt_crossed", "false_positives",
                                          "sum_resign_ply", "sum_plies_saved")
    p = inspect.signature(Player.__init__).parameters["resign"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert "which plays every game to the end" in Player.__init__.__doc__
    doc = policy_trainer.train.__doc__
    assert 'config["resign"]' in doc and "does NOT get it" in doc and "not measured" in doc


# ---- the exemption draw -------------------------------------------------------------------------------------------
def exempt(seed, uids, p):
    f = L().azx_resign_is_exempt
    return np.array([f(seed, int(u), p) for u in uids], np.int64)


def test_keep_prob_zero_exempts_none_and_one_exempts_all():
    uids = range(10 ** 4)
    assert exempt(4242, uids, 0.0).sum() == 0
    assert exempt(4242, uids, 1.0).all()
    assert exempt(0xFFFFFFFFFFFFFFFF, [0, 1, -1, 2 ** 62], 1.0).all()
    assert exempt(0xFFFFFFFFFFFFFFFF, [0, 1, -1, 2 ** 62], 0.0).sum() == 0


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_the_exempt_share_is_keep_prob(p):
    n = 10 ** 5
    a = exempt(20261019, range(n), p)
    assert set(np.unique(a)) == {0, 1}
    bound = 5 * math.sqrt(p * (1 - p) / n)
    assert abs(a.mean() - p) <= bound, (a.mean(), bound)


def test_the_draw_is_a_function_of_seed_plus_uid_and_monotone_in_keep_prob():
    from azalea_amd import engine
    a = exempt(12345, range(2000), 0.5)
    assert np.array_equal(a, exempt(12345, range(2000), 0.5))
    assert not np.array_equal(a, exempt(12346 + (1 << 40), range(2000), 0.5))
    assert not np.array_equal(a[:1000], a[1000:])
    # the key is seed + uid, as for every other stream of a game (game_rng)
    assert np.array_equal(exempt(1000, range(50, 150), 0.5), exempt(1050, range(100), 0.5))
    # the Python wrapper is the same function
    assert [engine.resign_is_exempt(12345, u, 0.5) for u in range(200)] == [bool(x) for x in a[:200]]
    assert engine.resign_is_exempt(12345, 3, 0.0) is False and engine.resign_is_exempt(12345, 3, 1.0) is True
    # the bit is a threshold on one word: a game exempt at p stays exempt at every larger p
    ladder = [exempt(99, range(3000), p) for p in (0.0, 1e-9, 0.1, 0.25, 0.5, 0.75, 0.999, 1.0)]
    for lo, hi in zip(ladder, ladder[1:]):
        assert (hi >= lo).all()
    assert ladder[3].sum() < ladder[5].sum()


def test_the_stream_is_not_the_playout_caps():
    """Over the same uids at p = 0.5 the exemption bit agrees with the cap's bit of ply 0 on about half of them: the
    share of agreements lies within five binomial deviations of 0.5."""
    n, p, seed = 10 ** 5, 0.5, 20261019
    a = exempt(seed, range(n), p)
    cap = L().azx_playout_cap_is_full
    b = np.array([cap(seed, u, 0, p) for u in range(n)], np.int64)
    agree = (a == b).mean()
    bound = 5 * math.sqrt(p * (1 - p) / n)
    assert abs(agree - 0.5) <= bound, (agree, bound)


def test_a_bad_keep_prob_is_refused():
    from azalea_amd import engine
    f = L().azx_resign_is_exempt
    for p in (-0.25, -1e-300, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")):
        assert f(1, 2, p) == EINVAL, p
        assert b"keep_prob" in L().azx_last_error(), p
        with pytest.raises(ValueError, match="keep_prob"):
            engine.resign_is_exempt(1, 2, p)
    assert f(1, 2, 0.5) in (0, 1) and f(1, 2, 1.0) == 1 and f(1, 2, 0.0) == 0


def test_null_engines_are_einval_before_any_device_work():
    lib = L()
    assert lib.azx_set_resign(None, -0.9, 0, 0.1) == EINVAL and b"null" in lib.azx_last_error()
    assert lib.azx_clear_resign(None) == EINVAL
    assert lib.azx_resign_stats(None, None) == EINVAL
    assert lib.azx_resign_value(None, None) == EINVAL


# ---- Player and train: the refusal comes before anything touches a GPU (the stubs of tests/option_api_stubs.py) -----
BAD = (((-1.5, 4, 0.1), "threshold"), ((1.01, 4, 0.1), "threshold"), ((float("nan"), 4, 0.1), "threshold"),
       ((-0.9, -1, 0.1), "min_ply"), ((-0.9, 2.5, 0.1), "must be"), ((-0.9, True, 0.1), "must be"),
       ((-0.9, 4, -0.1), "keep_prob"), ((-0.9, 4, 1.5), "keep_prob"), ((-0.9, 4, float("nan")), "keep_prob"),
       ((-0.9, 4), "must be"), ("never", "must be"), ({"threshold": -0.9}, "must be"),
       ({"threshold": -0.9, "min_ply": 4, "keep_prob": 0.1, "x": 1}, "must be"))


def test_player_takes_resign_for_device_self_play_and_refuses_it_elsewhere(no_engines):
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    assert Player(None, [a]).resign is None
    assert Player(None, [a], resign=(-0.9, 10, 0.1)).resign == (-0.9, 10, 0.1)
    assert Player(None, [a], resign={"threshold": -1, "min_ply": 0, "keep_prob": 1}).resign == (-1.0, 0, 1.0)
    assert Player(None, [a], resign=(1.0, 0, 0.0)).resign == (1.0, 0, 0.0)
    assert Player(None, [a], resign=(-0.9, 10, 0.1)).resign_stats() is None        # no engine yet
    # agents that play on the host: two agents, a random mover
    for agents in ([a, b], [_RandomAgent()]):
        with pytest.raises(ValueError, match="resign needs the games to run in a device engine"):
            Player(None, agents, resign=(-0.9, 10, 0.1))
    with pytest.raises(ValueError):
        Player(None, [a, b], device_match=True, resign=(-0.9, 10, 0.1))
    for value, word in BAD:
        with pytest.raises(ValueError, match=word):
            Player(None, [a], resign=value)


def test_device_match_refuses_resign_by_name(no_engines, monkeypatch):
    """With the match's own requirements met (stubbed: they need networks on a GPU), resign is what is refused."""
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    monkeypatch.setattr(Player, "_match_policies", lambda self: [a.policy, b.policy])
    assert Player(None, [a, b], device_match=True).resign is None
    with pytest.raises(ValueError, match="resign is a self-play option"):
        Player(None, [a, b], device_match=True, resign=(-0.9, 10, 0.1))


def test_train_refuses_a_bad_resign_before_it_builds_anything(no_engines, tmp_path, monkeypatch):
    from azalea_amd import policy_trainer

    def refuse(*a, **kw):
        raise AssertionError("train went on after a bad config['resign']")
    monkeypatch.setattr(policy_trainer, "initialize_replay_buffer", refuse)
    monkeypatch.setattr(policy_trainer, "Player", refuse)
    policy = _cpu_policy()
    base = dict(seed=1, device="cpu", game="azalea_amd.game.hex.HexGame", board_size=5)
    for value, word in (({"threshold": -2.0, "min_ply": 4, "keep_prob": 0.1}, "threshold"),
                        ({"threshold": -0.9, "min_ply": -4, "keep_prob": 0.1}, "min_ply"),
                        ({"threshold": -0.9, "min_ply": 4, "keep_prob": 1.1}, "keep_prob"),
                        ({"threshold": -0.9}, "must be"), ({"t": -0.9, "min_ply": 4, "keep_prob": 0.1}, "must be")):
        with pytest.raises(ValueError, match=word):
            policy_trainer.train(policy, dict(base, resign=value), str(tmp_path / "run"))
    assert not (tmp_path / "run").exists()


def test_train_hands_resign_to_the_self_play_player_only(no_engines, tmp_path, monkeypatch):
    """train() fills the first buffer with a random-mover player built without resign (initialize_replay_buffer is not
    given it), then builds exactly one self-play Player, which gets the triple."""
    from azalea_amd import policy_trainer
    first, players = [], []

    class Stop(Exception):
        pass

    def first_buffer(*a, **kw):
        first.append((a, kw))
        return object()                       # train goes on to build its optimizer and its Player

    def player(*a, **kw):
        players.append(kw)
        raise Stop
    monkeypatch.setattr(policy_trainer, "Player", player)
    monkeypatch.setattr(policy_trainer, "initialize_replay_buffer", first_buffer)
    config = dict(seed=1, device="cpu", game="azalea_amd.game.hex.HexGame", board_size=5, replaybuf_size=64,
                  replaybuf_oversampling=1.0, batch_size=16, lr_initial=0.05, lr_decay=0.1, lr_decay_epochs=1,
                  momentum=0.9, l2_regularization=1e-4, total_epochs=1, selfplay_games=8,
                  resign={"threshold": -0.9, "min_ply": 4, "keep_prob": 0.25})
    with pytest.raises(Stop):
        policy_trainer.train(_cpu_policy(), config, str(tmp_path / "run"))
    assert len(first) == 1 and "resign" not in first[0][1]
    assert not any(isinstance(x, (tuple, dict)) and "resign" in repr(x) for x in first[0][0])
    assert len(players) == 1 and players[0]["resign"] == (-0.9, 4, 0.25), players
    # the same train without the option builds its Player without it
    del players[:]
    with pytest.raises(Stop):
        policy_trainer.train(_cpu_policy(), {k: v for k, v in config.items() if k != "resign"}, str(tmp_path / "run2"))
    assert len(players) == 1 and players[0]["resign"] is None
    # initialize_replay_buffer builds its own random-mover Player: nothing in it knows of resign
    assert "resign" not in inspect.getsource(policy_trainer.initialize_replay_buffer)
