"""Early stop of a search whose move can no longer change (azx_set_early_stop; NOT the reference's behaviour, off by
default), as far as it can be held without a GPU: the C ABI's two entry points (declared, bound), the header's
definition, the Python surface, the refusals of Player and train, which come before any engine is made, and the CPU
reference of the rule (tests/early_stop_reference.py) against one-call oracle searches.  The searches on the device are
tests/test_gpu_early_stop.py's."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import early_stop_reference as ref  # noqa: E402
from option_api_stubs import _Agent, _RandomAgent, _cpu_policy, no_engines  # noqa: E402,F401

NEW_SYMBOLS = ("azx_set_early_stop", "azx_early_stop_stats")


def header():
    return open(os.path.join(ROOT, "include", "azx.h")).read()


def L():
    from azalea_amd import _lib
    return _lib.lib()


def test_the_header_declares_the_two_symbols_and_the_binding_requires_them():
    from azalea_amd import _lib
    text = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    assert L().azx_version() == 7
    # azx_config and azx_play_stats are unchanged: the option is set beside them
    assert len(_lib.Config._fields_) == 18 and len(_lib.PlayStats._fields_) == 20


def test_the_header_states_the_rule_and_that_it_is_not_the_reference():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    sec = text[text.index("Early stop of a search whose move can no longer change"):text.index("int azx_set_early_stop(")]
    assert "NOT the reference's behaviour" in sec and "off by default" in sec
    assert "azx_version stays 7" in sec and "dlsym azx_set_early_stop" in sec
    # the rule, in the issue's words
    assert "ply >= exploration_depth or temperature == 0" in sec
    assert "n1 - n2 > batches_left * search_batch_size" in sec
    assert "all earlier batches are expanded and backed up and their virtual losses undone" in sec
    assert "largest and second-largest num_visits among the root's children" in sec and "n2 = 0 with one child" in sec
    assert "integers held in float32" in sec and "The inequality is strict" in sec
    assert "An unevaluated root (all counts 0) never satisfies the rule" in sec
    assert "Stopping means batches_left = 0" in sec
    assert "Resignation's judgement (azx_set_resign) is then made on the stopped search's root" in sec
    assert "fast plies stop early too" in sec
    assert "divided by the selects the ply made" in sec
    assert "same kernels and returns the same bytes" in sec
    assert "not measured" in sec
    assert "estop=on or estop=off" in sec


def test_the_python_surface():
    from azalea_amd import engine, policy_trainer
    from azalea_amd.parallel_player import Player
    for name in ("set_early_stop", "early_stop_stats"):
        assert callable(getattr(engine.Engine, name)), name
    p = inspect.signature(engine.Engine.set_early_stop).parameters["on"]
    assert p.default is True
    p = inspect.signature(Player.__init__).parameters["early_stop"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    for doc in (engine.Engine.set_early_stop.__doc__, Player.__init__.__doc__, policy_trainer.train.__doc__):
        assert "NOT the reference's behaviour" in doc and "not measured" in doc
    assert 'config["early_stop"]' in policy_trainer.train.__doc__


# ---- Player and train: the refusal comes before anything touches a GPU (the stubs of tests/option_api_stubs.py) -------
def test_player_takes_the_option_for_device_self_play_and_refuses_it_elsewhere(no_engines):
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    assert Player(None, [a]).early_stop is False
    assert Player(None, [a], early_stop=True).early_stop is True
    assert Player(None, [a], early_stop=True).early_stop_stats() is None       # no engine yet
    # agents that play on the host: two agents, a random mover -- refused only when the option is on
    for agents in ([a, b], [_RandomAgent()]):
        assert Player(None, agents, early_stop=False).early_stop is False
        with pytest.raises(ValueError, match="early_stop needs the games to run in a device engine"):
            Player(None, agents, early_stop=True)
    with pytest.raises(ValueError):
        Player(None, [a, b], device_match=True, early_stop=True)
    for bad in (1, 0, "yes", 0.5, (True,)):
        with pytest.raises(ValueError, match="early_stop must be True or False"):
            Player(None, [a], early_stop=bad)


def test_device_match_refuses_the_option_by_name(no_engines, monkeypatch):
    """With the match's own requirements met (stubbed: they need networks on a GPU), the option is what is refused."""
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    monkeypatch.setattr(Player, "_match_policies", lambda self: [a.policy, b.policy])
    assert Player(None, [a, b], device_match=True).early_stop is False
    with pytest.raises(ValueError, match="early_stop is a self-play option"):
        Player(None, [a, b], device_match=True, early_stop=True)


def test_train_refuses_a_bad_value_before_it_builds_anything(no_engines, tmp_path, monkeypatch):
    from azalea_amd import policy_trainer

    def refuse(*a, **kw):
        raise AssertionError("train went on after a bad config['early_stop']")
    monkeypatch.setattr(policy_trainer, "initialize_replay_buffer", refuse)
    monkeypatch.setattr(policy_trainer, "Player", refuse)
    policy = _cpu_policy()
    base = dict(seed=1, device="cpu", game="azalea_amd.game.hex.HexGame", board_size=5)
    for bad in (1, "on", 0.5, {"on": True}):
        with pytest.raises(ValueError, match=r"config\['early_stop'\]: early_stop must be True or False"):
            policy_trainer.train(policy, dict(base, early_stop=bad), str(tmp_path / "run"))
    assert not (tmp_path / "run").exists()


# ---- the CPU reference of the rule ----------------------------------------------------------------------------------
def test_top_two_and_the_rule():
    assert ref.top_two([3, 9, 9, 1]) == (9.0, 9.0, 1)          # a tie: the margin is 0
    assert ref.top_two([7]) == (7.0, 0.0, 0)                   # n2 = 0 with one child
    assert ref.rule_holds([31, 0, 0], 3) and not ref.rule_holds([30, 0, 0], 3)     # strict
    assert not ref.rule_holds([0, 0, 0], 1)                    # an unevaluated root never stops


def dumps_equal(a, b):
    da, db = a.dump(), b.dump()
    assert da["num_nodes"] == db["num_nodes"] and da["root_id"] == db["root_id"]
    for k in ("parent", "first_child", "num_children"):
        assert np.array_equal(da[k], db[k]), k
    for k in ("num_visits", "total_value", "prior_prob"):
        assert np.array_equal(da[k].view(np.uint32), db[k].view(np.uint32)), k


@pytest.mark.parametrize("kind", ["hash", "uniform"])
def test_a_search_run_batch_by_batch_leaves_the_tree_of_one_call(kind):
    """NB calls of simulations = bs - 1 against one call of the whole search, on the empty board and mid-game."""
    from oracle import oracle as orc
    for prefix in ([], [13, 7], [1, 25, 13, 12, 8, 18]):
        b, t, _ = ref.search_batches(prefix, kind, stop=False)
        assert b == ref.NB
        one = orc.Tree(1 << 16)
        st = orc.search(one, ref.game_at(prefix), ref.evaluator(kind), ref.SIMS, ref.BS, ref.C_PUCT)
        assert st.status == 0
        dumps_equal(t, one)


def test_the_reference_positions_meet_their_caps_and_agree_with_the_full_search():
    from oracle import oracle as orc
    refs, dropped = ref.positions("hash")
    stopping = [r for r in refs if r["b_star"] < ref.NB]
    print("positions %d, dropped for a tie %d, stopping early %d, mean batches of those %.2f of %d"
          % (len(refs), dropped, len(stopping), np.mean([r["b_star"] for r in stopping]), ref.NB))
    assert dropped <= ref.MAX_DROPPED_SHARE * (len(refs) + dropped)
    assert len(stopping) >= ref.MIN_STOPPING
    assert any(r["b_star"] == ref.NB for r in refs)            # ... and some never stop
    for r in refs:
        assert 1 <= r["b_star"] <= ref.NB
        # the leader at a stop is the full search's leader: the remaining selects cannot change the move
        assert r["leader"] == r["full_leader"], r["prefix"]
        if r["b_star"] == ref.NB:
            # the rule never fired: the helper's tree is the one-call search's
            one = orc.Tree(1 << 16)
            orc.search(one, ref.game_at(r["prefix"]), ref.evaluator("hash"), ref.SIMS, ref.BS, ref.C_PUCT)
            one.move(r["leader"])
            for x, y in zip(ref.root_after(one), r["stop_root"]):
                assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
        else:
            # a stopped search carries a subtree with no more visits than the full search's
            assert r["stop_root"][2] <= r["full_root"][2], r["prefix"]
    assert any(r["stop_root"][2] < r["full_root"][2] for r in stopping)       # ... and a thinner one somewhere
    assert ref.counts_of(refs)["batches_skipped"] == sum(ref.NB - r["b_star"] for r in stopping) > 0
