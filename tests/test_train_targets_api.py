"""Training targets of the recorded self-play rows (azx_set_train_targets: visit-share policy rows, z/q-blended rewards;
NOT the reference's behaviour, off by default), as far as they can be held without a GPU: the C ABI's three entry
points (declared, bound), the header's definition, the Python surface, the refusals of Player and train, which come
before any engine is made, and the numpy twins (tests/train_targets_reference.py) on hand-made cases.  The rows on the
device are tests/test_gpu_train_targets.py's."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_targets_reference as ref  # noqa: E402
from option_api_stubs import _Agent, _RandomAgent, _cpu_policy, no_engines  # noqa: E402,F401

NEW_SYMBOLS = ("azx_set_train_targets", "azx_get_train_targets", "azx_train_targets_stats")


def header():
    return open(os.path.join(ROOT, "include", "azx.h")).read()


def L():
    from azalea_amd import _lib
    return _lib.lib()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_header_declares_the_three_symbols_and_the_binding_requires_them():
    from azalea_amd import _lib
    text = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    assert re.search(r"^#define AZX_ROWS_REFERENCE 0\b", text, re.M) and re.search(r"^#define AZX_ROWS_VISITS +1\b", text, re.M)
    assert _lib.SYMBOLS["azx_set_train_targets"][1][1:] == [C.c_int, C.c_float]
    assert L().azx_version() == 7
    # azx_config and azx_play_stats are unchanged: the option is set beside them
    assert len(_lib.Config._fields_) == 18 and len(_lib.PlayStats._fields_) == 20


def test_the_header_carries_the_definition_and_that_it_is_not_the_reference():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    sec = text[text.index("Training targets of the rows throughput self-play records"):text.index("#define AZX_ROWS_REFERENCE")]
    assert "NOT the reference's behaviour" in sec and "off by default" in sec and "outside every parity claim" in sec
    assert "azx_version stays 7" in sec and "dlsym azx_set_train_targets" in sec
    # the move draw
    assert "The move draw is untouched" in sec
    assert "Row metric 2 stays the log-probability of the drawn move under the draw's distribution" in sec
    assert "move for move the game the same seed plays with the option off" in sec
    # the rows
    assert "row[j] = nv_j / nv_sum" in sec and "integers held in float32" in sec and "which is exact" in sec
    assert "ONE float32 IEEE division" in sec
    assert "rows of T = 1 plies are bit for bit what they were" in sec
    assert "A root with nv_sum == 0 cannot occur at a recorded ply; if it does, the reference row is written" in sec
    # the blend
    assert "reward = (1 - lambda) * z + lambda * v" in sec
    assert "two float32 products and one sum, unfused" in sec
    assert "If v is not finite the reward is z" in sec and "lambda = 0 stores z itself, with no arithmetic" in sec
    assert "sum_reward_last keeps summing z" in sec
    assert "Row metric 7 carries v whenever resignation or either part of this option is set, and 0 otherwise" in sec
    # beside the other options
    assert "A fast ply of a playout cap still records nothing" in sec
    assert "the rows of a resigned game blend the conceded z" in sec
    assert "visit shares AT THE STOP" in sec
    assert "holds for the reference's one-hot row only" in sec
    # scope, arguments, off
    assert "refuse an engine with the option set with AZX_EINVAL before touching any engine" in sec
    assert "NaN, a value outside [0, 1] or an unknown policy_rows is AZX_EINVAL and leaves the setting in place" in sec
    assert '(AZX_ROWS_REFERENCE, 0.0f) is "off"' in sec
    assert "The call zeroes the statistics" in sec
    assert "same kernels and returns the same bytes" in sec and "metric 7 = 0" in sec
    # the early-stop section is as it was
    assert "those selects can change neither the move nor the row" in text


def test_the_python_surface():
    from azalea_amd import engine, policy_trainer
    from azalea_amd.parallel_player import Player
    for name in ("set_train_targets", "clear_train_targets", "train_targets", "train_targets_stats"):
        assert callable(getattr(engine.Engine, name)), name
    sig = inspect.signature(engine.Engine.set_train_targets).parameters
    assert sig["policy_rows"].default == "reference" and sig["value_mix"].default == 0.0
    p = inspect.signature(Player.__init__).parameters["train_targets"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert callable(Player.train_targets_stats)
    for doc in (engine.Engine.set_train_targets.__doc__, Player.__init__.__doc__, policy_trainer.train.__doc__):
        assert "NOT the reference's behaviour" in doc and "DESIGN 7.12" in doc
    assert 'config["train_targets"]' in policy_trainer.train.__doc__


def test_normalize_train_targets():
    from azalea_amd.parallel_player import normalize_train_targets as norm
    assert norm(None) is None and norm(False) is None
    assert norm("visits") == ("visits", 0.0)
    assert norm(("visits", 0.5)) == ("visits", 0.5) and norm(["reference", 1]) == ("reference", 1.0)
    assert norm({"policy_rows": "visits", "value_mix": 0.25}) == ("visits", 0.25)
    assert norm(("visits", np.float32(0.5))) == ("visits", 0.5)
    assert norm(("reference", 0.0)) is None                    # the pair that is "off"
    for bad in (True, 1, 0.5, "reference", "on", ("visits",), ("visits", 0.5, 1), ("shares", 0.5), ("visits", 1.5),
                ("visits", -0.1), ("visits", float("nan")), ("visits", "0.5"), ("visits", None), ("visits", True),
                {"policy_rows": "visits"}, {"policy_rows": "visits", "value_mix": 0.5, "x": 1}, {"rows": "visits", "mix": 0},
                {"policy_rows": "visits", "value_mix": 2}):
        with pytest.raises(ValueError, match="train_targets"):
            norm(bad)


# ---- Player and train: the refusal comes before anything touches a GPU (the stubs of tests/option_api_stubs.py) --------
def test_player_takes_the_option_for_device_self_play_and_refuses_it_elsewhere(no_engines):
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    assert Player(None, [a]).train_targets is None
    assert Player(None, [a], train_targets="visits").train_targets == ("visits", 0.0)
    assert Player(None, [a], train_targets=("visits", 0.5)).train_targets == ("visits", 0.5)
    assert Player(None, [a], train_targets=("reference", 0.0)).train_targets is None
    assert Player(None, [a], train_targets="visits").train_targets_stats() is None       # no engine yet
    # agents that play on the host: two agents, a random mover -- refused only when the option is on
    for agents in ([a, b], [_RandomAgent()]):
        assert Player(None, agents, train_targets=None).train_targets is None
        assert Player(None, agents, train_targets=False).train_targets is None
        with pytest.raises(ValueError, match="train_targets needs the games to run in a device engine"):
            Player(None, agents, train_targets="visits")
    with pytest.raises(ValueError):
        Player(None, [a, b], device_match=True, train_targets=("reference", 0.5))
    for bad in (1, "yes", ("visits", 2.0), {"policy_rows": "visits"}):
        with pytest.raises(ValueError, match="train_targets"):
            Player(None, [a], train_targets=bad)


def test_device_match_refuses_the_option_by_name(no_engines, monkeypatch):
    """With the match's own requirements met (stubbed: they need networks on a GPU), the option is what is refused."""
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    monkeypatch.setattr(Player, "_match_policies", lambda self: [a.policy, b.policy])
    assert Player(None, [a, b], device_match=True).train_targets is None
    with pytest.raises(ValueError, match="train_targets is a self-play option"):
        Player(None, [a, b], device_match=True, train_targets="visits")


def test_train_refuses_a_bad_value_before_it_builds_anything(no_engines, tmp_path, monkeypatch):
    from azalea_amd import policy_trainer

    def refuse(*a, **kw):
        raise AssertionError("train went on after a bad config['train_targets']")
    monkeypatch.setattr(policy_trainer, "initialize_replay_buffer", refuse)
    monkeypatch.setattr(policy_trainer, "Player", refuse)
    policy = _cpu_policy()
    base = dict(seed=1, device="cpu", game="azalea_amd.game.hex.HexGame", board_size=5)
    for bad in (1, "on", 0.5, ("visits", 1.5), {"on": True}):
        with pytest.raises(ValueError, match=r"config\['train_targets'\]: train_targets"):
            policy_trainer.train(policy, dict(base, train_targets=bad), str(tmp_path / "run"))
    assert not (tmp_path / "run").exists()


class _FakeEngine:
    def __init__(self, targets):
        self.targets = targets

    def train_targets(self):
        return self.targets


def test_match_and_tournament_refuse_an_engine_with_the_option_set():
    from azalea_amd import engine
    off, on = _FakeEngine(("reference", 0.0)), _FakeEngine(("visits", 0.5))
    engine._refuse_train_targets((off, off), "match")
    with pytest.raises(ValueError, match="engine 1 has training targets"):
        engine._refuse_train_targets((off, on), "match")
    with pytest.raises(ValueError, match="engine 0 has training targets"):
        engine._refuse_train_targets((on, off, off), "tournament")
    for cls in (engine.Match, engine.Tournament):
        assert "_refuse_train_targets(" in inspect.getsource(cls.play)


# ---- the numpy twins ------------------------------------------------------------------------------------------------
def test_visit_rows_on_hand_made_cases():
    r = ref.visit_rows([3, 0, 1, 0])
    assert r.dtype == np.float32 and np.array_equal(bits(r), bits([0.75, 0.0, 0.25, 0.0]))
    assert np.array_equal(bits(ref.visit_rows([7])), bits([1.0]))                      # one child
    tie = ref.visit_rows([5, 5, 0, 5])                                                 # a tie: equal shares, one division each
    third = np.float32(5) / np.float32(15)
    assert np.array_equal(bits(tie), bits([third, third, 0.0, third]))
    odd = ref.visit_rows([1, 2, 38])
    assert np.array_equal(bits(odd), bits([np.float32(1) / np.float32(41), np.float32(2) / np.float32(41),
                                           np.float32(38) / np.float32(41)]))
    two = ref.visit_rows([[1, 1], [0, 0]])                                             # rows at once; an all-zero row stays 0
    assert np.array_equal(two, np.array([[0.5, 0.5], [0.0, 0.0]], np.float32))
    n, S = ref.recover_counts(odd, 3, np.float32(41) / np.float32(3))
    assert S == 41 and n.tolist() == [1, 2, 38]


def test_blend_on_hand_made_cases():
    z = np.array([1.0, -1.0, 1.0, -1.0], np.float32)
    v = np.array([0.5, 0.25, -0.75, np.nan], np.float32)
    assert ref.blend(z, v, 0.0).dtype == np.float32
    assert np.array_equal(bits(ref.blend(z, v, 0.0)), bits(z))                         # lambda = 0: z itself
    assert np.array_equal(bits(ref.blend(z, v, 1.0)), bits([0.5, 0.25, -0.75, -1.0]))  # lambda = 1: v; z where v is NaN
    assert np.array_equal(bits(ref.blend(z, v, 0.5)), bits([0.75, -0.375, 0.125, -1.0]))
    inf = ref.blend([1.0, -1.0], [np.inf, -np.inf], 0.5)
    assert np.array_equal(bits(inf), bits([1.0, -1.0]))                                # not finite: z
    # two products and a sum, each rounded to float32
    lam, zz, vv = np.float32(0.3), np.float32(-1.0), np.float32(0.123456789)
    want = np.float32(np.float32((np.float32(1.0) - lam) * zz) + np.float32(lam * vv))
    assert bits(ref.blend([zz], [vv], 0.3))[0] == bits([want])[0]
