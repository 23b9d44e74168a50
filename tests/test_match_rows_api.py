"""Replay rows from device matches, as far as they can be held without a GPU: the C ABI's new entry points (declared,
bound, argument checks that come before any device work) and the argument checks of the two-agent device Player.
The rows themselves are tests/test_gpu_match_rows.py's."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from option_api_stubs import _Agent, _cpu_policy, no_engines  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("azx_match_set_harvest", "azx_match_set_first_mover", "azx_match_rows", "azx_tournament_set_harvest",
               "azx_tournament_set_first_mover", "azx_tournament_rows", "azx_rows_read")
EINVAL = -1


def header():
    return open(os.path.join(ROOT, "include", "azx.h")).read()


def test_the_header_declares_every_new_symbol_and_the_binding_binds_it():
    from azalea_amd import _lib
    text = header()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    assert EINVAL == int(re.search(r"AZX_EINVAL\s*=\s*(-?\d+)", text).group(1))
    # the play calls keep their signatures: the additions are setters beside them
    assert len(_lib.SYMBOLS["azx_match_play"][1]) == 7 and len(_lib.SYMBOLS["azx_tournament_play"][1]) == 11


def test_abi_revision_is_still_7():
    from azalea_amd import _lib
    assert _lib.lib().azx_version() == 7


def test_null_handles_are_einval():
    from azalea_amd import _lib
    L = _lib.lib()
    rows = C.c_int64(-5)
    assert L.azx_match_set_harvest(None, 1) == EINVAL
    assert b"null" in L.azx_last_error()
    assert L.azx_match_set_first_mover(None, 0) == EINVAL
    assert L.azx_match_rows(None, C.byref(rows)) == EINVAL
    assert L.azx_tournament_set_harvest(None, 0) == EINVAL
    assert L.azx_tournament_set_first_mover(None, -1) == EINVAL
    assert L.azx_tournament_rows(None, C.byref(rows)) == EINVAL
    assert L.azx_rows_read(None, 0, 0, None, None, None, None, None, None) == EINVAL
    assert rows.value == -5


def test_a_bad_first_mover_mode_is_einval_and_the_message_names_it():
    """(checked before the handle, so that it can be held here; a live handle: tests/test_gpu_match_rows.py)"""
    from azalea_amd import _lib
    L = _lib.lib()
    for fn in (L.azx_match_set_first_mover, L.azx_tournament_set_first_mover):
        for mode in (-2, 2, 7):
            assert fn(None, mode) == EINVAL
            assert ("first mover mode %d" % mode).encode() in L.azx_last_error()
        for mode in (-1, 0, 1):
            assert fn(None, mode) == EINVAL and b"null" in L.azx_last_error()


def test_the_header_says_what_a_match_does_to_the_queues_and_in_what_order_rows_come():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    sec = text[text.index("replay rows from matches"):text.index("int azx_match_rows(")]
    assert "azx_version stays 7" in sec and "dlsym azx_match_set_harvest" in sec
    assert re.search(r"EVERY match and tournament call, harvesting or not[^.]*empties them", sec)
    assert re.search(r"Row order: games in the order their settling steps reserved", sec)
    assert "plies ascending" in sec and "1012 bytes" in sec and "AZX_ENOMEM" in sec and "AZX_ESTATE" in sec
    assert "voided game leaves no rows" in sec


# ---- the two-agent device Player: every refusal comes before anything touches a GPU -----------------------------
def test_device_match_is_a_keyword_of_player_and_off_by_default():
    from azalea_amd.parallel_player import Player
    p = inspect.signature(Player.__init__).parameters["device_match"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_device_match_needs_exactly_two_agents(no_engines):
    from azalea_amd.parallel_player import Player
    one = _Agent(_cpu_policy())
    for agents in ([one], [one, one, one]):
        with pytest.raises(ValueError, match="exactly two agents, got %d" % len(agents)):
            Player(None, agents, device_match=True)


def test_device_match_refuses_a_random_mover_and_an_agent_without_a_policy(no_engines):
    from azalea_amd.parallel_player import Player
    from azalea_amd.random_policy import RandomPolicy
    good = _Agent(_cpu_policy())
    for bad in (_Agent(RandomPolicy()), _Agent(None)):
        for agents in ([good, bad], [bad, good]):
            with pytest.raises(ValueError, match=r"agent %d.*Policy" % agents.index(bad)):
                Player(None, agents, device_match=True)


def test_device_match_refuses_a_network_on_the_cpu_and_names_the_device(no_engines):
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    with pytest.raises(ValueError, match=r"CUDA \(ROCm\) device.*\bcpu\b"):
        Player(None, [a, b], device_match=True)
    # without the switch the same two agents are the host loop's, as before
    p = Player(None, [a, b])
    assert p.device_match is False and p._device_policy() is None


def test_collect_is_a_keyword_of_the_python_surface():
    from azalea_amd import engine, evaluation
    for fn, names in ((engine.Match.play, ("collect", "first_mover")),
                      (engine.Tournament.play, ("collect", "sink", "first_mover"))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert name in params, (fn, name)
    assert inspect.signature(engine.Match.play).parameters["collect"].default is False
    assert inspect.signature(engine.Tournament.play).parameters["sink"].default == 0
    p = inspect.signature(evaluation.evaluate_throughput).parameters["collect"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert callable(engine.Engine.rows_read)
