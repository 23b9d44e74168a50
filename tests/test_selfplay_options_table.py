"""The table of the self-play options (azalea_amd/selfplay_options.py) against the layers that read it:
every entry has its Player keyword, its Engine methods and its paragraph in train's docstring; Player refuses every
option by name under device_match and where the host loop plays, before any engine is made; a new engine gets the
options in the table's order; and the one exclusion the table states is raised by Player and by train alike."""
import inspect
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from option_api_stubs import _Agent, _RandomAgent, _cpu_policy, no_engines  # noqa: E402,F401

from azalea_amd import engine, parallel_player, policy_trainer, selfplay_options  # noqa: E402
from azalea_amd.parallel_player import Player  # noqa: E402
from azalea_amd.selfplay_options import BY_NAME, OPTIONS  # noqa: E402

ORDER = ("selfplay_openings", "playout_cap", "resign", "early_stop", "train_targets", "forced_playouts", "gumbel")

# one value per option that is "on", as Player takes it, and what the Engine setter is then called with
ON = dict(selfplay_openings=[[13], [7, 19]], playout_cap=(0.5, 4), resign=(-0.9, 4, 0.25), early_stop=True,
          train_targets="visits", forced_playouts=True, gumbel=8)
SET_WITH = dict(selfplay_openings=([[13], [7, 19]], None), playout_cap=(0.5, 4), resign=(-0.9, 4, 0.25),
                early_stop=(True,), train_targets=("visits", 0.0), forced_playouts=(2.0, True),
                gumbel=(8, 50.0, 1.0, True))


def test_the_table_is_a_plain_tuple_in_the_application_order():
    assert isinstance(OPTIONS, tuple) and tuple(o.name for o in OPTIONS) == ORDER
    assert BY_NAME == {o.name: o for o in OPTIONS}
    assert type(OPTIONS[0]).__mro__ == (selfplay_options.Option, object)           # no metaclass, no base machinery
    assert type(selfplay_options.Option) is type


@pytest.mark.parametrize("name", ORDER)
def test_every_entry_names_what_the_layers_have(name):
    opt = BY_NAME[name]
    params = inspect.signature(Player.__init__).parameters
    for keyword in opt.keywords:
        assert params[keyword].kind is inspect.Parameter.KEYWORD_ONLY, keyword
        assert "`%s`" % keyword in Player.__init__.__doc__, keyword
    assert opt.keywords[0] == name
    assert callable(getattr(engine.Engine, opt.setter)) and opt.setter.startswith("set_")
    assert callable(getattr(engine.Engine, opt.stats)) and opt.stats.endswith("_stats")
    assert 'config["%s"]' % name in policy_trainer.train.__doc__
    assert callable(opt.normalize) and getattr(parallel_player, opt.normalize.__name__) is opt.normalize
    assert opt.match_reason and opt.host_reason and opt.title and callable(opt.log)
    assert all(other in BY_NAME for other in opt.excludes)


def test_parallel_player_re_exports_the_normalisers_and_defines_none():
    source = inspect.getsource(parallel_player)
    assert "def normalize_" not in source
    for fn in ("normalize_playout_cap", "normalize_resign", "normalize_early_stop", "normalize_train_targets",
               "normalize_forced_playouts", "normalize_gumbel", "normalize_selfplay_openings"):
        assert getattr(parallel_player, fn) is getattr(selfplay_options, fn)
    assert parallel_player.GUMBEL_DEFAULT is selfplay_options.GUMBEL_DEFAULT == (16, 50.0, 1.0, True)


@pytest.mark.parametrize("name", ORDER)
def test_player_refuses_every_option_by_name_where_no_self_play_engine_runs(name, no_engines, monkeypatch):
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    for agents in ([a, b], [_RandomAgent()]):
        if name == "selfplay_openings" and len(agents) == 2:
            word = "selfplay_openings is a self-play option: it needs a single agent, got 2"
        else:
            word = "%s needs the games to run in a device engine" % name
        with pytest.raises(ValueError, match=word) as err:
            Player(None, agents, **{name: ON[name]})
        assert BY_NAME[name].host_reason in str(err.value) or len(agents) == 2 and name == "selfplay_openings"
    # with the match's own requirements met (stubbed: they need networks on a GPU), the option is what is refused
    monkeypatch.setattr(Player, "_match_policies", lambda self: [a.policy, b.policy])
    with pytest.raises(ValueError) as err:
        Player(None, [a, b], device_match=True, gather=False, **{name: ON[name]})
    assert str(err.value) == "%s is a self-play option: %s" % (name, BY_NAME[name].match_reason)
    # ... and off, every option is taken everywhere
    assert getattr(Player(None, [a, b]), name) == BY_NAME[name].off
    assert getattr(Player(None, [_RandomAgent()], **{name: BY_NAME[name].off}), name) == BY_NAME[name].off


class _RecordingEngine:
    """Stands in for engine.Engine: remembers every set_* call, in order."""
    calls = []

    def __init__(self, **kw):
        type(self).calls.append(("create", None))

    def __getattr__(self, attr):
        if not attr.startswith("set_"):
            raise AttributeError(attr)
        return lambda *args: type(self).calls.append((attr, args))


def test_a_new_engine_gets_the_options_in_the_tables_order(monkeypatch):
    a = _Agent(_cpu_policy())
    monkeypatch.setattr(_RecordingEngine, "calls", [])
    monkeypatch.setattr(engine, "Engine", _RecordingEngine)
    monkeypatch.setattr(Player, "_device_policy", lambda self: a.policy)
    compatible = [n for n in ORDER if n != "gumbel"]
    for names in (compatible, ["selfplay_openings", "playout_cap", "resign", "train_targets", "gumbel"], []):
        del _RecordingEngine.calls[:]
        p = Player(None, [a], n_games=4, **{n: ON[n] for n in names})
        p._seed_base = 1
        p._get_engine(a.policy)
        assert _RecordingEngine.calls == [("create", None)] + [(BY_NAME[n].setter, SET_WITH[n]) for n in ORDER if n in names]
        p._get_engine(a.policy)                                     # the same key: the engine stays, nothing is set again
        assert len(_RecordingEngine.calls) == 1 + len(names)


def test_gumbel_excludes_forced_playouts_and_early_stop_in_player_and_in_train(no_engines, tmp_path, monkeypatch):
    assert BY_NAME["gumbel"].excludes == ("forced_playouts", "early_stop")
    assert [o.name for o in OPTIONS if o.excludes] == ["gumbel"]
    a = _Agent(_cpu_policy())
    why = "that option is a rule about PUCT visit leaders, which a Gumbel root search does not play"
    for others, named in ((dict(forced_playouts=True), "forced_playouts"), (dict(early_stop=True), "early_stop"),
                          (dict(forced_playouts=True, early_stop=True), "forced_playouts")):
        with pytest.raises(ValueError) as err:
            Player(None, [a], gumbel=8, **others)
        assert str(err.value) == "gumbel cannot be set together with %s: %s" % (named, why)

        def refuse(*args, **kw):
            raise AssertionError("train went on after an excluded pair of options")
        monkeypatch.setattr(policy_trainer, "initialize_replay_buffer", refuse)
        monkeypatch.setattr(policy_trainer, "Player", refuse)
        config = dict(seed=1, device="cpu", game="azalea_amd.game.hex.HexGame", board_size=5, gumbel=8, **others)
        with pytest.raises(ValueError) as err:
            policy_trainer.train(_cpu_policy(), config, str(tmp_path / "run"))
        assert str(err.value) == ("config['gumbel']: gumbel cannot be set together with config['%s']: %s" % (named, why))
    assert not (tmp_path / "run").exists()
    # each alone is taken
    assert Player(None, [a], gumbel=8).gumbel == (8, 50.0, 1.0, True)
    assert Player(None, [a], forced_playouts=True, early_stop=True).gumbel is None


def test_from_config_gives_train_the_player_keywords_and_one_log_line_per_option():
    policy = _cpu_policy()
    keywords, lines = selfplay_options.from_config({"board_size": 5}, policy)
    assert keywords == dict(selfplay_openings=None, selfplay_opening_weights=None, playout_cap=None, resign=None,
                            early_stop=False, train_targets=None, forced_playouts=None, gumbel=None)
    assert len(lines) == len(OPTIONS) and all(line.endswith(": off") for line in lines)
    config = dict(board_size=5, selfplay_openings={"book": [[13], [7]], "weights": [3, 1]}, playout_cap=(0.25, 4),
                  resign=(-0.9, 4, 0.25), train_targets="visits", gumbel=8)
    keywords, lines = selfplay_options.from_config(config, policy)
    assert keywords == dict(selfplay_openings=[[13], [7]], selfplay_opening_weights=[3.0, 1.0], playout_cap=(0.25, 4),
                            resign=(-0.9, 4, 0.25), early_stop=False, train_targets=("visits", 0.0),
                            forced_playouts=None, gumbel=(8, 50.0, 1.0, True))
    assert set(keywords) <= set(inspect.signature(Player.__init__).parameters)
    on = [line for line in lines if "on -- NOT the reference's behaviour: " in line]
    assert len(on) == 5 and all("(config['" in line for line in lines)
    # the two options whose messages carry no config[...] prefix keep theirs, the others name the key
    with pytest.raises(ValueError, match=r"^resign: threshold"):
        selfplay_options.from_config(dict(resign=(-2.0, 4, 0.1)), policy)
    with pytest.raises(ValueError, match=r"^playout_cap: full_prob"):
        selfplay_options.from_config(dict(playout_cap=(0.0, 4)), policy)
    with pytest.raises(ValueError, match=r"^config\['playout_cap'\]: fast_simulations 11 above simulations 10"):
        selfplay_options.from_config(dict(playout_cap=(0.5, 11)), policy)
    with pytest.raises(ValueError, match=r"^config\['early_stop'\]: early_stop must be True or False"):
        selfplay_options.from_config(dict(early_stop=1), policy)
