"""The plain-f16 tower switch (AZX_FLAG_TOWER_F16, policy attribute tower_precision, config["selfplay_tower"]): the
host surface, CPU only.  The device side is tests/test_gpu_tower_f16.py."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _policy(n=5, blocks=1, chans=64, precision="f16"):
    from azalea_amd.policy import Policy
    pol = Policy()
    pol.initialize(dict(device="cpu", network="HexNetwork", board_size=n, num_blocks=blocks, base_chans=chans,
                        simulations=20, search_batch_size=4, exploration_coef=0.5, exploration_depth=4,
                        exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0, seed=1))
    if precision is not None:
        pol.tower_precision = precision
    return pol


def _agent(pol, n=None):
    from functools import partial
    from azalea_amd import AzaleaAgent, HexGame
    return AzaleaAgent(partial(HexGame, n or pol.board_size), policy=pol, device="cpu")


def test_header_and_bindings():
    from azalea_amd import _lib, engine
    hdr = open(os.path.join(ROOT, "include", "azx.h")).read()
    m = re.search(r"\bAZX_FLAG_TOWER_F16\s*=\s*(\d+)\b", hdr)
    assert m and int(m.group(1)) == 4
    assert _lib.FLAG_TOWER_F16 == 4 and engine.FLAG_TOWER_F16 == 4
    assert _lib.FLAG_TOWER_F16 & (_lib.FLAG_NO_COMPACT | _lib.FLAG_RANDOM_REFLECT) == 0
    assert _lib.lib().azx_version() == 7              # an addition within the revision: the struct did not change


def test_tower_flags_of_a_policy():
    from azalea_amd import engine
    from azalea_amd.policy import tower_flags
    assert tower_flags(_policy(precision=None)) == 0
    assert tower_flags(_policy(precision="f16x3")) == 0
    assert tower_flags(_policy(precision="f16")) == engine.FLAG_TOWER_F16
    assert tower_flags(_policy(11, 6, 64)) == engine.FLAG_TOWER_F16
    for bad in ("fp16", "bf16", "", 16):
        with pytest.raises(ValueError, match="tower_precision"):
            tower_flags(_policy(precision=bad))
    with pytest.raises(ValueError, match="64 channels"):
        tower_flags(_policy(5, 1, 32))
    with pytest.raises(ValueError, match="121 cells"):
        tower_flags(_policy(13, 1, 64))
    with pytest.raises(ValueError, match="at least one block"):
        tower_flags(_policy(5, 0, 64))


def test_player_refuses_what_it_cannot_honour():
    """Before any engine is made, without a GPU."""
    from azalea_amd import Player
    good = _policy()
    player = Player(None, [_agent(good)])              # one agent with a HexNetwork: the device engine would play
    assert player._engine is None
    player.stop()
    with pytest.raises(ValueError, match="host loop"):               # two agents without device_match: the host loop
        Player(None, [_agent(_policy()), _agent(_policy(precision=None))])
    with pytest.raises(ValueError, match="64 channels"):
        Player(None, [_agent(_policy(5, 1, 32))])
    with pytest.raises(ValueError, match="121 cells"):
        Player(None, [_agent(_policy(13, 1, 64))])
    with pytest.raises(ValueError, match="tower_precision"):
        Player(None, [_agent(_policy(precision="half"))])
    # today's spellings change nothing
    for prec in (None, "f16x3"):
        player = Player(None, [_agent(_policy(5, 1, 32, precision=prec))])
        player.stop()


def test_evaluate_throughput_refuses_before_any_engine():
    from azalea_amd.evaluation import evaluate_throughput
    with pytest.raises(ValueError, match="64 channels"):
        evaluate_throughput([_agent(_policy(5, 1, 32)), _agent(_policy(5, 1, 32, precision=None))], 2)
    with pytest.raises(ValueError, match="tower_precision"):
        evaluate_throughput([_agent(_policy(precision="f8")), _agent(_policy())], 2)


def test_training_config_key_reaches_the_policy(tmp_path):
    from azalea_amd import policy_trainer
    pol = _policy(precision=None)
    policy_trainer.apply_selfplay_tower(pol, {})
    assert getattr(pol, "tower_precision", None) is None            # absent: today
    policy_trainer.apply_selfplay_tower(pol, {"selfplay_tower": "f16"})
    assert pol.tower_precision == "f16"
    policy_trainer.apply_selfplay_tower(pol, {"selfplay_tower": None})
    assert pol.tower_precision is None
    with pytest.raises(ValueError, match="tower_precision"):
        policy_trainer.apply_selfplay_tower(pol, {"selfplay_tower": "int8"})
    assert pol.tower_precision is None                               # a refused value is not left behind
    # train() itself reads the key first: a value the network cannot honour stops it before anything is made
    narrow = _policy(5, 1, 32, precision=None)
    with pytest.raises(ValueError, match="64 channels"):
        policy_trainer.train(narrow, {"selfplay_tower": "f16"}, str(tmp_path / "run"))
    assert getattr(narrow, "tower_precision", None) is None and not (tmp_path / "run").exists()
    assert "selfplay_tower" in policy_trainer.train.__doc__ and "parity" in policy_trainer.train.__doc__


def test_parity_mode_policy_does_not_read_the_attribute():
    """Policy's own engine (parity mode) keys on nothing of the sort: the attribute is for throughput mode only."""
    import inspect
    from azalea_amd.policy import Policy
    assert "tower" not in inspect.getsource(Policy._get_engine)
