"""The plain-f16 tower switch on the wide shapes (128 / 256 channels: policy attribute tower_precision,
config["selfplay_tower"]): the host surface, CPU only.  The device side is tests/test_gpu_wide_f16.py; the 6x64-class
shapes are tests/test_tower_f16_api.py."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _policy(n, blocks, chans, precision="f16"):
    from azalea_amd.policy import Policy
    pol = Policy()
    pol.initialize(dict(device="cpu", network="HexNetwork", board_size=n, num_blocks=blocks, base_chans=chans,
                        simulations=20, search_batch_size=4, exploration_coef=0.5, exploration_depth=4,
                        exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0, seed=1))
    if precision is not None:
        pol.tower_precision = precision
    return pol


def _agent(pol):
    from functools import partial
    from azalea_amd import AzaleaAgent, HexGame
    return AzaleaAgent(partial(HexGame, pol.board_size), policy=pol, device="cpu")


WIDE = [(13, 2, 256), (5, 1, 128)]


@pytest.mark.parametrize("shape", WIDE)
def test_tower_flags_accepts_the_wide_shapes(shape):
    from azalea_amd import engine
    from azalea_amd.policy import tower_flags
    assert tower_flags(_policy(*shape)) == engine.FLAG_TOWER_F16
    assert tower_flags(_policy(*shape, precision=None)) == 0
    assert tower_flags(_policy(*shape, precision="f16x3")) == 0


def test_what_was_refused_stays_refused():
    from azalea_amd.policy import tower_flags
    with pytest.raises(ValueError, match="at least one block"):
        tower_flags(_policy(5, 0, 128))                   # the wide tower without a block: a stem, no convolution
    with pytest.raises(ValueError, match="64 channels") as ei:
        tower_flags(_policy(5, 1, 32))
    assert "121 cells" in str(ei.value) and "at least one block" in str(ei.value) and "128" in str(ei.value)
    with pytest.raises(ValueError, match="121 cells") as ei:
        tower_flags(_policy(13, 1, 64))
    assert "64 channels" in str(ei.value) and "at least one block" in str(ei.value) and "128" in str(ei.value)
    with pytest.raises(ValueError, match="64 channels"):
        tower_flags(_policy(5, 1, 16))
    with pytest.raises(ValueError, match="64 channels"):
        tower_flags(_policy(5, 1, 192))                   # a multiple of 64 that is not one of 128: no wide tower


@pytest.mark.parametrize("shape", WIDE)
def test_player_accepts_a_wide_policy_before_any_engine(shape):
    from azalea_amd import Player
    player = Player(None, [_agent(_policy(*shape))])      # one agent with a HexNetwork: the device engine would play
    assert player._engine is None
    player.stop()
    with pytest.raises(ValueError, match="host loop"):    # two agents without device_match: the host loop
        Player(None, [_agent(_policy(*shape)), _agent(_policy(*shape, precision=None))])


def test_player_and_evaluate_throughput_still_refuse():
    from azalea_amd import Player
    from azalea_amd.evaluation import evaluate_throughput
    with pytest.raises(ValueError, match="at least one block"):
        Player(None, [_agent(_policy(5, 0, 128))])
    with pytest.raises(ValueError, match="at least one block"):
        evaluate_throughput([_agent(_policy(5, 0, 128)), _agent(_policy(5, 0, 128, precision=None))], 2)


def test_training_config_key_reaches_a_wide_policy(tmp_path):
    from azalea_amd import policy_trainer
    pol = _policy(5, 1, 128, precision=None)
    policy_trainer.apply_selfplay_tower(pol, {"selfplay_tower": "f16"})
    assert pol.tower_precision == "f16"
    policy_trainer.apply_selfplay_tower(pol, {"selfplay_tower": None})
    assert pol.tower_precision is None
    # train() reads the key first: it passes the check for a wide policy and stops at the next thing it needs (this
    # config has nothing else), where a refused shape stops at the key itself, before anything is made
    with pytest.raises(KeyError):
        policy_trainer.train(pol, {"selfplay_tower": "f16"}, str(tmp_path / "wide"))
    assert pol.tower_precision == "f16"
    blockless = _policy(5, 0, 128, precision=None)
    with pytest.raises(ValueError, match="at least one block"):
        policy_trainer.train(blockless, {"selfplay_tower": "f16"}, str(tmp_path / "blockless"))
    assert getattr(blockless, "tower_precision", None) is None and not (tmp_path / "blockless").exists()


def test_header_defines_the_wide_arithmetic():
    hdr = open(os.path.join(ROOT, "include", "azx.h")).read()
    flag = hdr[hdr.index("AZX_FLAG_TOWER_F16 = 4"):hdr.index("typedef struct")]
    for word in ("k_conv_wide_f16_s16", "k_stem_wide_f16", "multiple of 128", "residual"):
        assert word in flag, word
