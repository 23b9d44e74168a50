"""What the tests/test_*_api.py files share to hold Player and train to their refusals without a GPU: agents around a
CPU policy, a random mover, and `no_engines`, under which making an engine fails the test -- every refusal has to come
before anything touches a GPU.  A plain module (imported like early_stop_reference), not a conftest."""
import pytest

SEARCH = dict(simulations=10, search_batch_size=2, exploration_coef=0.5, exploration_depth=3,
              exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0)


class _Agent:
    def __init__(self, policy, n=5):
        from azalea_amd.game.hex import HexGame
        self.policy = policy
        self.game = HexGame(n)


class _RandomAgent:
    def __init__(self, n=5):
        from azalea_amd.game.hex import HexGame
        self.game = HexGame(n)


def _cpu_policy():
    from azalea_amd.policy import Policy
    p = Policy()
    p.initialize(dict(device="cpu", network="HexNetwork", board_size=5, num_blocks=1, base_chans=32, **SEARCH))
    return p


@pytest.fixture
def no_engines(monkeypatch):
    from azalea_amd import engine

    def refuse(*a, **kw):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(engine, "Engine", refuse)
    monkeypatch.setattr(engine, "Match", refuse)
