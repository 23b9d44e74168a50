"""Random 180-degree reflection of network inputs (AZX_FLAG_RANDOM_REFLECT, azx_replay_set_reflect,
prep.rot180_batch, Player(random_reflect=...)): the host surface, CPU only.  The device side is
tests/test_gpu_reflect.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_bindings():
    from azalea_amd import _lib, engine
    hdr = open(os.path.join(ROOT, "include", "azx.h")).read()
    assert re.search(r"\bAZX_FLAG_RANDOM_REFLECT\s*=\s*2\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+azx_replay_set_reflect\s*\(\s*azx_engine\s*\*\s*e\s*,\s*int\s+on\s*,\s*uint64_t\s+seed\s*\)\s*;",
                     code)
    assert _lib.FLAG_RANDOM_REFLECT == 2 and engine.FLAG_RANDOM_REFLECT == 2
    assert _lib.FLAG_RANDOM_REFLECT & _lib.FLAG_NO_COMPACT == 0
    res, args = _lib.SYMBOLS["azx_replay_set_reflect"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_uint64]
    L = _lib.lib()
    assert L.azx_version() == 7                       # an addition within the revision: the struct did not change
    assert L.azx_replay_set_reflect(None, 1, 5) == -1  # AZX_EINVAL
    assert b"null" in L.azx_last_error()


def _random_game(n, rng):
    """One random host game: its moves, and per ply the state before the move with a random target distribution."""
    from azalea_amd.game.hex import HexGame
    g = HexGame(n)
    moves, rows = [], []
    while g.state.result == 0:
        st = g.state
        p = rng.dirichlet(np.ones(len(st.legal_moves))).astype(np.float32)
        rows.append((st, p))
        m = int(rng.choice(st.legal_moves))
        moves.append(m)
        g.step(m)
    return moves, rows, g.state.result


def _replay(n, moves):
    from azalea_amd.game.hex import HexGame
    g = HexGame(n)
    states = []
    for m in moves:
        assert g.state.result == 0 and m in g.state.legal_moves
        states.append(g.state)
        g.step(m)
    return states, g.state.result


def _batch(states, probs, rewards):
    from azalea_amd.prep import torch_batch_replays
    from azalea_amd.replay_buffer import ReplayDataFrame
    frame = ReplayDataFrame(list(states), list(probs), list(rewards))
    return torch_batch_replays([frame[i] for i in range(len(frame))])


@pytest.mark.parametrize("n", [3, 5, 11])
def test_rot180_batch_against_the_host_rules(n):
    """Turning a game by 180 degrees (every move m -> cells + 1 - m, i.e. tile c -> cells - 1 - c) is a symmetry
    of Hex that keeps both players' directions: same result, same length, and the turned game's rows are
    rot180_batch of the original rows."""
    from azalea_amd.prep import rot180_batch
    cells = n * n
    rng = np.random.RandomState(100 + n)
    for _ in range(4):
        moves, rows, result = _random_game(n, rng)
        turned_states, turned_result = _replay(n, [cells + 1 - m for m in moves])
        assert turned_result == result and len(turned_states) == len(rows)
        rewards = [np.float32(1 - 2 * ((len(rows) - 1 - i) & 1)) for i in range(len(rows))]
        orig = _batch([s for s, _ in rows], [p for _, p in rows], rewards)
        # the turned game's targets: the same probability on the same (turned) move; its ascending list is the
        # original list reversed
        want = _batch(turned_states, [p[::-1].copy() for _, p in rows], rewards)
        ones = torch.ones(len(rows), dtype=torch.bool)
        got = rot180_batch(orig, ones)
        assert set(got) == set(orig)
        assert torch.equal(got["board"], want["board"])
        assert got["board"].dtype == orig["board"].dtype and got["legal_moves"].dtype == orig["legal_moves"].dtype
        for key in ("color", "result", "reward"):
            assert torch.equal(got[key], orig[key]) and torch.equal(got[key], want[key]), key
        assert torch.equal(got["moves_prob"], orig["moves_prob"])           # aligned by list position, untouched
        for i in range(len(rows)):
            a = sorted(zip(got["legal_moves"][i].tolist(), got["moves_prob"][i].tolist()))
            b = sorted(zip(want["legal_moves"][i].tolist(), want["moves_prob"][i].tolist()))
            assert a == b, i
            k = len(rows[i][0].legal_moves)
            assert (got["legal_moves"][i, k:] == 0).all() and (got["legal_moves"][i, :k] > 0).all()
        # mask = 0: every tensor bit-equal; a mixed mask: row by row; twice = identity
        none = rot180_batch(orig, torch.zeros(len(rows), dtype=torch.bool))
        for key in orig:
            assert torch.equal(none[key], orig[key]), key
        mask = torch.from_numpy(rng.randint(0, 2, len(rows)).astype(np.int64))
        mixed = rot180_batch(orig, mask)
        for i in range(len(rows)):
            src = got if mask[i] else orig
            assert torch.equal(mixed["board"][i], src["board"][i])
            assert torch.equal(mixed["legal_moves"][i], src["legal_moves"][i])
        twice = rot180_batch(rot180_batch(orig, mask), mask)
        for key in orig:
            assert torch.equal(twice[key], orig[key]), key
        before = {k: v.clone() for k, v in orig.items()}
        rot180_batch(orig, ones)
        for key in orig:
            assert torch.equal(before[key], orig[key]), key               # the input is not modified


def test_refusals_and_defaults():
    from azalea_amd import AzaleaAgent, HexGame, Player
    from azalea_amd.device_replay import DeviceReplayBuffer
    game_factory = lambda: HexGame(5)   # noqa: E731
    with pytest.raises(ValueError, match="host loop"):
        Player(None, [AzaleaAgent(game_factory)], random_reflect=True)       # the random mover
    with pytest.raises(ValueError, match="host loop"):
        Player(None, [AzaleaAgent(game_factory), AzaleaAgent(game_factory)], random_reflect=True)
    player = Player(None, [AzaleaAgent(game_factory)])
    assert player.random_reflect is False and player._engine_flags == 0
    frame, metrics = player.read(20)                                          # behaves as today: the host loop plays
    assert len(frame) >= 20 and metrics["games"] >= 1
    player.stop()
    assert isinstance(DeviceReplayBuffer.random_reflect, property)
    # HexGame.random_reflect stays the reference's identity (hex.py:124-134)
    b, m = np.zeros((3, 3), np.int32), np.array([1, 2], np.int32)
    assert HexGame.random_reflect(b, m)[0] is b
