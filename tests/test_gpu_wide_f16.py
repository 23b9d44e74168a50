"""The plain-f16 WIDE tower on the device (AZX_FLAG_TOWER_F16 on 128 / 256 channels -> k_stem_wide_f16 +
k_conv_wide_f16_s16 per layer; opt-in, outside every parity claim).

Accuracy is held to the definition, not to the reference: tests/f16_wide_emulation.py is that definition in float64,
and its own error e_emu against the exact float64 module -- computed here, per fixture and per quantity -- is the unit.
Summation order alone moves a correct implementation by up to 1.3 e_emu from the float64 emulation, so by
up to 2.3 e_emu from exact; on these randomly initialised networks e_emu is of the order of the fp32 error of the heads
and of the split-f16 tower itself, so that error -- e_x3, the DEFAULT engine's own error on the same fixture, measured
in the same test -- is added: the bound is 4 e_emu + e_x3 + 1e-5.  A wrong tap, tile or fragment gives errors of order 1."""
import functools
import os
from contextlib import contextmanager

import numpy as np
import pytest

import f16_wide_emulation as emu
from azalea_amd import engine as eng
from azalea_amd._lib import AzxError

pytestmark = pytest.mark.gpu

NEW_TOWER, OLD_TOWER = "k_stem_wide_f16 + k_conv_wide_f16_s16 per layer", "k_stem_wide_f16x3 + k_conv_wide_f16x3_s16 per layer"


@contextmanager
def _environ(**env):
    """The switches are read once, by azx_create: set them around the creation of an engine."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(n, blocks, chans, flags=eng.FLAG_TOWER_F16, env=None, **kw):
    kw = dict(dict(n_games=8, simulations=10, search_batch_size=10, evaluator=eng.EVAL_RESNET), **kw)
    with _environ(**(env or {})):
        return eng.Engine(board_size=n, num_blocks=blocks, base_chans=chans, flags=flags, **kw)


def _forward(name, flags, env=None, boards=None, lm=None):
    """(kernel_info, value, logprob) of one engine on a fixture's weights (and its positions unless others are given)."""
    c = emu.case(name)
    E = _engine(c["n"], c["blocks"], c["chans"], flags=flags, env=env)
    try:
        E.set_weights(c["state"])
        value, logprob = E.forward(c["boards"] if boards is None else boards, c["lm"] if lm is None else lm)
        return E.kernel_info(), value, logprob
    finally:
        E.close()


@functools.lru_cache(maxsize=None)
def _flagged(name):
    return _forward(name, eng.FLAG_TOWER_F16)


@functools.lru_cache(maxsize=None)
def _default(name):
    return _forward(name, 0)


def _errors(c, value, logprob):
    return np.abs(value - c["value"]).max(), np.abs(logprob - c["logprob"])[c["legal"]].max()


def _check_accuracy(name, value, logprob):
    """The kernel's outputs against the exact float64 module: <= 4 e_emu + e_x3 + 1e-5; padded entries as
    test_gpu_tower_f16._check_forward holds them."""
    c = emu.case(name)
    legal = c["legal"]
    e_v, e_lp = _errors(c, c["emu_value"], c["emu_logprob"])
    _, dv, dlp = _default(name)
    x_v, x_lp = _errors(c, dv, dlp)
    k_v, k_lp = _errors(c, value, logprob)
    print("%s: kernel vs exact: value %.3g, log-prob %.3g; emulation vs exact: value %.3g, log-prob %.3g; default engine vs "
          "exact: value %.3g, log-prob %.3g; kernel vs emulation: value %.3g, log-prob %.3g"
          % (name, k_v, k_lp, e_v, e_lp, x_v, x_lp, np.abs(value - c["emu_value"]).max(),
             np.abs(logprob - c["emu_logprob"])[legal].max()))
    assert np.isfinite(value).all() and np.isfinite(logprob).all()
    assert k_v <= 4 * e_v + x_v + 1e-5, (k_v, e_v, x_v)
    assert k_lp <= 4 * e_lp + x_lp + 1e-5, (k_lp, e_lp, x_lp)
    assert (~legal).any()
    # a padded entry is -99 minus the row's log-normaliser: every padded entry of a row is the same number, within 1e-3
    # of the exact one plus the normaliser's share (4 x the emulation's own error on these entries)
    e_pad = np.abs(c["emu_logprob"] - c["logprob"])[~legal].max()
    k_pad = np.abs(logprob - c["logprob"])[~legal].max()
    print("%s: padded entries: kernel vs exact %.3g, emulation vs exact %.3g" % (name, k_pad, e_pad))
    assert k_pad <= 4 * e_pad + 1e-3, (k_pad, e_pad)
    for row, ok in zip(logprob, legal):
        if (~ok).any():
            assert np.ptp(row[~ok]) <= 1e-3 and row[~ok].max() < -90.0


@pytest.mark.parametrize("name", sorted(emu.FIXTURES))
def test_forward_accuracy(name):
    info, value, logprob = _flagged(name)
    assert NEW_TOWER in info and "AZX_TOWER=f16" in info and "k_heads" in info and "k_heads_mfma" not in info, info
    _check_accuracy(name, value, logprob)


def test_flag_is_in_effect():
    c = emu.case("19x256")
    fi, fv, flp = _flagged("19x256")
    di, dv, dlp = _default("19x256")
    assert NEW_TOWER in fi and "AZX_TOWER=f16" in fi and OLD_TOWER not in fi
    assert OLD_TOWER in di and "k_conv_wide_f16x3_s16" in di and "AZX_TOWER=default" in di and NEW_TOWER not in di
    assert di == fi.replace(NEW_TOWER, OLD_TOWER).replace("AZX_TOWER=f16", "AZX_TOWER=default")
    x_v, x_lp = _errors(c, dv, dlp)
    assert x_v <= 1e-4 and x_lp <= 1e-4, (x_v, x_lp)                      # the default engine is today's
    _, e_lp = _errors(c, c["emu_value"], c["emu_logprob"])
    diff = np.abs(flp - dlp)[c["legal"]].max()
    print("19x256: flagged vs default engine on legal log-probs %.3g, e_emu %.3g" % (diff, e_lp))
    assert diff >= e_lp / 4, (diff, e_lp)


def test_the_stream_split_does_not_change_a_bit():
    """11 boards: one part of 11, 8 + 3 over two streams, 8 + 3 with two more streams idle."""
    _, v2, lp2 = _flagged("13x13")                       # AZX_WIDE_STREAMS unset: 2
    for streams in ("1", "2", "4"):
        info, v, lp = _forward("13x13", eng.FLAG_TOWER_F16, env={"AZX_WIDE_STREAMS": streams})
        assert NEW_TOWER in info and "AZX_WIDE_STREAMS=%s" % streams in info
        assert v.tobytes() == v2.tobytes() and lp.tobytes() == lp2.tobytes(), streams


def test_a_row_does_not_depend_on_its_batch():
    c = emu.case("13x13")
    _, v, lp = _flagged("13x13")
    _, vr, lpr = _forward("13x13", eng.FLAG_TOWER_F16, boards=c["boards"][::-1].copy(), lm=c["lm"][::-1].copy())
    assert vr[::-1].tobytes() == v.tobytes() and lpr[::-1].tobytes() == lp.tobytes()     # another block, group and stream
    for i in (0, 10):
        _, v1, lp1 = _forward("13x13", eng.FLAG_TOWER_F16, boards=c["boards"][i:i + 1].copy(), lm=c["lm"][i:i + 1].copy())
        assert v1.tobytes() == v[i:i + 1].tobytes() and lp1.tobytes() == lp[i:i + 1].tobytes(), i


def test_environment_selects_the_tower_leniently():
    info, value, logprob = _forward("5x5", 0, env={"AZX_TOWER": "f16"})
    assert NEW_TOWER in info and "AZX_TOWER=f16" in info
    _check_accuracy("5x5", value, logprob)
    _, fv, flp = _flagged("5x5")
    assert value.tobytes() == fv.tobytes() and logprob.tobytes() == flp.tobytes()        # the same kernels as the flag's
    # no plain-f16 tower for 64 channels on 13x13: ignored, a working default engine
    state = emu.seeded_net(13, 1, 64, 5)
    boards, lm = emu.positions(13, 5, 6)
    E = _engine(13, 1, 64, flags=0, env={"AZX_TOWER": "f16"})
    try:
        assert "f16_s16" not in E.kernel_info() and "k_tower_mfma" in E.kernel_info()
        E.set_weights(state)
        value, logprob = E.forward(boards, lm)
        want_v, want_lp = emu.exact(13, 1, 64, state, boards, lm)
        assert np.abs(value - want_v).max() <= 1e-4 and np.abs(logprob - want_lp)[lm > 0].max() <= 1e-4
    finally:
        E.close()


@pytest.mark.parametrize("kw,env", [
    (dict(n=5, blocks=0, chans=128), {}),
    (dict(n=5, blocks=1, chans=128), {"AZX_TOWER": "fp32"}),
    (dict(n=5, blocks=1, chans=128, evaluator=eng.EVAL_UNIFORM), {}),
])
def test_refusals(kw, env):
    with pytest.raises(AzxError) as ei:
        _engine(env=env, **kw).close()
    assert "azx error -1:" in str(ei.value) and "AZX_FLAG_TOWER_F16" in str(ei.value), str(ei.value)     # AZX_EINVAL


def test_range_guard():
    n, blocks, chans = 7, 2, 128
    state = emu.seeded_net(n, blocks, chans, 71)
    boards, lm = emu.positions(n, 6, 72)
    huge = {k: v.copy() for k, v in state.items()}
    huge["resblocks.0.bn2.bias"] += 2e5
    E = _engine(n, blocks, chans)
    try:
        assert NEW_TOWER in E.kernel_info()
        E.set_weights(huge)
        with pytest.raises(AzxError) as ei:
            E.forward(boards, lm)
        assert "azx error -6:" in str(ei.value) and "activation" in str(ei.value), str(ei.value)     # AZX_ERANGE
        E.set_weights(state)                    # the flag does not stick to the next, valid network
        value, logprob = E.forward(boards, lm)
        assert np.isfinite(value).all() and np.isfinite(logprob).all()
        want_v, want_lp = emu.exact(n, blocks, chans, state, boards, lm)
        assert np.abs(value - want_v).max() <= 1e-3 and np.abs(logprob - want_lp)[lm > 0].max() <= 1e-3
    finally:
        E.close()


# ---- search level: a seeded 1x128 net on 5x5, 20 simulations, batch 4, device noise on -----------------------------
SEARCH = dict(simulations=20, search_batch_size=4, exploration_coef=0.5, exploration_depth=4, noise_alpha=0.3,
              noise_scale=0.25, temperature=1.0, seed=4321)
GAMES = 64


def _play_state():
    return emu.case("5x5")["state"]


@functools.lru_cache(maxsize=None)
def _harvest(slots):
    """{uid: (boards, colours, nlegal, moves_prob, reward)} of the games uid < GAMES."""
    E = _engine(5, 1, 128, n_games=slots, **SEARCH)
    try:
        assert NEW_TOWER in E.kernel_info()
        E.set_weights(_play_state())
        got = {}
        for _ in range(64):
            rows, st = E.play(slots * 8)
            m = E.play_row_metrics()
            assert st["game_errors"] == 0 and len(m) == len(rows["reward"])
            uid = rows["game_uid"]
            starts = np.flatnonzero(m[:, 3] > 0.5)
            for s, e in zip(starts, np.r_[starts[1:], len(uid)]):
                u = int(uid[s])
                assert (uid[s:e] == u).all() and u not in got
                got[u] = tuple(rows[k][s:e].copy() for k in ("board", "color", "nlegal", "moves_prob", "reward"))
            if all(u in got for u in range(GAMES)):
                break
        assert all(u in got for u in range(GAMES))
        return {u: got[u] for u in range(GAMES)}
    finally:
        E.close()


def test_harvested_games_are_legal_decided_hex_games():
    from oracle import oracle as orc
    games = _harvest(8)
    lengths = set()
    for u, (boards, colors, nlegal, prob, reward) in games.items():
        L = len(boards)
        lengths.add(L)
        h = orc.Hex(5)
        for p in range(L):
            assert h.result == 0 and h.color == colors[p] and np.array_equal(h.board, boards[p]), (u, p)
            assert nlegal[p] == len(h.legal_moves()) and abs(prob[p, :nlegal[p]].sum() - 1.0) < 1e-5
            assert reward[p] == (1.0 if (L - 1 - p) % 2 == 0 else -1.0), (u, p)     # the last mover won
            if p + 1 < L:
                new = np.flatnonzero(boards[p + 1].ravel() != boards[p].ravel())
                assert len(new) == 1 and boards[p].ravel()[new[0]] == 0, (u, p)
                h.step(int(new[0]) + 1)                  # raises on an illegal move
        wins = []
        for mv in h.legal_moves():                       # the move behind the last row ended the game: one exists
            h2 = h.copy()
            h2.step(int(mv))
            wins.append(h2.result != 0)
        assert any(wins), u
    assert len(lengths) > 3                               # noise and sampling are on: not one game played 64 times


def test_games_do_not_depend_on_the_pool_size():
    small, large = _harvest(8), _harvest(16)
    assert sorted(small) == sorted(large)
    for u in small:
        for x, y in zip(small[u], large[u]):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), u


def test_match_and_tournament_between_the_two_precisions():
    A = _engine(5, 1, 128, n_games=16, **SEARCH)
    B = _engine(5, 1, 128, flags=0, n_games=16, **dict(SEARCH, seed=1234))
    try:
        assert NEW_TOWER in A.kernel_info() and OLD_TOWER in B.kernel_info()
        A.set_weights(_play_state())
        B.set_weights(_play_state())
        M = eng.Match(A, B)
        try:
            one = M.play(16, moves=True)
        finally:
            M.close()
        wins_a, wins_b = int((one["outcome"] == 1).sum()), int((one["outcome"] == -1).sum())
        assert wins_a + wins_b == 16 and (one["length"] > 0).all(), one["outcome"]
        T = eng.Tournament([A, B])
        try:
            two = T.play([(0, 1)], 16, moves=True)[(0, 1)]
        finally:
            T.close()
        for k in ("outcome", "length", "moves"):
            assert np.array_equal(one[k], two[k]), k
    finally:
        A.close()
        B.close()
