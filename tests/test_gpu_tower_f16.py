"""The plain-f16 tower on the device (AZX_FLAG_TOWER_F16 -> k_tower_f16_s16; opt-in, outside every parity claim).

Accuracy is held to the definition, not to the reference: tests/f16_emulation.py is that definition in float64, and
its own error e_emu against the exact float64 module -- computed here, per fixture and per quantity -- is the unit.
Summation order alone moves a correct implementation by up to 1.3 e_emu from the float64 emulation (measured with
fp32-accumulating and channel-reordered emulations when the switch was specified), so by up to 2.3 e_emu from exact;
the bound is 4 e_emu + 1e-5.  A wrong tap, tile or fragment gives errors of order 1.

Kernel errors measured on an MI355X, value / legal log-prob (e_emu beside them): G3 1.2e-4 / 5.4e-4 (8.8e-5 / 5.5e-4),
G8 1.5e-3 / 2.7e-2 (9.1e-4 / 2.6e-2); DESIGN 7.8."""
import functools
import os
from contextlib import contextmanager
from functools import partial

import numpy as np
import pytest
import torch

import f16_emulation
from azalea_amd import engine as eng
from azalea_amd._lib import AzxError
from azalea_amd.network import HexNetwork

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW_TOWER, OLD_TOWER = "k_tower_f16_s16", "k_tower_f16x3_s16"


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


def _seeded_net(n, blocks, seed):
    """Seeded net with randomised BatchNorm statistics, as test_forward_13x13_64ch_vs_oracle makes its own."""
    torch.manual_seed(seed)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=64).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.3, 1.7)
    return {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}


def _positions(n, count, seed):
    rng = np.random.RandomState(seed)
    boards = rng.randint(0, 3, size=(count, n, n)).astype(np.int32)
    boards[:, 0, 0] = 0
    lm = np.zeros((count, n * n), np.int32)
    for i in range(count):
        e = np.flatnonzero(boards[i].ravel() == 0) + 1
        lm[i, :len(e)] = e
    return boards, lm


@functools.lru_cache(maxsize=None)
def _case(name):
    """One fixture: weights, inputs, the exact float64 module's outputs and the float64 emulation's.  Computed once."""
    if name in ("g3", "g8"):
        z = np.load(os.path.join(GOLDEN, "g3_forward_11_6x64.npz" if name == "g3" else "g8_checkpoint.npz"))
        n, blocks, chans = [int(x) for x in z["cfg"]]
        state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
        boards, lm = z["board"], z["legal_moves"]
        assert len(boards) == (96 if name == "g3" else 48)
    elif name == "5x5":       # 7 boards: a dead partner board in the last block; 25 cells: rows >= ncells, less than a tile group
        n, blocks, chans, state = 5, 1, 64, _seeded_net(5, 1, 11)
        boards, lm = _positions(5, 7, 12)
    else:
        n, blocks, chans, state = 8, 2, 64, _seeded_net(8, 2, 21)
        boards, lm = _positions(8, 33, 22)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).double().eval()
    net.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    with torch.no_grad():
        out = net(torch.as_tensor(boards), torch.as_tensor(lm))
    ev, elp = f16_emulation.forward(state, blocks, boards, lm, rounded=True)
    return dict(n=n, blocks=blocks, chans=chans, state=state, boards=boards, lm=lm, legal=lm > 0,
                value=out["value"].numpy(), logprob=out["moves_logprob"].numpy(), emu_value=ev, emu_logprob=elp)


def _best(logprob, legal):
    return np.where(legal, logprob, -np.inf).argmax(1)


def _check_forward(name, E):
    c = _case(name)
    legal = c["legal"]
    E.set_weights(c["state"])
    value, logprob = E.forward(c["boards"], c["lm"])
    e_v = np.abs(c["emu_value"] - c["value"]).max()
    e_lp = np.abs(c["emu_logprob"] - c["logprob"])[legal].max()
    k_v = np.abs(value - c["value"]).max()
    k_lp = np.abs(logprob - c["logprob"])[legal].max()
    print("%s: kernel vs exact: value %.3g, log-prob %.3g; emulation vs exact: value %.3g, log-prob %.3g; kernel vs "
          "emulation: value %.3g, log-prob %.3g" % (name, k_v, k_lp, e_v, e_lp, np.abs(value - c["emu_value"]).max(),
                                                    np.abs(logprob - c["emu_logprob"])[legal].max()))
    assert np.isfinite(value).all() and np.isfinite(logprob).all()
    assert k_v <= 4 * e_v + 1e-5, (k_v, e_v)
    assert k_lp <= 4 * e_lp + 1e-5, (k_lp, e_lp)
    if name in ("g3", "g8"):
        assert np.array_equal(_best(c["emu_logprob"], legal), _best(c["logprob"], legal))
        assert np.array_equal(_best(logprob, legal), _best(c["logprob"], legal))
    if (~legal).any():
        # A padded entry is -99 minus the row's log-normaliser, so it moves with that normaliser: on G8 (peaked policies,
        # large logits) the float64 emulation's own padded entries sit 1.2e-2 from the exact module's, and no correct
        # kernel is within the 1e-3 that the parity tests hold them to.  What holds: every padded entry of a row is the
        # same number (the kernel's -99 log-softmax of that row), and it is within 1e-3 of the exact one plus the
        # normaliser's share, bounded like the other quantities by 4 x the emulation's own error on these entries.
        e_pad = np.abs(c["emu_logprob"] - c["logprob"])[~legal].max()
        k_pad = np.abs(logprob - c["logprob"])[~legal].max()
        print("%s: padded entries: kernel vs exact %.3g, emulation vs exact %.3g" % (name, k_pad, e_pad))
        assert k_pad <= 4 * e_pad + 1e-3, (k_pad, e_pad)
        for row, ok in zip(logprob, legal):
            if (~ok).any():
                assert np.ptp(row[~ok]) <= 1e-3 and row[~ok].max() < -90.0
    return value, logprob


@pytest.mark.parametrize("name", ["g3", "g8", "5x5", "8x8"])
def test_forward_accuracy(name):
    c = _case(name)
    E = _engine(c["n"], c["blocks"], c["chans"])
    try:
        assert NEW_TOWER in E.kernel_info() and "k_heads_mfma" in E.kernel_info()
        _check_forward(name, E)
    finally:
        E.close()


def test_flag_is_in_effect():
    c = _case("g8")
    F = _engine(c["n"], c["blocks"], c["chans"])
    D = _engine(c["n"], c["blocks"], c["chans"], flags=0)
    try:
        fi, di = F.kernel_info(), D.kernel_info()
        assert NEW_TOWER in fi and "AZX_TOWER=f16" in fi and OLD_TOWER not in fi
        assert OLD_TOWER in di and "AZX_TOWER=default" in di and NEW_TOWER not in di
        assert di == fi.replace(NEW_TOWER, OLD_TOWER).replace("AZX_TOWER=f16", "AZX_TOWER=default")
        F.set_weights(c["state"])
        D.set_weights(c["state"])
        fv, flp = F.forward(c["boards"], c["lm"])
        dv, dlp = D.forward(c["boards"], c["lm"])
        assert np.abs(dlp - c["logprob"])[c["legal"]].max() <= 1e-4       # the default engine is today's
        assert np.abs(flp - dlp)[c["legal"]].max() > 1e-4                  # (the emulation says 2.5e-2)
    finally:
        F.close()
        D.close()


def test_forward_behind_the_scalar_heads():
    c = _case("g3")
    E = _engine(c["n"], c["blocks"], c["chans"], env={"AZX_HEADS": "valu"})
    try:
        info = E.kernel_info()
        assert NEW_TOWER in info and "k_heads_mfma" not in info and "AZX_HEADS=valu" in info
        _check_forward("g3", E)
    finally:
        E.close()


def test_environment_selects_the_tower_leniently():
    E = _engine(5, 1, 64, flags=0, env={"AZX_TOWER": "f16"})
    try:
        assert NEW_TOWER in E.kernel_info() and "AZX_TOWER=f16" in E.kernel_info()
        _check_forward("5x5", E)
    finally:
        E.close()
    # no fused tower on 13x13: ignored, a working default engine
    state = _seeded_net(13, 1, 5)
    boards, lm = _positions(13, 5, 6)
    E = _engine(13, 1, 64, flags=0, env={"AZX_TOWER": "f16"})
    try:
        assert NEW_TOWER not in E.kernel_info() and "k_tower_mfma" in E.kernel_info()
        E.set_weights(state)
        value, logprob = E.forward(boards, lm)
        net = HexNetwork(board_size=13, num_blocks=1, base_chans=64).eval()
        net.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
        with torch.no_grad():
            out = net(torch.as_tensor(boards), torch.as_tensor(lm))
        assert np.abs(value - out["value"].numpy()).max() <= 1e-4
        assert np.abs(logprob - out["moves_logprob"].numpy())[lm > 0].max() <= 1e-4
    finally:
        E.close()


@pytest.mark.parametrize("kw,env", [
    (dict(n=5, blocks=1, chans=32), {}),
    (dict(n=13, blocks=1, chans=64), {}),
    (dict(n=5, blocks=0, chans=64), {}),
    (dict(n=5, blocks=1, chans=64, evaluator=eng.EVAL_UNIFORM), {}),
    (dict(n=5, blocks=1, chans=64, evaluator=eng.EVAL_EXTERNAL), {}),
    (dict(n=5, blocks=1, chans=64), {"AZX_TOWER": "fp32"}),
])
def test_refusals(kw, env):
    with pytest.raises(AzxError) as ei:
        _engine(env=env, **kw).close()
    assert "azx error -1:" in str(ei.value) and "AZX_FLAG_TOWER_F16" in str(ei.value), str(ei.value)     # AZX_EINVAL


def test_range_guard():
    """The weight set with which test_gpu_weights.py drives the split-f16 tower's residual stream past 65504."""
    import test_gpu_weights as tw
    n, blocks, chans = 11, 6, 64
    net = tw._net(n, blocks, chans)
    state = tw._state_np(net)
    boards, lm = tw._positions(n, 8)
    big = tw._scaled(state, 3e4 / tw._max_activation(net, boards), blocks)
    huge = {k: v.copy() for k, v in big.items()}
    huge["resblocks.0.bn2.bias"] += 2e5
    E = _engine(n, blocks, chans, n_games=2, simulations=20)
    try:
        assert NEW_TOWER in E.kernel_info()
        E.set_weights(huge)
        with pytest.raises(AzxError) as ei:
            E.forward(boards, lm)
        assert "azx error -6:" in str(ei.value) and "activation" in str(ei.value) and "plain f16" in str(ei.value)   # AZX_ERANGE
        E.set_weights(state)                    # the flag does not stick to the next, valid network
        value, logprob = E.forward(boards, lm)
        assert np.isfinite(value).all() and np.isfinite(logprob).all()
    finally:
        E.close()


# ---- search level: a seeded 1x64 net on 5x5, 20 simulations, batch 4, device noise on ------------------------------
SEARCH = dict(simulations=20, search_batch_size=4, exploration_coef=0.5, exploration_depth=4, noise_alpha=0.3,
              noise_scale=0.25, temperature=1.0, seed=4321)


@functools.lru_cache(maxsize=None)
def _harvest(slots, games, pipeline):
    """{uid: (boards, colours, nlegal, moves_prob, reward)} of the games uid < `games`, and the engine's stagger counters."""
    E = _engine(5, 1, 64, env={} if pipeline else {"AZX_PIPELINE": "0"}, n_games=slots, **SEARCH)
    try:
        info = E.kernel_info()
        assert NEW_TOWER in info and ("half an evaluation apart" in info) == pipeline
        E.set_weights(_seeded_net(5, 1, 11))
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
            if all(u in got for u in range(games)):
                break
        assert all(u in got for u in range(games))
        return {u: got[u] for u in range(games)}, E.debug_stagger()
    finally:
        E.close()


def _same_games(a, b):
    assert sorted(a) == sorted(b)
    for u in a:
        for x, y in zip(a[u], b[u]):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), u


def test_harvested_games_are_legal_decided_hex_games():
    from oracle import oracle as orc
    games, _ = _harvest(1024, 2048, True)                # 1024 slots, two generations
    assert len(games) == 2048
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
    assert len(lengths) > 3                               # noise and sampling are on: not one game played 2048 times


def test_games_do_not_depend_on_the_schedule():
    """One stream against the two staggered half-pools with their cut evaluation: a board's evaluation does not depend
    on its block, its partner board or its launch."""
    piped, stagger = _harvest(1024, 2048, True)
    single, none = _harvest(1024, 2048, False)
    assert stagger["starts"] > 0 and stagger["empty"] < stagger["starts"] and stagger["rows_queued"] > 0, stagger
    assert none["starts"] == 0, none
    _same_games(piped, single)


def test_games_do_not_depend_on_the_pool_size():
    small, _ = _harvest(1024, 2048, True)
    large, _ = _harvest(2048, 2048, True)
    _same_games(small, large)


# ---- matches: the same weights at the two precisions ---------------------------------------------------------------
def test_match_between_the_two_precisions():
    from azalea_amd import AzaleaAgent, HexGame
    from azalea_amd.evaluation import evaluate_throughput
    from azalea_amd.policy import Policy
    state = _seeded_net(5, 1, 11)
    agents = []
    for prec in ("f16", None):
        pol = Policy()
        pol.initialize(dict(device="cuda:0", network="HexNetwork", board_size=5, num_blocks=1, base_chans=64,
                            simulations=20, search_batch_size=4, exploration_coef=0.5, exploration_depth=4,
                            exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0, seed=3))
        pol.net.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
        pol.net.eval()
        pol.settings["move_sampling"] = True
        if prec:
            pol.tower_precision = prec
        agents.append(AzaleaAgent(partial(HexGame, 5), policy=pol, device="cuda:0"))
    tallies = []
    for pooled in (False, True):
        collect, info, games = {}, {}, {}
        out = evaluate_throughput(agents, 64, seed=7, pooled=pooled, collect=collect, info=info, games=games)
        tally = out[(0, 1)]
        assert tally[0] + tally[2] == 64 and tally[1] == 0 and (games[(0, 1)]["outcome"] != 0).all(), tally
        assert NEW_TOWER in info[0] and OLD_TOWER in info[1] and NEW_TOWER not in info[1]
        rows = collect[(0, 1)]["rows"]
        assert len(rows["reward"]) == int(games[(0, 1)]["length"].sum())
        assert (rows["color"] == 0).any() and (rows["color"] == 1).any()      # rows of both engines' moves
        assert len(np.unique(rows["game_uid"])) == 64
        tallies.append(tally)
    assert tallies[0] == tallies[1], tallies
