"""Device matches with engines whose evaluator is the caller's (azx_match_* with AZX_EVAL_EXTERNAL engines that
have an evaluator registered, engine.Match, evaluation.evaluate_throughput(external_batch=True)).

What is held:
  1. an EVAL_EXTERNAL engine with the uniform-hash stub registered as its evaluator plays, on either side of a match
     or on both, bit for bit the games of the inline uniform-hash engine (7x7 and 13x13);
  2. the games depend neither on the ply schedule (AZX_MATCH_INTERLEAVE) nor on the pool size;
  3. a real custom network (PyTorch forward of a seeded 1x64 HexNetwork inside a module that is not a HexNetwork)
     against the device tower plays the distribution of the all-device match of the same two weight sets;
  4. failures: an evaluator that raises, bad rows at a middle and at the last evaluation point of a search, an
     evaluator unregistered after the match was made, SearchTreeFull in an external engine's tree;
  5. the engines are the caller's again after a match;
  6. evaluate_throughput(external_batch=True) is the round robin over a mixed field.
No test here faults the device: the error paths raise Python exceptions and return bad VALUES from a callback.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import game_stats as gs                                          # noqa: E402
import oracle_match_games as omg                                 # noqa: E402
from test_gpu_external_eval import uniform_hash_evaluator        # noqa: E402
from test_gpu_match import AGENT_A, AGENT_B, check_games, make_engine, net_state   # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEEDS = (11, 1 << 40)
AZX_ESTATE, AZX_EEXTERNAL = -4, -7


def code_of(err):
    """The azx return code an AzxError carries in its text ("azx error -4: ...")."""
    return int(re.match(r"azx error (-?\d+):", str(err)).group(1))


@pytest.fixture(scope="module")
def eng():
    from azalea_amd import engine
    return engine


def ext_engine(eng, n, G, cfg, seed, evaluator=None, seen=None, **kw):
    """An EVAL_EXTERNAL engine with `evaluator` (default: the uniform-hash stub) registered."""
    E = eng.Engine(board_size=n, n_games=G, simulations=cfg["sims"], search_batch_size=cfg["batch"],
                   exploration_coef=cfg["c"], exploration_depth=cfg["depth"], noise_alpha=cfg["alpha"],
                   noise_scale=cfg["eps"], temperature=cfg["temp"], seed=seed, evaluator=eng.EVAL_EXTERNAL, **kw)
    E.set_external_evaluator(evaluator if evaluator is not None else uniform_hash_evaluator(n * n, seen))
    return E


def play_pair(eng, n, G, kinds, n_games, first_game, cfgs=(AGENT_A, AGENT_B), seen=None):
    """kinds: per agent 'ext' (external engine, hash stub registered) or 'hash' (the inline stub)."""
    engines = []
    for i, kind in enumerate(kinds):
        if kind == "ext":
            engines.append(ext_engine(eng, n, G, cfgs[i], SEEDS[i], seen=None if seen is None else seen[i]))
        else:
            engines.append(make_engine(eng, n, G, cfgs[i], SEEDS[i], "hash"))
    m = eng.Match(*engines)
    res = m.play(n_games, first_game=first_game, moves=True)
    m.close()
    for E in engines:
        E.close()
    return res


TALLIES = ("games", "wins", "first_player_wins", "voided", "plies")


def assert_same_records(x, y):
    for k in ("outcome", "length", "moves"):
        assert np.array_equal(x[k], y[k]), k
    for k in TALLIES:
        assert x["stats"][k] == y["stats"][k], k


_INLINE = {}


def inline_records(eng, n, G, n_games, first_game, cfgs=(AGENT_A, AGENT_B)):
    key = (n, n_games, first_game, tuple(tuple(sorted(c.items())) for c in cfgs))
    if key not in _INLINE:
        _INLINE[key] = play_pair(eng, n, G, ("hash", "hash"), n_games, first_game, cfgs)
    return _INLINE[key]


# ---- 1. bit for bit against the inline stub ---------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [("ext", "ext"), ("ext", "hash"), ("hash", "ext")])
def test_external_hash_engines_play_the_inline_stubs_games(eng, kinds):
    n, G = 7, 64
    n_games = 3 * G + 5
    want = inline_records(eng, n, G, n_games, 7)
    check_games(want, n, n_games, first_game=7)
    seen = ([], [])
    got = play_pair(eng, n, G, kinds, n_games, 7, seen=seen)
    assert_same_records(got, want)
    for i, kind in enumerate(kinds):
        if kind == "ext":
            batch = (AGENT_A, AGENT_B)[i]["batch"]
            print("agent %d: %d hand-overs, rows max %d mean %.1f" % (i, len(seen[i]), max(seen[i]), np.mean(seen[i])))
            assert max(seen[i]) > batch                          # more than one game's leaf batch ...
            assert max(seen[i]) <= G * batch                     # ... and never more than the pool's


def test_external_hash_engines_play_the_inline_stubs_games_on_13x13(eng):
    """Three mask words and flipped legal lists; a small pool and short searches (the stub's hash walks the 169
    cells in PyTorch at every hand-over)."""
    n, G = 13, 8
    n_games = G + 3
    cfgs = (dict(AGENT_A, sims=20), dict(AGENT_B, sims=16))
    want = inline_records(eng, n, G, n_games, 7, cfgs)
    check_games(want, n, n_games, first_game=7)
    seen = ([], [])
    assert_same_records(play_pair(eng, n, G, ("ext", "ext"), n_games, 7, cfgs, seen=seen), want)
    assert_same_records(play_pair(eng, n, G, ("hash", "ext"), n_games, 7, cfgs), want)
    for i in range(2):
        assert cfgs[i]["batch"] < max(seen[i]) <= G * cfgs[i]["batch"]


# ---- 2. schedule independence -----------------------------------------------------------------------------------
_CHILD = r"""
import os
import sys
import numpy as np
sys.path[:0] = [sys.argv[1], os.path.dirname(sys.argv[1])]
from azalea_amd import engine as eng
import test_gpu_match_external as t
res = t.play_pair(eng, 7, int(sys.argv[3]), ("ext", "ext"), int(sys.argv[4]), 7)
np.savez(sys.argv[2], outcome=res["outcome"], length=res["length"], moves=res["moves"],
         **{k: np.asarray(res["stats"][k]) for k in t.TALLIES})
"""


def child_records(tmp_path, tag, G, n_games, interleave):
    """The ext-vs-ext match in a fresh process (the switch is read at azx_match_create from the environment)."""
    out = str(tmp_path / ("match_%s.npz" % tag))
    env = dict(os.environ, AZX_MATCH_INTERLEAVE=str(interleave))
    subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(os.path.abspath(__file__)), out, str(G),
                    str(n_games)], env=env, check=True, timeout=600)
    z = dict(np.load(out))
    return dict(outcome=z["outcome"], length=z["length"], moves=z["moves"],
                stats={k: z[k].tolist() for k in TALLIES})


def test_the_games_do_not_depend_on_the_schedule_or_the_pool_size(eng, tmp_path):
    n, n_games = 7, 3 * 64 + 5
    plain = child_records(tmp_path, "plain", 64, n_games, 0)
    inter = child_records(tmp_path, "inter", 64, n_games, 1)
    assert_same_records(plain, inter)
    assert_same_records(plain, inline_records(eng, n, 64, n_games, 7))
    large = play_pair(eng, n, 256, ("ext", "ext"), n_games, 7)
    assert_same_records(large, plain)
    check_games(large, n, n_games, first_game=7)


# ---- 3. a real custom network -----------------------------------------------------------------------------------
class WrappedNet(torch.nn.Module):
    """A network that is NOT a HexNetwork (so nothing can take the device tower for it) and evaluates with the
    PyTorch forward of one."""

    def __init__(self, n, seed, blocks=1, chans=64):
        super().__init__()
        from azalea_amd.network import HexNetwork
        self.inner = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans)
        self.inner.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in net_state(n, seed, blocks, chans).items()},
                                   strict=False)
        self.eval()

    def run(self, batch):
        return self.inner.run(batch)


def sample_of(res, games):
    assert res["stats"]["voided"] == 0
    agent0_first = (np.arange(games) & 1) == 0
    agent0_wins = res["outcome"] > 0
    return dict(length=res["length"].astype(np.int32), agent0_wins=agent0_wins.astype(np.int8),
                first_wins=(agent0_wins == agent0_first).astype(np.int8), agent0_first=agent0_first.astype(np.int8))


def net_match(eng, n, G, games, seeds, custom, moves=False):
    """Weights 3 under AGENT_A against weights 4 under AGENT_B; `custom`: agent 0 through WrappedNet in PyTorch."""
    from azalea_amd.policy import external_evaluator
    if custom:
        net = WrappedNet(n, 3).to(DEV)
        a = ext_engine(eng, n, G, AGENT_A, seeds[0], evaluator=external_evaluator(net))
    else:
        a = make_engine(eng, n, G, AGENT_A, seeds[0], "net", net_seed=3)
    b = make_engine(eng, n, G, AGENT_B, seeds[1], "net", net_seed=4)
    m = eng.Match(a, b)
    res = m.play(games, moves=moves)
    m.close()
    a.close()
    b.close()
    return res


def test_a_custom_network_plays_the_device_towers_distribution(eng):
    """4096 games on 1024 slots, 7x7, as tests/test_gpu_match.py::test_the_match_plays_the_reference_distribution.
    The PyTorch forward and the device tower agree to 1e-4, not bitwise, so the games are compared as a
    distribution: this match against the pooled sample of two all-device matches on other engine seeds, which
    are first compared with each other (the calibration).  Measured on an MI355X: 30 s for the test, 27 s of it the
    custom network's match (mostly the convolution library preparing its kernels for each padded batch size)."""
    n, games, G = 7, 4096, 1024
    res = net_match(eng, n, G, games, (20261016, 20261016 + (1 << 40)), custom=True, moves=True)
    check_games(res, n, games)
    assert res["stats"]["voided"] == 0 and 0 < res["stats"]["wins"][0] < games
    e = sample_of(res, games)
    a = sample_of(net_match(eng, n, G, games, (777, 777 + (1 << 40)), custom=False), games)
    b = sample_of(net_match(eng, n, G, games, (31337, 31337 + (1 << 40)), custom=False), games)
    same = omg.compare(a, b)
    ref = {k: np.concatenate([a[k], b[k]]) for k in e}
    got = omg.compare(e, ref)
    print("device vs device: %s" % same)
    print("custom vs device: %s" % got)
    print("agent 0 wins: custom %.4f device %.4f / %.4f; length %.2f vs %.2f / %.2f; seconds %.2f" % (
        e["agent0_wins"].mean(), a["agent0_wins"].mean(), b["agent0_wins"].mean(), e["length"].mean(),
        a["length"].mean(), b["length"].mean(), res["stats"]["seconds"]))
    assert gs.worst(same)[1] > min(gs.P_MIN, 0.05 / len(same)), gs.worst(same)
    bad = {k: v for k, v in got.items() if v <= gs.P_MIN}
    assert not bad, bad


# ---- 4. errors --------------------------------------------------------------------------------------------------
class Boom(Exception):
    pass


def counting(cells, act, at):
    """The hash stub; on its `at`-th call (1-based) `act(value, prior)` spoils the results or raises."""
    inner = uniform_hash_evaluator(cells)
    calls = [0]

    def evaluate(board, legal):
        calls[0] += 1
        value, prior = inner(board, legal)
        if calls[0] == at:
            return act(value, prior, legal)
        return value, prior
    evaluate.calls = calls
    return evaluate


def test_an_evaluator_that_raises_fails_the_match_and_the_engine_until_reset(eng):
    from azalea_amd._lib import AzxError
    n, G = 7, 64
    n_games = 3 * G + 5

    def boom(value, prior, legal):
        raise Boom("evaluator failed")

    a = ext_engine(eng, n, G, AGENT_A, SEEDS[0])
    b = ext_engine(eng, n, G, AGENT_B, SEEDS[1])
    hash_b = uniform_hash_evaluator(n * n)
    # in the middle of a ply: the third evaluation point of engine b's second search
    b.set_external_evaluator(counting(n * n, boom, b.num_batches + 1 + 3))
    m = eng.Match(a, b)
    with pytest.raises(Boom) as info:
        m.play(n_games, first_game=7, moves=True)
    cause = info.value.__cause__
    assert isinstance(cause, AzxError) and code_of(cause) == AZX_EEXTERNAL and "engine b" in str(cause), cause
    b.set_external_evaluator(hash_b)
    with pytest.raises(AzxError) as info:
        b.play(200)
    assert code_of(info.value) == AZX_ESTATE
    with pytest.raises(AzxError) as info:
        m.play(5)
    assert code_of(info.value) == AZX_ESTATE
    m.close()
    a.reset()
    b.reset()
    m = eng.Match(a, b)
    assert_same_records(m.play(n_games, first_game=7, moves=True), inline_records(eng, n, G, n_games, 7))
    m.close()
    a.close()
    b.close()


def nan_value(value, prior, legal):
    value = value.clone()
    value[3] = float("nan")
    return value, prior


def short_priors(value, prior, legal):
    prior = prior.clone()
    prior[5] *= 0.9
    return value, prior


@pytest.mark.parametrize("where", ["middle", "last"])
@pytest.mark.parametrize("what", ["nan", "sum"])
@pytest.mark.parametrize("side", ["a", "b"])
def test_a_bad_row_fails_the_match_with_the_engine_and_the_row(eng, side, what, where):
    """The evaluator counts its calls; a search has engine.num_batches + 1 of them.  'last': the final point of the
    engine's second search, whose import no later hand-over of that search follows."""
    from azalea_amd._lib import AzxError
    n, G = 7, 64
    a = ext_engine(eng, n, G, AGENT_A, SEEDS[0])
    b = ext_engine(eng, n, G, AGENT_B, SEEDS[1])
    E = a if side == "a" else b
    points = E.num_batches + 1
    at = points + (3 if where == "middle" else points)
    act, row, text = (nan_value, 3, "not finite") if what == "nan" else (short_priors, 5, "sum is not 1")
    fn = counting(n * n, act, at)
    E.set_external_evaluator(fn)
    m = eng.Match(a, b)
    with pytest.raises(AzxError) as info:
        m.play(2 * G)
    err = info.value
    assert code_of(err) == AZX_EEXTERNAL, err
    assert "engine %s" % side in str(err) and "row %d " % row in str(err) and text in str(err), err
    # found before the evaluator is asked again: a middle point's error word comes with the next point's read, the
    # last point's with the ply's read-back, before the next ply's searches are enqueued
    assert fn.calls[0] == at, (at, fn.calls[0])
    with pytest.raises(AzxError) as info:
        m.play(5)
    assert code_of(info.value) == AZX_ESTATE
    m.close()
    a.close()
    b.close()


def test_unregistering_the_evaluator_after_create_is_a_state_error(eng):
    from azalea_amd._lib import AzxError
    n, G = 7, 16
    a = ext_engine(eng, n, G, AGENT_A, SEEDS[0])
    b = make_engine(eng, n, G, AGENT_B, SEEDS[1], "hash")
    m = eng.Match(a, b)
    assert m.play(5)["stats"]["games"] == 5
    a.set_external_evaluator(None)
    with pytest.raises(AzxError, match="EXTERNAL") as info:
        m.play(5)
    assert code_of(info.value) == AZX_ESTATE
    a.set_external_evaluator(uniform_hash_evaluator(n * n))
    assert m.play(5)["stats"]["games"] == 5
    m.close()
    a.close()
    b.close()


def test_search_tree_full_in_an_external_engine_voids_the_game_and_nothing_else(eng):
    """The shape of tests/test_gpu_match.py::test_search_tree_full_voids_the_game_and_nothing_else with agent 0 an
    external engine whose arena cannot hold one search."""
    n, G = 11, 16
    n_games = 2 * G + 1
    small = dict(AGENT_A, sims=40)
    a = ext_engine(eng, n, G, small, 11, nodes_per_game=500)
    b = make_engine(eng, n, G, AGENT_B, 1 << 40, "hash")
    m = eng.Match(a, b)
    res = m.play(n_games, moves=True)
    st = res["stats"]
    assert st["voided"] == st["games"] == n_games and st["wins"] == [0, 0]
    assert (res["outcome"] == 0).all() and (res["length"] <= 1).all()
    assert st["plies"] == int(res["length"].sum())
    m.close()
    a.close()
    b.close()
    res = play_pair(eng, 7, 32, ("ext", "hash"), 40, 0)       # a normal match afterwards
    check_games(res, 7, 40)


# ---- 5. the engines are the caller's again ----------------------------------------------------------------------
def test_the_engines_are_the_callers_again_after_a_match(eng):
    n, G = 7, 64
    a = ext_engine(eng, n, G, AGENT_A, SEEDS[0])
    b = ext_engine(eng, n, G, AGENT_B, SEEDS[1])
    m = eng.Match(a, b)
    m.play(G + 3)
    for E in (a, b):
        rows, st = E.play(200)
        assert st["games"] > 0 and st["game_errors"] == 0 and len(rows["reward"]) >= 200
        assert len(np.unique(rows["game_uid"])) == st["games"]           # whole games
    m.play(3)
    m.close()
    for E in (a, b):
        rows, st = E.play(200)
        assert st["games"] > 0 and st["game_errors"] == 0 and len(rows["reward"]) >= 200
        E.close()


# ---- 6. the round robin over a mixed field ----------------------------------------------------------------------
def mixed_agents(n=7):
    """One HexNetwork agent and two custom ones (1x32 towers inside WrappedNet)."""
    from azalea_amd.azalea_agent import AzaleaAgent
    from azalea_amd.game.hex import HexGame
    from azalea_amd.policy import Policy
    out = []
    for seed in (1, 2, 3):
        torch.manual_seed(seed)
        p = Policy()
        p.initialize(dict(device="cuda:0", network="HexNetwork", board_size=n, num_blocks=1, base_chans=32,
                          simulations=20 + 10 * seed, search_batch_size=10, exploration_coef=0.5, exploration_depth=6,
                          exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0))
        if seed > 1:
            p.net = WrappedNet(n, 10 + seed, blocks=1, chans=32).to(DEV)
        p.settings["move_sampling"] = True
        p.settings["move_exploration"] = seed == 2
        out.append(AzaleaAgent(lambda: HexGame(n), policy=p, device="cuda:0"))
    return out


def test_evaluate_throughput_is_the_round_robin_over_a_mixed_field():
    from azalea_amd import evaluation
    n, rounds = 7, 25
    agents = mixed_agents(n)
    with pytest.raises(TypeError):
        evaluation.evaluate_throughput(agents, rounds, n_slots=16, seed=5)
    games = {}
    out = evaluation.evaluate_throughput(agents, rounds, n_slots=16, seed=5, games=games, external_batch=True)
    assert list(out) == evaluation.gen_pairs(3) == list(games)
    for s, p in enumerate(out):
        w = out[p]
        assert w[1] == 0 and sum(w) == rounds
        g = games[p]
        assert w[0] == int((g["outcome"] > 0).sum()) and w[2] == int((g["outcome"] < 0).sum())
        check_games(dict(g, stats=dict(games=rounds, voided=0, wins=[w[0], w[2]], plies=int(g["length"].sum()),
                                       first_player_wins=int(sum((g["outcome"][i] > 0) == (((s * rounds + i) & 1) == 0)
                                                                 for i in range(rounds))), seconds=1.0)),
                    n, rounds, first_game=s * rounds)
    again = evaluation.evaluate_throughput(agents, rounds, n_slots=16, seed=5, games=(g1 := {}), external_batch=True)
    other_slots = evaluation.evaluate_throughput(agents, rounds, n_slots=8, seed=5, games=(g2 := {}), external_batch=True)
    for p in games:
        for k in ("outcome", "length", "moves"):
            assert np.array_equal(g1[p][k], games[p][k]), (p, k)
            assert np.array_equal(g2[p][k], games[p][k]), (p, k)
    assert {p: list(v) for p, v in again.items()} == {p: list(v) for p, v in out.items()}
    assert {p: list(v) for p, v in other_slots.items()} == {p: list(v) for p, v in out.items()}
    other = evaluation.evaluate_throughput(agents, rounds, n_slots=16, seed=6, games=(g3 := {}), external_batch=True)
    assert any(not np.array_equal(g3[p]["moves"], games[p]["moves"]) for p in games)
    assert all(sum(v) == rounds for v in other.values())
