"""Evaluation matches between two engines played entirely on the device (azx_match_*, engine.Match,
evaluation.evaluate_throughput).

What is held:
  1. every recorded game is a legal game with the recorded result (replayed by the host rules);
  2. the match plays exactly the games the two engines play when the host drives them ply by ply through the
     existing calls (set_active / search / debug_choose / advance): same kernels, same (seed, uid, ply) streams;
  3. the games do not depend on the pool size (uid = game index, refills start from a clean slot);
  4. the two agents are neither interchangeable nor mixed up, and bad pairings are AZX_EINVAL;
  5. SearchTreeFull voids a game and nothing else;
  6. the match plays the REFERENCE's two-agent games as a distribution: against the CPU oracle under numpy's RNG
     (tests/oracle_match_games.py), two-sample tests of tests/game_stats.py, thresholds as in
     tests/test_gpu_game_distribution.py (the power of the comparison: tests/test_match_api.py);
  7. evaluate_throughput returns the round robin's tallies, reproducibly.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import game_stats as gs              # noqa: E402
import oracle_match_games as omg     # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# two different agents (test 2 and the cases of test 6 use the same vocabulary as tests/oracle_match_games.py)
AGENT_A = dict(sims=60, batch=10, c=0.5, depth=6, eps=0.0, alpha=0.3, temp=1.0)
AGENT_B = dict(sims=40, batch=8, c=1.5, depth=10, eps=0.25, alpha=0.3, temp=1.0)


@pytest.fixture(scope="module")
def eng():
    from azalea_amd import engine
    return engine


_NETS = {}


def net_state(n, seed, blocks=1, chans=64):
    """A seeded 1x64 HexNetwork with non-trivial BatchNorm statistics (the `net7` construction of
    tests/test_gpu_game_distribution.py)."""
    import torch
    from azalea_amd.network import HexNetwork
    key = (n, seed, blocks, chans)
    if key not in _NETS:
        torch.manual_seed(seed)
        net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).eval()
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.6, 1.4)
        _NETS[key] = {k: v.detach().numpy() for k, v in net.state_dict().items() if v.dtype.is_floating_point}
    return _NETS[key]


def make_engine(eng, n, G, cfg, seed, kind, net_seed=3, **kw):
    """kind 'hash': the uniform-prior / board-hash stub evaluator; 'net': the seeded 1x64 device network."""
    common = dict(board_size=n, n_games=G, simulations=cfg["sims"], search_batch_size=cfg["batch"],
                  exploration_coef=cfg["c"], exploration_depth=cfg["depth"], noise_alpha=cfg["alpha"],
                  noise_scale=cfg["eps"], temperature=cfg["temp"], seed=seed, **kw)
    if kind == "hash":
        E = eng.Engine(evaluator=eng.EVAL_UNIFORM_HASH, **common)
        E.set_prior_table(omg.prior_table(n))
    else:
        E = eng.Engine(evaluator=eng.EVAL_RESNET, num_blocks=1, base_chans=64, **common)
        E.set_weights(net_state(n, net_seed))
    return E


def pair(eng, n, G, kind, seeds=(11, 1 << 40), cfgs=(AGENT_A, AGENT_B)):
    return (make_engine(eng, n, G, cfgs[0], seeds[0], kind, net_seed=3),
            make_engine(eng, n, G, cfgs[1], seeds[1], kind, net_seed=4))


def check_games(res, n, n_games, first_game=0):
    """Test 1: replay every record with the host rules."""
    from azalea_amd.game.hex import HexGame
    outcome, length, moves, st = res["outcome"], res["length"], res["moves"], res["stats"]
    assert outcome.shape == (n_games,) and length.shape == (n_games,) and moves.shape == (n_games, n * n)
    for i in range(n_games):
        u = first_game + i
        L = int(length[i])
        assert 2 * n - 1 <= L <= n * n, (u, L)
        assert (moves[i, L:] == 0).all()
        h = HexGame(n)
        for p in range(L):
            assert h.state.result == 0, (u, p)                # not over before its recorded length
            assert int(moves[i, p]) in h.state.legal_moves, (u, p)
            h.step(int(moves[i, p]))
        result = h.state.result
        assert result in (1, 3), (u, "not over at its recorded length")
        first = u & 1                                         # the agent that moved first (colour X)
        winner = first if result == 3 else 1 - first
        assert outcome[i] == (1 if winner == 0 else -1), u
    first_wins = int(sum((outcome[i] > 0) == (((first_game + i) & 1) == 0) for i in range(n_games)))
    assert st["games"] == n_games and st["voided"] == 0
    assert st["wins"] == [int((outcome > 0).sum()), int((outcome < 0).sum())]
    assert st["wins"][0] + st["wins"][1] + st["voided"] == st["games"]
    assert st["first_player_wins"] == first_wins
    assert st["plies"] == int(length.sum())
    assert st["seconds"] > 0


@pytest.mark.parametrize("kind", ["hash", "net"])
def test_every_recorded_game_is_a_legal_game_with_the_recorded_result(eng, kind):
    n, G = 7, 64
    n_games = 3 * G + 5                                       # refills, an odd remainder, idle slots at the end
    a, b = pair(eng, n, G, kind)
    m = eng.Match(a, b)
    res = m.play(n_games, first_game=7, moves=True)
    check_games(res, n, n_games, first_game=7)
    assert 0 < res["stats"]["wins"][0] < n_games              # both agents win some
    lean = m.play(5)                                          # fewer games than slots, no records asked for
    assert "moves" not in lean and lean["stats"]["games"] == 5
    m.close()
    a.close()
    b.close()


def drive_by_hand(a, b, cfgs, n):
    """The match of games u = slot, played through the existing per-ply calls with the host in the loop."""
    G, cells = a.G, n * n
    slot = np.arange(G)
    alive = np.ones(G, bool)
    moves = np.zeros((G, cells), np.int16)
    length = np.zeros(G, np.int16)
    outcome = np.zeros(G, np.int8)
    for ply in range(cells):
        if not alive.any():
            break
        mover = (slot & 1) ^ (ply & 1)
        ids = np.full(G, -1, np.int32)
        legal = a.get_root()["legal_moves"]
        for agent, E in enumerate((a, b)):
            mask = alive & (mover == agent)
            E.set_active(mask.astype(np.int32))
            if not mask.any():
                continue
            E.search(noise=None, noise_scale=cfgs[agent]["eps"])
            assert (E.get_status()[mask] == 0).all()
            mid, _ = E.debug_choose()
            assert (mid[mask] >= 0).all() and (mid[~mask] == -1).all()
            ids[mask] = mid[mask]
        for E in (a, b):                                      # every agent follows every move
            E.set_active(alive.astype(np.int32))
            E.advance(ids)
        for g in np.flatnonzero(alive):
            moves[g, ply] = legal[g, ids[g]]
        ga, gb = a.get_games(), b.get_games()
        assert np.array_equal(ga["board"], gb["board"]) and np.array_equal(ga["result"], gb["result"])
        done = alive & (ga["result"] != 0)
        for g in np.flatnonzero(done):
            first = g & 1
            winner = first if ga["result"][g] == 3 else 1 - first
            outcome[g] = 1 if winner == 0 else -1
            length[g] = ply + 1
        alive &= ~done
    assert not alive.any()
    return outcome, length, moves


@pytest.mark.parametrize("kind", ["hash", "net"])
def test_the_match_is_the_two_engines_driven_by_hand(eng, kind):
    n, G = 7, 64
    cfgs = (AGENT_A, AGENT_B)
    a, b = pair(eng, n, G, kind)
    outcome, length, moves = drive_by_hand(a, b, cfgs, n)
    a.close()
    b.close()
    a, b = pair(eng, n, G, kind)
    m = eng.Match(a, b)
    res = m.play(G, first_game=0, moves=True)
    m.close()
    a.close()
    b.close()
    assert np.array_equal(res["moves"], moves)
    assert np.array_equal(res["length"], length)
    assert np.array_equal(res["outcome"], outcome)


def play_in(eng, n, G, kind, n_games, first_game, swap=False):
    a, b = pair(eng, n, G, kind)
    m = eng.Match(b, a) if swap else eng.Match(a, b)
    res = m.play(n_games, first_game=first_game, moves=True)
    m.close()
    a.close()
    b.close()
    return res


@pytest.mark.parametrize("kind", ["hash", "net"])
def test_the_games_do_not_depend_on_the_pool_size(eng, kind):
    """uid = game index: game u draws from (engine seed + u, ply) whatever slot it lands in, and a refilled slot
    starts from a clean tree."""
    n, n_games, first_game = 7, 256, 1000
    small = play_in(eng, n, 64, kind, n_games, first_game)
    large = play_in(eng, n, 256, kind, n_games, first_game)
    for k in ("outcome", "length", "moves"):
        assert np.array_equal(small[k], large[k]), k
    check_games(small, n, n_games, first_game)


def test_agents_are_not_interchangeable_and_bad_pairings_are_refused(eng):
    from azalea_amd._lib import AzxError
    n, G = 7, 64
    ab = play_in(eng, n, G, "hash", G, 0)
    again = play_in(eng, n, G, "hash", G, 0)
    ba = play_in(eng, n, G, "hash", G, 0, swap=True)
    assert np.array_equal(ab["moves"], again["moves"])         # deterministic ...
    assert not np.array_equal(ab["moves"], ba["moves"])        # ... and Match(b, a) is a different match
    a, b = pair(eng, n, G, "hash")
    with pytest.raises(AzxError, match="a == b"):
        eng.Match(a, a)
    other_board = make_engine(eng, 5, G, AGENT_B, 5, "hash")
    with pytest.raises(AzxError, match="board"):
        eng.Match(a, other_board)
    other_pool = make_engine(eng, n, G // 2, AGENT_B, 5, "hash")
    with pytest.raises(AzxError, match="n_games"):
        eng.Match(a, other_pool)
    external = eng.Engine(board_size=n, n_games=G, evaluator=eng.EVAL_EXTERNAL)
    with pytest.raises(AzxError, match="EXTERNAL"):
        eng.Match(a, external)
    no_weights = eng.Engine(board_size=n, n_games=G, evaluator=eng.EVAL_RESNET, num_blocks=1, base_chans=64)
    with pytest.raises(AzxError, match="weights"):
        eng.Match(a, no_weights)
    for E in (other_board, other_pool, external, no_weights):
        E.close()
    # the engines are the caller's again after a match, and after the match is closed
    m = eng.Match(a, b)
    m.play(G + 3)
    for E in (a, b):
        rows, st = E.play(200)
        assert st["games"] > 0 and st["game_errors"] == 0 and len(rows["reward"]) >= 200
    m.play(3)
    m.close()
    for E in (a, b):
        rows, st = E.play(200)
        assert st["games"] > 0 and st["game_errors"] == 0
        E.close()


def test_search_tree_full_voids_the_game_and_nothing_else(eng):
    """Engine a's arena cannot hold one search (the status tests/test_gpu_tree_parity.py::test_tree_full_sets_status
    provokes): a searches every game within its first two plies, so every game is voided; the slots refill and
    finally go idle, and the call returns."""
    from azalea_amd.policy import SearchTreeFull
    n, G = 11, 16
    n_games = 2 * G + 1
    small = dict(AGENT_A, sims=40)
    a = make_engine(eng, n, G, small, 11, "hash", nodes_per_game=500)
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
    # a normal match afterwards
    a, b = pair(eng, 7, 32, "hash")
    m = eng.Match(a, b)
    check_games(m.play(40, moves=True), 7, 40)
    m.close()
    a.close()
    b.close()
    agents = device_agents(2, n=11, sims=40)
    agents[0].policy.nodes_per_game = 500
    from azalea_amd import evaluation
    with pytest.raises(SearchTreeFull):
        evaluation.evaluate_throughput(agents, 4)


# ---- 6. the distribution is the reference's ---------------------------------------------------------------------
def oracle_sample(tmp_path, n, cfgs, games, seed0):
    out = str(tmp_path / ("oracle_match_%d_%d.npz" % (games, seed0)))
    subprocess.check_call([sys.executable, os.path.join(HERE, "oracle_match_games.py"), "--n", str(n), "--agents",
                           json.dumps(list(cfgs)), "--games", str(games), "--seed0", str(seed0), "--out", out])
    return dict(np.load(out))


def engine_sample(eng, n, cfgs, games, G, seeds):
    a = make_engine(eng, n, G, cfgs[0], seeds[0], "hash")
    b = make_engine(eng, n, G, cfgs[1], seeds[1], "hash")
    m = eng.Match(a, b)
    res = m.play(games)
    m.close()
    a.close()
    b.close()
    assert res["stats"]["voided"] == 0
    agent0_first = (np.arange(games) & 1) == 0
    agent0_wins = res["outcome"] > 0
    return dict(length=res["length"].astype(np.int32), agent0_wins=agent0_wins.astype(np.int8),
                first_wins=(agent0_wins == agent0_first).astype(np.int8), agent0_first=agent0_first.astype(np.int8))


MATCH_CASES = {
    "A": (AGENT_A, dict(AGENT_A, sims=10)),
    "B": (AGENT_A, AGENT_B),
}


@pytest.mark.parametrize("case", ["A", "B"])
def test_the_match_plays_the_reference_distribution(eng, case, tmp_path):
    n, games, G = 7, 4096, 1024
    cfgs = MATCH_CASES[case]
    a = oracle_sample(tmp_path, n, cfgs, games, 0)
    b = oracle_sample(tmp_path, n, cfgs, games, 1000000)
    same = omg.compare(a, b)
    e = engine_sample(eng, n, cfgs, games, G, seeds=(20261016, 20261016 + (1 << 40)))
    ref = {k: np.concatenate([a[k], b[k]]) for k in e}
    res = omg.compare(e, ref)
    print("[%s] oracle vs oracle: %s" % (case, same))
    print("[%s] engine vs oracle: %s" % (case, res))
    print("[%s] agent 0 wins: engine %.4f oracle %.4f / %.4f; first player wins %.4f vs %.4f / %.4f; "
          "length %.2f vs %.2f / %.2f" % (case, e["agent0_wins"].mean(), a["agent0_wins"].mean(), b["agent0_wins"].mean(),
                                          e["first_wins"].mean(), a["first_wins"].mean(), b["first_wins"].mean(),
                                          e["length"].mean(), a["length"].mean(), b["length"].mean()))
    assert gs.worst(same)[1] > min(gs.P_MIN, 0.05 / len(same)), gs.worst(same)
    bad = {k: v for k, v in res.items() if v <= gs.P_MIN}
    assert not bad, bad


# ---- 7. the round robin -----------------------------------------------------------------------------------------
def device_agents(count, n=7, sims=20):
    import torch
    from azalea_amd.azalea_agent import AzaleaAgent
    from azalea_amd.game.hex import HexGame
    from azalea_amd.policy import Policy
    out = []
    for seed in range(1, count + 1):
        torch.manual_seed(seed)
        p = Policy()
        p.initialize(dict(device="cuda:0", network="HexNetwork", board_size=n, num_blocks=1, base_chans=32,
                          simulations=sims + 10 * seed, search_batch_size=10, exploration_coef=0.5, exploration_depth=6,
                          exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0))
        p.settings["move_sampling"] = True
        p.settings["move_exploration"] = seed == 2            # one agent with device noise
        out.append(AzaleaAgent(lambda: HexGame(n), policy=p, device="cuda:0"))
    return out


def test_evaluate_throughput_is_the_round_robin():
    from azalea_amd import evaluation
    n, rounds = 7, 25
    agents = device_agents(3, n=n)
    games = {}
    out = evaluation.evaluate_throughput(agents, rounds, n_slots=16, seed=5, games=games)
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
    again = evaluation.evaluate_throughput(agents, rounds, n_slots=16, seed=5)
    assert {p: list(v) for p, v in again.items()} == {p: list(v) for p, v in out.items()}
    default_slots = evaluation.evaluate_throughput(agents, rounds, seed=5)          # 26 slots: the same games
    assert {p: list(v) for p, v in default_slots.items()} == {p: list(v) for p, v in out.items()}
    other = evaluation.evaluate_throughput(agents, rounds, n_slots=16, seed=6, games=(g2 := {}))
    assert any(not np.array_equal(g2[p]["moves"], games[p]["moves"]) for p in games)
    assert all(sum(v) == rounds for v in other.values())
