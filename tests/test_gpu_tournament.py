"""A whole round robin as one device-resident tournament (azx_tournament_*, engine.Tournament,
evaluation.evaluate_throughput(pooled=True)): P matches side by side in one ply loop, sharing K engines.

What is held:
  1. the tournament is its matches, bit for bit: pair s = (i, j) plays the games of
     Match(engine_i, engine_j).play(rounds, first_game + rounds * s) on freshly built engines (records and tallies);
  2. the records depend neither on tables_per_pair nor on spare slots, and a gauntlet is its matches too;
  3. every recorded game replays under the host rules to its recorded result;
  4. SearchTreeFull voids the games of the pairs it occurs in and nothing else;
  5. bad arguments are AZX_EINVAL with a telling message, and the engines stay the caller's;
  6. engines with a registered external evaluator play the inline engines' games, and an evaluator's exception is
     re-raised from play();
  7. evaluate_throughput(pooled=True) returns exactly what pooled=False returns.
No tolerance anywhere: Match is already held to the reference's distribution and to the engines driven by hand
(tests/test_gpu_match.py).  No test here faults the device: tree-full is a status, and the failing evaluator raises
a Python exception.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_match_games as omg     # noqa: E402

pytestmark = pytest.mark.gpu

AZX_EINVAL, AZX_ESTATE, AZX_EEXTERNAL = -1, -4, -7
# four different agents, in the vocabulary of tests/test_gpu_match.py (AGENT_A and AGENT_B are its two)
AGENT_A = dict(sims=60, batch=10, c=0.5, depth=6, eps=0.0, alpha=0.3, temp=1.0)
AGENT_B = dict(sims=40, batch=8, c=1.5, depth=10, eps=0.25, alpha=0.3, temp=1.0)
AGENT_C = dict(sims=30, batch=6, c=1.0, depth=8, eps=0.25, alpha=0.5, temp=1.0)
AGENT_D = dict(sims=50, batch=10, c=0.8, depth=4, eps=0.0, alpha=0.3, temp=0.5)
AGENTS = (AGENT_A, AGENT_B, AGENT_C, AGENT_D)
SEEDS = (11, 1 << 40, (2 << 40) + 5, (3 << 40) + 9)
TALLIES = ("games", "wins", "first_player_wins", "voided", "plies")
ALL_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def code_of(err):
    """The azx return code an AzxError carries in its text ("azx error -4: ...")."""
    return int(re.match(r"azx error (-?\d+):", str(err)).group(1))


@pytest.fixture(scope="module")
def eng():
    from azalea_amd import engine
    return engine


_NETS = {}


def net_state(n, seed, blocks=1, chans=64):
    """A seeded 1x64 HexNetwork with non-trivial BatchNorm statistics (as tests/test_gpu_match.py)."""
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
    """kind 'hash': the uniform-prior / board-hash stub evaluator; 'net': the seeded 1x64 device network;
    'ext': an EVAL_EXTERNAL engine with the hash stub registered (tests/test_gpu_match_external.py's ext_engine)."""
    common = dict(board_size=n, n_games=G, simulations=cfg["sims"], search_batch_size=cfg["batch"],
                  exploration_coef=cfg["c"], exploration_depth=cfg["depth"], noise_alpha=cfg["alpha"],
                  noise_scale=cfg["eps"], temperature=cfg["temp"], seed=seed, **kw)
    if kind == "hash":
        E = eng.Engine(evaluator=eng.EVAL_UNIFORM_HASH, **common)
        E.set_prior_table(omg.prior_table(n))
    elif kind == "ext":
        from test_gpu_external_eval import uniform_hash_evaluator
        E = eng.Engine(evaluator=eng.EVAL_EXTERNAL, **common)
        E.set_external_evaluator(uniform_hash_evaluator(n * n, None))
    else:
        E = eng.Engine(evaluator=eng.EVAL_RESNET, num_blocks=1, base_chans=64, **common)
        E.set_weights(net_state(n, net_seed))
    return E


def field(eng, n, G, kinds, count=4, **kw):
    """Engines 0 .. count-1: agent k under AGENTS[k], SEEDS[k], network weights 3 + k.  G: one pool size or one per
    engine; kinds: one kind or one per engine."""
    Gs = [G] * count if isinstance(G, int) else list(G)
    ks = [kinds] * count if isinstance(kinds, str) else list(kinds)
    return [make_engine(eng, n, Gs[k], AGENTS[k], SEEDS[k], ks[k], net_seed=3 + k, **kw) for k in range(count)]


def close_all(engines):
    for E in engines:
        E.close()


def play_tournament(eng, n, G, kinds, pairs, rounds, first_game, tables, count=4):
    engines = field(eng, n, G, kinds, count)
    t = eng.Tournament(engines)
    res = t.play(pairs, rounds, first_game=first_game, tables_per_pair=tables, moves=True)
    t.close()
    close_all(engines)
    return res


_MATCHES = {}


def match_records(eng, n, kind, pair, rounds, first_game, G=16):
    """Match(engine_i, engine_j).play on freshly built engines of the same seeds and configurations."""
    key = (n, kind, pair, rounds, first_game)
    if key not in _MATCHES:
        i, j = pair
        a = make_engine(eng, n, G, AGENTS[i], SEEDS[i], kind, net_seed=3 + i)
        b = make_engine(eng, n, G, AGENTS[j], SEEDS[j], kind, net_seed=3 + j)
        m = eng.Match(a, b)
        _MATCHES[key] = m.play(rounds, first_game=first_game, moves=True)
        m.close()
        a.close()
        b.close()
    return _MATCHES[key]


def assert_same_records(x, y, what=""):
    for k in ("outcome", "length", "moves"):
        assert np.array_equal(x[k], y[k]), (what, k)
    for k in TALLIES:
        assert x["stats"][k] == y["stats"][k], (what, k)


def check_games(res, n, n_games, first_game=0):
    """Replay every record with the host rules (tests/test_gpu_match.py's check_games)."""
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


# ---- 1. the tournament is its matches ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hash", "net"])
def test_the_tournament_is_its_matches_bit_for_bit(eng, kind):
    """Four engines, all six pairs, 21 rounds on 8 tables per pair: refills, a remainder, tables that go idle.  Every
    engine is in three pairs and owns exactly its 24 slots."""
    n, rounds, tables, first_game = 7, 21, 8, 1000
    res = play_tournament(eng, n, 3 * tables, kind, ALL_PAIRS, rounds, first_game, tables)
    assert list(res) == ALL_PAIRS
    for s, p in enumerate(ALL_PAIRS):
        want = match_records(eng, n, kind, p, rounds, first_game + rounds * s)
        assert_same_records(res[p], want, p)
        assert res[p]["stats"]["seconds"] > 0
    assert len({res[p]["stats"]["seconds"] for p in ALL_PAIRS}) == 1          # the whole call's device time
    assert any(0 < res[p]["stats"]["wins"][0] < rounds for p in ALL_PAIRS)


# ---- 2. independence of the layout ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hash", "net"])
def test_the_records_do_not_depend_on_the_layout(eng, kind):
    n, rounds, first_game = 7, 21, 1000
    base = play_tournament(eng, n, 24, kind, ALL_PAIRS, rounds, first_game, 8)
    three = play_tournament(eng, n, 24, kind, ALL_PAIRS, rounds, first_game, 3)
    spare = play_tournament(eng, n, (24, 40, 64, 25), kind, ALL_PAIRS, rounds, first_game, 8)
    for p in ALL_PAIRS:
        assert_same_records(three[p], base[p], ("3 tables", p))
        assert_same_records(spare[p], base[p], ("spare slots", p))
    # tables_per_pair left to the wrapper: the most every engine has room for
    engines = field(eng, n, (24, 40, 64, 25), kind)
    t = eng.Tournament(engines)
    auto = t.play(ALL_PAIRS, rounds, first_game=first_game, moves=True)
    t.close()
    close_all(engines)
    for p in ALL_PAIRS:
        assert_same_records(auto[p], base[p], ("default tables", p))


@pytest.mark.parametrize("kind", ["hash", "net"])
def test_a_gauntlet_is_its_matches(eng, kind):
    """One candidate (engine 3, always the pair's second engine) against three others: engine 3 holds three pairs'
    slots, the others one pair's."""
    n, rounds, tables, first_game = 7, 21, 8, 1000
    pairs = [(0, 3), (1, 3), (2, 3)]
    res = play_tournament(eng, n, (8, 8, 8, 24), kind, pairs, rounds, first_game, tables)
    for s, p in enumerate(pairs):
        assert_same_records(res[p], match_records(eng, n, kind, p, rounds, first_game + rounds * s), p)
    # ... and in another order, with the candidate first in one pair: other game numbers, other matches
    pairs = [(3, 1), (2, 3)]
    res = play_tournament(eng, n, (8, 8, 8, 24), kind, pairs, rounds, first_game, tables)
    for s, p in enumerate(pairs):
        assert_same_records(res[p], match_records(eng, n, kind, p, rounds, first_game + rounds * s), p)


# ---- 3. legal games ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hash", "net"])
def test_every_recorded_game_is_a_legal_game_with_the_recorded_result(eng, kind):
    n, rounds, first_game = 7, 21, 7
    res = play_tournament(eng, n, 24, kind, ALL_PAIRS, rounds, first_game, 8)
    for s, p in enumerate(ALL_PAIRS):
        check_games(res[p], n, rounds, first_game=first_game + rounds * s)
    lean_engines = field(eng, n, 24, kind)
    t = eng.Tournament(lean_engines)
    lean = t.play([(0, 1), (2, 3)], 5)                         # fewer rounds than tables, no records asked for
    t.close()
    close_all(lean_engines)
    assert all("moves" not in v and v["stats"]["games"] == 5 for v in lean.values())


# ---- 4. SearchTreeFull ------------------------------------------------------------------------------------------
def test_search_tree_full_voids_the_game_and_nothing_else(eng):
    """Engine 0's arena cannot hold one search (the construction of tests/test_gpu_match.py's test of the same
    name): it searches every game of its two pairs within their first two plies, so all of those are voided, while
    the third pair plays on beside them."""
    n, rounds, tables = 11, 9, 4
    small = dict(AGENT_A, sims=40)
    engines = [make_engine(eng, n, 2 * tables, small, SEEDS[0], "hash", nodes_per_game=500),
               make_engine(eng, n, 2 * tables, AGENT_B, SEEDS[1], "hash"),
               make_engine(eng, n, 2 * tables, AGENT_C, SEEDS[2], "hash")]
    t = eng.Tournament(engines)
    pairs = [(0, 1), (0, 2), (1, 2)]
    res = t.play(pairs, rounds, tables_per_pair=tables, moves=True)          # returns OK
    t.close()
    close_all(engines)
    for p in pairs[:2]:
        st = res[p]["stats"]
        assert st["voided"] == st["games"] == rounds and st["wins"] == [0, 0], (p, st)
        assert (res[p]["outcome"] == 0).all() and (res[p]["length"] <= 1).all()
        assert st["plies"] == int(res[p]["length"].sum())
    check_games(res[(1, 2)], n, rounds, first_game=2 * rounds)
    # a normal tournament afterwards
    engines = field(eng, 7, 16, "hash", count=3)
    t = eng.Tournament(engines)
    res = t.play(pairs, 12, tables_per_pair=8, moves=True)
    t.close()
    close_all(engines)
    for s, p in enumerate(pairs):
        check_games(res[p], 7, 12, first_game=12 * s)


# ---- 5. bad arguments -------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_the_engines_stay_the_callers(eng):
    from azalea_amd._lib import AzxError
    n, G = 7, 16
    engines = field(eng, n, G, "hash", count=3)
    a, b, c = engines

    def refused(make, text):
        with pytest.raises(AzxError, match=text) as info:
            make()
        assert code_of(info.value) == AZX_EINVAL, info.value

    other_board = make_engine(eng, 5, G, AGENT_B, 5, "hash")
    refused(lambda: eng.Tournament([a, b, other_board]), "board")
    refused(lambda: eng.Tournament([a, b, a]), "same engine")
    refused(lambda: eng.Tournament([a]), "two engines")
    external = eng.Engine(board_size=n, n_games=G, evaluator=eng.EVAL_EXTERNAL)
    refused(lambda: eng.Tournament([a, external, b]), "engine 1 .*EXTERNAL")
    no_weights = eng.Engine(board_size=n, n_games=G, evaluator=eng.EVAL_RESNET, num_blocks=1, base_chans=64)
    refused(lambda: eng.Tournament([a, b, no_weights]), "engine 2 .*weights")
    close_all([other_board, external, no_weights])

    t = eng.Tournament(engines)
    refused(lambda: t.play([(0, 1), (1, 2), (0, 1)], 4, tables_per_pair=2), "repeats")
    refused(lambda: t.play([(0, 1), (1, 0)], 4, tables_per_pair=2), "repeats")
    refused(lambda: t.play([(0, 1), (2, 2)], 4, tables_per_pair=2), "a == b")
    refused(lambda: t.play([(0, 1), (1, 3)], 4, tables_per_pair=2), "out of range")
    refused(lambda: t.play([(0, 1), (-1, 2)], 4, tables_per_pair=2), "out of range")
    refused(lambda: t.play([(0, 1)], 0, tables_per_pair=2), "rounds")
    refused(lambda: t.play([(0, 1)], 4, tables_per_pair=0), "tables_per_pair")
    refused(lambda: t.play([], 4, tables_per_pair=2), "pair")
    # engine 1 is in two pairs: 2 * 9 = 18 slots needed, it has 16
    refused(lambda: t.play([(0, 1), (1, 2)], 4, tables_per_pair=9), r"engine 1 has n_games = 16 .* need 18")
    # the engines are the caller's again after a tournament, and after the tournament is closed
    t.play([(0, 1), (0, 2), (1, 2)], 11, tables_per_pair=8)
    for E in engines:
        rows, st = E.play(200)
        assert st["games"] > 0 and st["game_errors"] == 0 and len(rows["reward"]) >= 200
    t.play([(0, 1)], 3)
    t.close()
    for E in engines:
        rows, st = E.play(200)
        assert st["games"] > 0 and st["game_errors"] == 0
        E.close()


# ---- 6. external evaluators -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [("hash", "ext", "hash", "hash"), ("ext", "hash", "hash", "ext")])
def test_external_engines_play_the_inline_stubs_tournament(eng, kinds):
    n, rounds, tables, first_game = 7, 21, 8, 1000
    res = play_tournament(eng, n, 24, kinds, ALL_PAIRS, rounds, first_game, tables)
    for s, p in enumerate(ALL_PAIRS):
        assert_same_records(res[p], match_records(eng, n, "hash", p, rounds, first_game + rounds * s), p)


class Boom(Exception):
    pass


def test_an_evaluator_that_raises_is_reraised_and_fails_its_engine_until_reset(eng):
    from azalea_amd._lib import AzxError
    from test_gpu_external_eval import uniform_hash_evaluator
    n, rounds, tables, first_game = 7, 21, 8, 1000
    pairs = [(0, 1), (0, 2), (1, 2)]
    engines = field(eng, n, 16, ("hash", "hash", "ext"), count=3)
    bad = engines[2]
    inner = uniform_hash_evaluator(n * n, None)
    calls = [0]

    def evaluate(board, legal):
        calls[0] += 1
        if calls[0] == bad.num_batches + 1 + 3:               # the third evaluation point of its second search
            raise Boom("evaluator failed")
        return inner(board, legal)

    bad.set_external_evaluator(evaluate)
    t = eng.Tournament(engines)
    with pytest.raises(Boom) as info:
        t.play(pairs, rounds, first_game=first_game, tables_per_pair=tables, moves=True)
    cause = info.value.__cause__
    assert isinstance(cause, AzxError) and code_of(cause) == AZX_EEXTERNAL and "engine 2" in str(cause), cause
    bad.set_external_evaluator(inner)
    with pytest.raises(AzxError) as info:
        bad.play(200)
    assert code_of(info.value) == AZX_ESTATE
    with pytest.raises(AzxError) as info:
        t.play(pairs, 5)
    assert code_of(info.value) == AZX_ESTATE
    for E in engines:
        E.reset()
    res = t.play(pairs, rounds, first_game=first_game, tables_per_pair=tables, moves=True)
    t.close()
    close_all(engines)
    for s, p in enumerate(pairs):
        assert_same_records(res[p], match_records(eng, n, "hash", p, rounds, first_game + rounds * s), p)


# ---- 7. the round robin -----------------------------------------------------------------------------------------
def device_agents(count, n=7, sims=20):
    """tests/test_gpu_match.py's device_agents: 1x32 networks, agent 2 with device noise."""
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


def test_evaluate_throughput_pooled_returns_what_the_pairs_loop_returns():
    from azalea_amd import evaluation
    n, rounds = 7, 25
    agents = device_agents(3, n=n)
    want_games = {}
    want = evaluation.evaluate_throughput(agents, rounds, n_slots=16, seed=5, games=want_games)
    for n_slots in (16, None):                                # 8 tables per pair (< rounds); the default: 25
        games = {}
        got = evaluation.evaluate_throughput(agents, rounds, n_slots=n_slots, seed=5, games=games, pooled=True)
        assert list(got) == list(want) == evaluation.gen_pairs(3) == list(games)
        assert {p: list(v) for p, v in got.items()} == {p: list(v) for p, v in want.items()}
        for p in want_games:
            assert set(games[p]) == set(want_games[p]) == {"outcome", "length", "moves"}
            for k in want_games[p]:
                assert games[p][k].dtype == want_games[p][k].dtype
                assert np.array_equal(games[p][k], want_games[p][k]), (n_slots, p, k)
    assert all(v[1] == 0 and sum(v) == rounds for v in want.values())
