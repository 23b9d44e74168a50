"""Replay rows harvested from device matches (azx_match_set_harvest, engine.Match.play(collect=...), the two-agent
device Player).  Everything is bit-exact: no tolerance is involved.

What is held, on the smallest shapes that reach both step instantiations (5x5 and 11x11: two cell slots, 13x13: three)
and the refill path (16 slots, 40 games from game 7: two refills, a remainder, idle slots at the end, both parities of
the game index):
  1. harvesting changes no game;
  2. every game's rows are that game (boards replayed by the host rules, colours, legal counts, rewards, first-row flag);
  3. the rows are the movers' rows, bit for bit (the two engines driven by hand, the draws' rows kept);
  4. the rows do not depend on the pool size;
  5. first_mover fixes who starts;
  6. voided games leave no rows and disturb no other game's;
  7. the queue's consumers (rows_pack, play_row_metrics) see the rows;
  8. a tournament's rows are its pairs' matches' rows, whatever the sink;
  9. Player(device_match=True).read hands out whole games.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_match_games as omg     # noqa: E402  (the prior table of the hash evaluator)

pytestmark = pytest.mark.gpu

# the two agent configurations of tests/test_gpu_match.py; simulations cut on the larger boards
AGENT_A = dict(sims=60, batch=10, c=0.5, depth=6, eps=0.0, alpha=0.3, temp=1.0)
AGENT_B = dict(sims=40, batch=8, c=1.5, depth=10, eps=0.25, alpha=0.3, temp=1.0)
SMALL = (dict(AGENT_A, sims=30), dict(AGENT_B, sims=24))
CASES = {                      # board size, evaluator, the two agents
    "hash5": (5, "hash", (AGENT_A, AGENT_B)),
    "hash11": (11, "hash", SMALL),
    "hash13": (13, "hash", SMALL),
    "net7": (7, "net", (AGENT_A, AGENT_B)),
}
SLOTS, GAMES, FIRST = 16, 40, 7
ROW_KEYS = ("board", "color", "nlegal", "moves_prob", "reward", "game_uid")


@pytest.fixture(scope="module")
def eng():
    from azalea_amd import engine
    return engine


_NETS = {}


def net_state(n, seed):
    """A seeded 1x64 HexNetwork with non-trivial BatchNorm statistics (as in tests/test_gpu_match.py)."""
    import torch
    from azalea_amd.network import HexNetwork
    if (n, seed) not in _NETS:
        torch.manual_seed(seed)
        net = HexNetwork(board_size=n, num_blocks=1, base_chans=64).eval()
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.6, 1.4)
        _NETS[(n, seed)] = {k: v.detach().numpy() for k, v in net.state_dict().items() if v.dtype.is_floating_point}
    return _NETS[(n, seed)]


def make_engine(n, G, cfg, seed, kind, net_seed=3, **kw):
    from azalea_amd import engine as eng
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


def pair(case, G, **kw_a):
    n, kind, cfgs = CASES[case]
    return (make_engine(n, G, cfgs[0], 11, kind, net_seed=3, **kw_a),
            make_engine(n, G, cfgs[1], 1 << 40, kind, net_seed=4))


@functools.lru_cache(maxsize=None)
def played(case, G=SLOTS, n_games=GAMES, first_game=FIRST, collect=True, first_mover=None):
    """One match on fresh engines; computed once and shared (nobody writes to it)."""
    from azalea_amd import engine as eng
    a, b = pair(case, G)
    m = eng.Match(a, b)
    res = m.play(n_games, first_game=first_game, moves=True, collect=collect, first_mover=first_mover)
    m.close()
    a.close()
    b.close()
    return res


def by_game(rows, metrics=None):
    """{u: that game's rows}; a game's rows must be contiguous."""
    uid = rows["game_uid"]
    out = {}
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]]) if len(uid) else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], len(uid)]
    for s, e in zip(starts, ends):
        u = int(uid[s])
        assert u not in out, "the rows of game %d are not contiguous" % u
        out[u] = {k: rows[k][s:e] for k in ROW_KEYS}
        if metrics is not None:
            out[u]["metrics"] = metrics[s:e]
    return out


def same_games(x, y):
    assert sorted(x) == sorted(y)
    for u in x:
        for k in x[u]:
            assert np.array_equal(x[u][k], y[u][k]), (u, k)


def first_agent(u, first_mover):
    return (u & 1) if first_mover is None else first_mover


def check_rows(res, n, first_game, first_mover=None):
    """Test 2 for one result of Match.play(moves=True, collect=True)."""
    from azalea_amd.game.hex import HexGame
    rows, meta = res["rows"], res["row_metrics"]
    games = by_game(rows, meta)
    length, outcome, moves = res["length"], res["outcome"], res["moves"]
    won = [i for i in range(len(outcome)) if outcome[i] != 0]
    assert sorted(games) == [first_game + i for i in won]                 # voided games leave no rows
    assert len(rows["reward"]) == res["n_rows"] == int(sum(length[i] for i in won)) == len(meta)
    assert rows["board"].shape == (res["n_rows"], n, n) and rows["moves_prob"].shape == (res["n_rows"], n * n)
    for i in won:
        u = first_game + i
        g = games[u]
        L = int(length[i])
        assert len(g["reward"]) == L, u
        x_won = (0 if outcome[i] > 0 else 1) == first_agent(u, first_mover)   # colour 1 = the first mover
        h = HexGame(n)
        for p in range(L):
            assert np.array_equal(g["board"][p], h.state.board), (u, p)
            k = int((h.state.board == 0).sum())
            assert g["color"][p] == (p & 1) and g["nlegal"][p] == k, (u, p)
            assert g["reward"][p] == (1.0 if x_won == (p % 2 == 0) else -1.0), (u, p)
            prob = g["moves_prob"][p]
            assert (prob[k:] == 0).all() and (prob[:k] >= 0).all() and abs(float(prob.sum()) - 1.0) < 1e-5, (u, p)
            assert prob[int(np.searchsorted(h.state.legal_moves, moves[i, p]))] > 0, (u, p)   # the move drawn had mass
            assert g["metrics"][p, 3] == (1.0 if p == 0 else 0.0), (u, p)
            assert g["metrics"][p, 6] == k, (u, p)                                        # search_root_children
            h.step(int(moves[i, p]))
        assert h.state.result == (3 if x_won else 1), u
    return games


def plain(res):
    st = dict(res["stats"])
    st.pop("seconds")
    return res["outcome"], res["length"], res["moves"], st


# ---- 1, 2, 4 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_harvesting_changes_no_game(case):
    off, on = played(case, collect=False), played(case)
    assert "rows" not in off and "n_rows" not in off
    for x, y in zip(plain(off), plain(on)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    st = on["stats"]
    assert st["voided"] == 0 and st["games"] == GAMES and st["wins"][0] + st["wins"][1] == GAMES


@pytest.mark.parametrize("case", list(CASES))
def test_every_games_rows_are_that_game(case):
    res = played(case)
    assert res["stats"]["voided"] == 0
    games = check_rows(res, CASES[case][0], FIRST)
    assert len(games) == GAMES and res["n_rows"] == int(res["length"].sum()) == res["stats"]["plies"]


@pytest.mark.parametrize("case", list(CASES))
def test_the_rows_do_not_depend_on_the_pool_size(case):
    small, large = played(case), played(case, G=64)
    assert small["stats"]["voided"] == large["stats"]["voided"] == 0
    same_games(by_game(small["rows"], small["row_metrics"]), by_game(large["rows"], large["row_metrics"]))


# ---- 3, 5: the two engines driven by hand -------------------------------------------------------------------------
def drive_by_hand(a, b, cfgs, n, first_mover=None):
    """tests/test_gpu_match.py's drive_by_hand (games u = slot through set_active / search / debug_choose / advance),
    keeping what every draw recorded: per game the list of (board before the move, legal count, moves_prob row)."""
    G, cells = a.G, n * n
    slot = np.arange(G)
    alive = np.ones(G, bool)
    kept = [[] for _ in range(G)]
    first = (slot & 1) if first_mover is None else np.full(G, first_mover)
    for ply in range(cells):
        if not alive.any():
            break
        mover = first ^ (ply & 1)
        ids = np.full(G, -1, np.int32)
        boards = a.get_games()["board"]
        for agent, E in enumerate((a, b)):
            mask = alive & (mover == agent)
            E.set_active(mask.astype(np.int32))
            if not mask.any():
                continue
            E.search(noise=None, noise_scale=cfgs[agent]["eps"])
            assert (E.get_status()[mask] == 0).all()
            mid, prob = E.debug_choose()
            assert (mid[mask] >= 0).all() and (mid[~mask] == -1).all()
            ids[mask] = mid[mask]
            for g in np.flatnonzero(mask):
                kept[g].append((boards[g].reshape(n, n).copy(), int((boards[g] == 0).sum()), prob[g].copy()))
        for E in (a, b):                                      # every agent follows every move
            E.set_active(alive.astype(np.int32))
            E.advance(ids)
        alive &= a.get_games()["result"] == 0
    assert not alive.any()
    return kept


def assert_rows_are_the_hand_rows(case, first_mover):
    from azalea_amd import engine as eng
    n, kind, cfgs = CASES[case]
    a, b = pair(case, SLOTS)
    kept = drive_by_hand(a, b, cfgs, n, first_mover)
    a.close()
    b.close()
    res = played(case, n_games=SLOTS, first_game=0, first_mover=first_mover)
    assert res["stats"]["voided"] == 0
    games = by_game(res["rows"])
    assert sorted(games) == list(range(SLOTS))
    for u, rows in enumerate(kept):
        g = games[u]
        assert len(rows) == len(g["reward"]) == res["length"][u], u
        for p, (board, k, prob) in enumerate(rows):
            assert np.array_equal(g["board"][p], board), (u, p)
            assert g["nlegal"][p] == k, (u, p)
            assert g["moves_prob"][p].tobytes() == prob.tobytes(), (u, p)      # bit for bit
    return res


@pytest.mark.parametrize("case", list(CASES))
def test_the_rows_are_the_movers_rows_bit_for_bit(case):
    assert_rows_are_the_hand_rows(case, None)


@pytest.mark.parametrize("mode", [0, 1])
def test_first_mover_fixes_who_starts(mode):
    case = "hash5"
    res = assert_rows_are_the_hand_rows(case, mode)           # every game's row 0 is agent `mode`'s
    check_rows(res, 5, 0, first_mover=mode)
    st = res["stats"]
    assert st["first_player_wins"] == st["wins"][mode] and st["voided"] == 0
    default = played(case, n_games=SLOTS, first_game=0)
    assert not np.array_equal(default["moves"], res["moves"])


def test_first_mover_default_is_todays_games_and_a_bad_mode_is_refused(eng):
    from azalea_amd._lib import AzxError
    a, b = pair("hash5", SLOTS)
    m = eng.Match(a, b)
    m.play(4, first_mover=1)
    with pytest.raises(AzxError, match="first mover mode 2"):
        m.play(4, first_mover=2)
    again = m.play(GAMES, first_game=FIRST, moves=True)       # back to agent u & 1, harvest off, on the same match
    for x, y in zip(plain(again), plain(played("hash5", collect=False))):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
    with pytest.raises(AzxError, match="outside the 0 rows queued"):
        a.rows_read(0, 1)                                     # a match that does not harvest leaves no rows
    m.close()
    a.close()
    b.close()


# ---- 6. voided games ----------------------------------------------------------------------------------------------
def test_voided_games_leave_no_rows(eng):
    """Engine a's arena cannot hold one search (tests/test_gpu_match.py::test_search_tree_full_voids_the_game_and_nothing_else):
    every game a takes part in is voided within its first two plies and leaves no rows.  Beside such a pair in one
    tournament, with one queue for both, the other pair's rows are intact: those of its own match, bit for bit."""
    n, G, rounds, first_game = 11, 8, 6, 5
    small = dict(SMALL[0], sims=40)

    def engines():
        return [make_engine(n, G, small, 11, "hash", nodes_per_game=500),
                make_engine(n, G, SMALL[1], 1 << 40, "hash"), make_engine(n, G, SMALL[0], 2 << 40, "hash")]

    es = engines()
    m = eng.Match(es[0], es[1])
    res = m.play(2 * G + 1, first_game=first_game, moves=True, collect=True)
    st = res["stats"]
    assert st["voided"] == st["games"] == 2 * G + 1 and res["n_rows"] == 0 and len(res["rows"]["reward"]) == 0
    assert res["row_metrics"].shape == (0, 8)
    m.close()
    m = eng.Match(es[1], es[2])
    ref = m.play(rounds, first_game=first_game + rounds, moves=True, collect=True)
    assert ref["stats"]["voided"] == 0
    m.close()
    for e in es:
        e.close()
    es = engines()
    t = eng.Tournament(es)
    out = t.play([(0, 1), (1, 2)], rounds, first_game=first_game, tables_per_pair=3, moves=True, collect=True, sink=1)
    t.close()
    for e in es:
        e.close()
    assert out[(0, 1)]["stats"]["voided"] == rounds and out[(1, 2)]["stats"]["voided"] == 0
    assert out["n_rows"] == int(out[(1, 2)]["length"].sum())          # the sum of the non-voided lengths
    res = dict(out[(1, 2)], rows=out["rows"], row_metrics=out["row_metrics"], n_rows=out["n_rows"])
    check_rows(res, n, first_game + rounds)
    same_games(by_game(out["rows"], out["row_metrics"]), by_game(ref["rows"], ref["row_metrics"]))


# ---- 7. the queue's consumers -------------------------------------------------------------------------------------
def test_the_queue_consumers_see_the_rows(eng):
    import torch
    from azalea_amd import distributed as azd
    from azalea_amd._lib import AzxError
    n = 5
    a, b = pair("hash5", SLOTS)
    m = eng.Match(a, b)
    res = m.play(GAMES, first_game=FIRST, collect="device")
    assert "rows" not in res and res["n_rows"] == int(res["length"].sum())
    rows = res["n_rows"]
    rec = torch.empty((rows, a.record_bytes), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    a.rows_pack(0, rows, rec.data_ptr())
    host = azd.unpack_rows(rec.cpu().numpy(), n)
    read = a.rows_read(0, rows)
    for k in ROW_KEYS:
        assert np.array_equal(np.asarray(host[k]).reshape(read[k].shape), read[k]), k
    same_games(by_game(read), by_game(played("hash5")["rows"]))
    assert a.play_row_metrics().shape == (rows, 8)
    part = a.rows_read(5, 9)                                  # a window of the queue
    for k in ROW_KEYS:
        assert np.array_equal(part[k], read[k][5:14]), k
    with pytest.raises(AzxError, match="outside"):
        a.rows_read(rows - 1, 2)
    # a queue that cannot hold the rows is an error, never a silent loss
    a.debug_set_queue_cap(rows // 2)
    with pytest.raises(AzxError, match="internal error"):
        m.play(GAMES, first_game=FIRST, collect="device")
    a.debug_set_queue_cap(0)
    a.reset()
    b.reset()
    assert m.play(GAMES, first_game=FIRST, collect="device")["n_rows"] == rows
    m.close()
    a.close()
    b.close()


# ---- 8. tournaments -----------------------------------------------------------------------------------------------
def test_a_tournaments_rows_are_its_pairs_matches_rows(eng):
    n, kind, rounds, first_game = 5, "hash", 6, 3
    cfgs = (AGENT_A, AGENT_B, dict(AGENT_A, sims=20, c=1.0))
    seeds = (11, 1 << 40, 2 << 40)
    pairs = [(0, 1), (0, 2), (1, 2)]

    def engines(G):
        return [make_engine(n, G, cfgs[k], seeds[k], kind) for k in range(3)]

    expect = {}
    for s, (i, j) in enumerate(pairs):
        es = engines(8)
        m = eng.Match(es[i], es[j])
        res = m.play(rounds, first_game=first_game + rounds * s, moves=True, collect=True)
        assert res["stats"]["voided"] == 0
        check_rows(res, n, first_game + rounds * s)
        expect[(i, j)] = (by_game(res["rows"], res["row_metrics"]), res["moves"])
        m.close()
        for e in es:
            e.close()
    for sink in (0, 2):
        es = engines(4)
        t = eng.Tournament(es)
        out = t.play(pairs, rounds, first_game=first_game, tables_per_pair=2, moves=True, collect=True, sink=sink)
        t.close()
        for e in es:
            e.close()
        games = by_game(out["rows"], out["row_metrics"])
        assert out["n_rows"] == sum(int(out[p]["length"].sum()) for p in pairs)
        for s, p in enumerate(pairs):
            assert np.array_equal(out[p]["moves"], expect[p][1])
            mine = {u: g for u, g in games.items() if first_game + rounds * s <= u < first_game + rounds * (s + 1)}
            same_games(mine, expect[p][0])


def test_evaluate_throughput_collects_each_pairs_rows():
    from azalea_amd import evaluation
    agents = device_agents(3)
    rounds = 4
    got = {}
    for pooled in (False, True):
        got[pooled] = {}
        games = {}
        evaluation.evaluate_throughput(agents, rounds, n_slots=4, seed=5, games=games, collect=got[pooled], pooled=pooled)
        for s, p in enumerate(evaluation.gen_pairs(3)):
            res = dict(games[p], rows=got[pooled][p]["rows"], row_metrics=got[pooled][p]["row_metrics"],
                       n_rows=len(got[pooled][p]["rows"]["reward"]))
            check_rows(res, 5, s * rounds)
    for p in got[False]:
        same_games(by_game(got[False][p]["rows"], got[False][p]["row_metrics"]),
                   by_game(got[True][p]["rows"], got[True][p]["row_metrics"]))


# ---- 9. the two-agent device Player -------------------------------------------------------------------------------
def device_agents(count, n=5, sims=20):
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


def test_player_reads_whole_two_agent_games_from_the_device():
    from azalea_amd.parallel_player import Player
    n = 5
    player = Player(None, device_agents(2), device_match=True, n_games=16)
    frame, metrics = player.read(200)
    assert len(frame) >= 200 and metrics["games"] >= 200 / (n * n)
    assert set(metrics) == {"games", "reward", "moves_per_game", "seconds_per_game", "game_error", "search_value",
                            "search_root_width", "action_logprob", "search_root_visits", "search_tree_nodes",
                            "search_root_children"}
    assert metrics["moves_per_game"] == len(frame) and metrics["game_error"] == 0
    # whole games: each starts from the empty board with colours alternating from 0, and ends just before a full stop
    starts = [i for i, s in enumerate(frame.state) if not s.board.any()]
    assert starts[0] == 0 and len(starts) == metrics["games"]
    for s, e in zip(starts, starts[1:] + [len(frame)]):
        assert 2 * n - 1 <= e - s <= n * n
        for p in range(s, e):
            st = frame.state[p]
            assert st.color == (p - s) & 1 and int((st.board != 0).sum()) == p - s
            assert len(frame.moves_prob[p]) == len(st.legal_moves) == n * n - (p - s)
        assert frame.reward[e - 1] == -frame.reward[e - 2] and abs(frame.reward[e - 1]) == 1.0
    player.stop()
    assert player._match is None


def test_reads_share_no_game():
    """The game indices behind successive reads, taken where the Player queues its games: chunk after chunk of
    2 * n_games games, no index twice."""
    from azalea_amd.parallel_player import Player
    player = Player(None, device_agents(2), device_match=True, n_games=16)
    seen = []
    orig = player._harvest

    def spy(eng_, rows, st, meta=None):
        seen.append(np.unique(rows["game_uid"]))
        return orig(eng_, rows, st, meta=meta)
    player._harvest = spy
    total = 0
    while len(seen) < 2:                                      # a chunk is 32 games of >= 9 rows: reads of 300 drain one
        frame, _ = player.read(300)
        total += len(frame)
    player.stop()
    assert len(seen) >= 2 and total >= 300
    assert not set(seen[0].tolist()) & set(seen[1].tolist())
    assert seen[0].min() == 0 and seen[0].max() == 31 and seen[1].min() == 32 and seen[1].max() == 63
