"""Device matches and tournaments from an opening book (azx_match_set_openings, azx_tournament_set_openings,
engine.Match / Tournament .play(openings=...), evaluate_throughput(openings=...), Player(device_match=True,
openings=...)).  Everything is bit-exact: no tolerance is involved.

What is held, on 5x5 and 7x7 in 16 to 64 slots (the smallest shapes that reach the refill path, idle slots at the
end, and both parities of the opening length and of the game index):
  1. every record begins with its game's opening -- (u >> 1) % n, or u % n under a fixed first mover -- and replays
     under the host rules to the recorded result at the recorded total length; stats.plies counts the played moves;
  2. the match is the two engines reset to the openings (Engine.reset(moves=...)) and driven by hand;
  3. a slot seeded at entry and a slot refilled later hold the same game (the games do not depend on the pool size);
  4. a tournament pair plays its match's games; evaluate_throughput pooled or not;
  5. the harvested rows of a game begin at its opening's length;
  6. without a book -- never set, cleared, or one empty opening -- nothing changes;
  7. a refused book leaves the previous one in place.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_match as tgm                                   # noqa: E402
from test_gpu_match import AGENT_A, AGENT_B, make_engine, pair  # noqa: E402
from test_gpu_match_rows import by_game, same_games            # noqa: E402

pytestmark = pytest.mark.gpu

# lengths 0, 1, 2, 3, 4 and 7: both parities, so the OTHER agent opens the search in some games
BOOK7 = [[], [25], [25, 18], [10, 40, 24], [1, 49, 2, 48], [4, 46, 11, 39, 18, 32, 26]]
BOOK5 = [[13], [], [7, 19, 12], [1, 25], [3, 8, 13, 18, 24]]


@pytest.fixture(scope="module")
def eng():
    from azalea_amd import engine
    assert hasattr(engine, "openings_check") and hasattr(engine.Match, "set_openings")
    return engine


def opening_of(u, book, first_mover=None):
    return ((u >> 1) if first_mover is None else u) % len(book)


def position(n, moves):
    from azalea_amd.game.hex import HexGame
    h = HexGame(n)
    for mv in moves:
        h.step(int(mv))
    return h


def check_games(res, n, n_games, first_game, book, first_mover=None):
    """tests/test_gpu_match.py's check_games for games that start from `book`."""
    outcome, length, moves, st = res["outcome"], res["length"], res["moves"], res["stats"]
    assert outcome.shape == (n_games,) and length.shape == (n_games,) and moves.shape == (n_games, n * n)
    assert res["opening"].dtype == np.int32 and res["opening"].shape == (n_games,)
    opened = 0
    for i in range(n_games):
        u = first_game + i
        o = opening_of(u, book, first_mover)
        assert res["opening"][i] == o, u
        op = book[o]
        opened += len(op)
        L = int(length[i])
        assert max(len(op) + 1, 2 * n - 1) <= L <= n * n, (u, L)
        assert moves[i, :len(op)].tolist() == op, (u, "the record does not begin with its opening")
        assert (moves[i, L:] == 0).all()
        h = position(n, [])
        for p in range(L):
            assert h.state.result == 0, (u, p)                # not over before its recorded length
            assert int(moves[i, p]) in h.state.legal_moves, (u, p)
            h.step(int(moves[i, p]))
        result = h.state.result
        assert result in (1, 3), (u, "not over at its recorded length")
        first = (u & 1) if first_mover is None else first_mover   # the agent that owns the even plies (colour X)
        winner = first if result == 3 else 1 - first
        assert outcome[i] == (1 if winner == 0 else -1), u
    assert st["games"] == n_games and st["voided"] == 0
    assert st["wins"] == [int((outcome > 0).sum()), int((outcome < 0).sum())]
    assert st["plies"] == int(length.sum()) - opened          # only the moves searched and played
    return opened


# ---- 1. records ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hash", "net"])
def test_every_record_begins_with_its_opening_and_replays_to_its_result(eng, kind):
    n, G = 7, 64
    n_games, first_game = 3 * G + 5, 6                        # refills, an odd remainder, idle slots at the end
    eng.openings_check(n, BOOK7)
    a, b = pair(eng, n, G, kind)
    m = eng.Match(a, b)
    res = m.play(n_games, first_game=first_game, moves=True, openings=BOOK7)
    check_games(res, n, n_games, first_game, BOOK7)
    assert 0 < res["stats"]["wins"][0] < n_games
    for j in range(first_game // 2, (first_game + n_games) // 2):      # 2j and 2j + 1: one opening, colours swapped
        i = 2 * j - first_game
        assert res["opening"][i] == res["opening"][i + 1] == j % len(BOOK7)
        L = len(BOOK7[j % len(BOOK7)])
        assert np.array_equal(res["moves"][i, :L], res["moves"][i + 1, :L])
        # first movers 0 and 1: the agents' colours are swapped (match_first = u & 1)
    if kind == "hash":
        fixed = m.play(G + 7, first_game=3, moves=True, first_mover=0)          # the book stays; the rule is u % n
        check_games(fixed, n, G + 7, 3, BOOK7, first_mover=0)
        assert fixed["opening"].tolist() == [(3 + i) % len(BOOK7) for i in range(G + 7)]
    m.close()
    a.close()
    b.close()


# ---- 2. the two engines driven by hand ------------------------------------------------------------------------------
def drive_by_hand_from(a, b, cfgs, n, opens, uids):
    """tests/test_gpu_match.py's drive_by_hand for games that start from `opens[slot]`: both engines are reset to the
    move prefixes, the mover comes from the parity of the slot's CURRENT ply (agent uid & 1 owns the even plies), and
    the record is prefilled with the opening."""
    G, cells = a.G, n * n
    a.reset(moves=opens)
    b.reset(moves=opens)
    first = uids & 1
    ply = np.array([len(o) for o in opens])
    alive = np.ones(G, bool)
    moves = np.zeros((G, cells), np.int16)
    for g, o in enumerate(opens):
        moves[g, :len(o)] = o
    length = np.zeros(G, np.int16)
    outcome = np.zeros(G, np.int8)
    for _ in range(cells):
        if not alive.any():
            break
        mover = first ^ (ply & 1)
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
            moves[g, ply[g]] = legal[g, ids[g]]
        ply[alive] += 1
        ga, gb = a.get_games(), b.get_games()
        assert np.array_equal(ga["board"], gb["board"]) and np.array_equal(ga["result"], gb["result"])
        done = alive & (ga["result"] != 0)
        for g in np.flatnonzero(done):
            winner = first[g] if ga["result"][g] == 3 else 1 - first[g]
            outcome[g] = 1 if winner == 0 else -1
            length[g] = ply[g]
        alive &= ~done
    assert not alive.any()
    return outcome, length, moves


@pytest.mark.parametrize("kind", ["hash", "net"])
def test_the_match_is_the_two_engines_reset_to_the_openings_and_driven_by_hand(eng, kind):
    """After Engine.reset the by-hand engines' uids are the next generation's, slot + G: the match plays the games
    first_game = G .. 2G - 1 (G is even, so the parity of u is the slot's), and the draws being equal confirms it."""
    n, G = 7, 64
    cfgs = (AGENT_A, AGENT_B)
    uids = np.arange(G) + G
    opens = [BOOK7[opening_of(int(u), BOOK7)] for u in uids]
    assert {len(o) & 1 for o in opens} == {0, 1}
    a, b = pair(eng, n, G, kind)
    outcome, length, moves = drive_by_hand_from(a, b, cfgs, n, opens, uids)
    a.close()
    b.close()
    a, b = pair(eng, n, G, kind)
    m = eng.Match(a, b)
    res = m.play(G, first_game=G, moves=True, openings=BOOK7)
    m.close()
    a.close()
    b.close()
    assert np.array_equal(res["moves"], moves)
    assert np.array_equal(res["length"], length)
    assert np.array_equal(res["outcome"], outcome)


# ---- 3. pool size ---------------------------------------------------------------------------------------------------
def play_in(eng, n, G, kind, n_games, first_game, book, **kw):
    a, b = pair(eng, n, G, kind)
    m = eng.Match(a, b)
    res = m.play(n_games, first_game=first_game, moves=True, openings=book, **kw)
    m.close()
    a.close()
    b.close()
    return res


@pytest.mark.parametrize("kind", ["hash", "net"])
def test_a_refilled_slot_and_a_slot_seeded_at_entry_hold_the_same_game(eng, kind):
    n, n_games, first_game = 5, 256, 1000
    small = play_in(eng, n, 64, kind, n_games, first_game, BOOK5)      # three of four games in a refilled slot
    large = play_in(eng, n, 256, kind, n_games, first_game, BOOK5)     # every game in a slot seeded at entry
    for k in ("outcome", "length", "moves", "opening"):
        assert np.array_equal(small[k], large[k]), k
    assert small["stats"]["plies"] == large["stats"]["plies"]
    check_games(small, n, n_games, first_game, BOOK5)


# ---- 4. tournaments -------------------------------------------------------------------------------------------------
def test_a_tournament_pair_plays_its_matchs_games_from_the_book(eng):
    n, kind, rounds, first_game = 5, "hash", 6, 4
    cfgs = (AGENT_A, AGENT_B, dict(AGENT_A, sims=20, c=1.0))
    seeds = (11, 1 << 40, 2 << 40)
    pairs = [(0, 1), (0, 2), (1, 2)]

    def engines(G):
        return [make_engine(eng, n, G, cfgs[k], seeds[k], kind) for k in range(3)]

    expect = {}
    for s, (i, j) in enumerate(pairs):
        es = engines(8)
        m = eng.Match(es[i], es[j])
        expect[(i, j)] = m.play(rounds, first_game=first_game + s * rounds, moves=True, openings=BOOK5)
        check_games(expect[(i, j)], n, rounds, first_game + s * rounds, BOOK5)
        m.close()
        for e in es:
            e.close()
    es = engines(4)
    t = eng.Tournament(es)
    out = t.play(pairs, rounds, first_game=first_game, tables_per_pair=2, moves=True, openings=BOOK5)
    for p in pairs:
        for k in ("outcome", "length", "moves", "opening"):
            assert np.array_equal(out[p][k], expect[p][k]), (p, k)
        st, ex = dict(out[p]["stats"]), dict(expect[p]["stats"])
        st.pop("seconds"), ex.pop("seconds")
        assert st == ex, p
    cleared = t.play(pairs, rounds, first_game=first_game, tables_per_pair=2, moves=True, openings=None)
    assert all("opening" not in cleared[p] for p in pairs)
    assert any(not np.array_equal(cleared[p]["moves"], out[p]["moves"]) for p in pairs)
    t.close()
    for e in es:
        e.close()


def test_evaluate_throughput_plays_the_book_pooled_or_not():
    from azalea_amd import evaluation
    n, rounds = 5, 6
    agents = tgm.device_agents(3, n=n)
    got = {}
    for pooled in (False, True):
        games = {}
        tallies = evaluation.evaluate_throughput(agents, rounds, n_slots=4, seed=5, games=games, pooled=pooled,
                                                 openings=BOOK5)
        got[pooled] = ({p: list(v) for p, v in tallies.items()}, games)
    assert got[False][0] == got[True][0]
    for s, p in enumerate(evaluation.gen_pairs(3)):
        for k in ("outcome", "length", "moves", "opening"):
            assert np.array_equal(got[False][1][p][k], got[True][1][p][k]), (p, k)
        g = got[True][1][p]
        assert g["opening"].tolist() == [opening_of(s * rounds + r, BOOK5) for r in range(rounds)]
        for r in range(rounds):
            op = BOOK5[g["opening"][r]]
            assert g["moves"][r, :len(op)].tolist() == op
    plain = {}
    evaluation.evaluate_throughput(agents, rounds, n_slots=4, seed=5, games=plain)
    assert all("opening" not in plain[p] for p in plain)
    with pytest.raises(ValueError, match="played twice"):
        evaluation.evaluate_throughput(agents, rounds, openings=[[1, 1]])


# ---- 5. harvest -----------------------------------------------------------------------------------------------------
def check_rows(res, n, first_game, book, first_mover=None):
    """tests/test_gpu_match_rows.py's check_rows for games whose rows begin at their opening's length."""
    rows, meta = res["rows"], res["row_metrics"]
    games = by_game(rows, meta)
    length, outcome, moves = res["length"], res["outcome"], res["moves"]
    assert (outcome != 0).all() and res["stats"]["voided"] == 0
    assert sorted(games) == [first_game + i for i in range(len(outcome))]
    assert len(rows["reward"]) == res["n_rows"] == res["stats"]["plies"] == len(meta)
    for i in range(len(outcome)):
        u = first_game + i
        g = games[u]
        L0 = len(book[opening_of(u, book, first_mover)])
        L = int(length[i])
        assert len(g["reward"]) == L - L0, u
        first = (u & 1) if first_mover is None else first_mover
        x_won = (0 if outcome[i] > 0 else 1) == first          # colour 1 = the agent that owns the even plies
        h = position(n, moves[i, :L0])
        for r in range(L - L0):
            p = L0 + r                                          # the ply counted from the empty board
            assert np.array_equal(g["board"][r], h.state.board), (u, p)
            k = int((h.state.board == 0).sum())
            assert g["color"][r] == (p & 1) and g["nlegal"][r] == k, (u, p)
            assert g["reward"][r] == (1.0 if x_won == (p % 2 == 0) else -1.0), (u, p)
            prob = g["moves_prob"][r]
            assert (prob[k:] == 0).all() and abs(float(prob.sum()) - 1.0) < 1e-5, (u, p)
            assert prob[int(np.searchsorted(h.state.legal_moves, moves[i, p]))] > 0, (u, p)
            assert g["metrics"][r, 3] == (1.0 if r == 0 else 0.0), (u, p)
            assert g["metrics"][r, 6] == k, (u, p)
            h.step(int(moves[i, p]))
        assert h.state.result == (3 if x_won else 1), u
    return games


@pytest.mark.parametrize("kind", ["hash", "net"])
def test_a_games_rows_begin_at_its_openings_length(eng, kind):
    n, G, n_games, first_game = 5, 16, 40, 6
    res = play_in(eng, n, G, kind, n_games, first_game, BOOK5, collect=True)
    check_games(res, n, n_games, first_game, BOOK5)
    games = check_rows(res, n, first_game, BOOK5)
    large = play_in(eng, n, 64, kind, n_games, first_game, BOOK5, collect=True)
    same_games(games, by_game(large["rows"], large["row_metrics"]))
    if kind == "hash":
        fixed = play_in(eng, n, G, kind, n_games, first_game, BOOK5, collect=True, first_mover=1)
        check_rows(fixed, n, first_game, BOOK5, first_mover=1)


def test_a_tournaments_rows_begin_at_the_openings_too(eng):
    n, kind, rounds, first_game = 5, "hash", 6, 2
    cfgs = (AGENT_A, AGENT_B, dict(AGENT_A, sims=20, c=1.0))
    pairs = [(0, 1), (0, 2), (1, 2)]
    es = [make_engine(eng, n, 4, cfgs[k], (11, 1 << 40, 2 << 40)[k], kind) for k in range(3)]
    t = eng.Tournament(es)
    out = t.play(pairs, rounds, first_game=first_game, tables_per_pair=2, moves=True, collect=True, sink=1, openings=BOOK5)
    t.close()
    for e in es:
        e.close()
    games = by_game(out["rows"], out["row_metrics"])
    assert out["n_rows"] == sum(out[p]["stats"]["plies"] for p in pairs)
    for s, p in enumerate(pairs):
        lo = first_game + s * rounds
        uid = out["rows"]["game_uid"]
        own = (uid >= lo) & (uid < lo + rounds)
        mine = {k: v[own] for k, v in out["rows"].items()}
        meta = out["row_metrics"][own]
        res = dict(out[p], rows=mine, row_metrics=meta, n_rows=len(meta))
        check_rows(res, n, lo, BOOK5)
    assert len(games) == len(pairs) * rounds


def test_the_device_player_plays_from_the_book():
    """agents[0] moves first in every game (first_mover = 0): game u starts from opening u % n."""
    from azalea_amd.parallel_player import Player
    n = 5
    player = Player(None, tgm.device_agents(2, n=n), device_match=True, n_games=16, openings=BOOK5)
    seen = []
    orig = player._harvest

    def spy(eng_, rows, st, meta=None):
        seen.append((rows, meta))
        return orig(eng_, rows, st, meta=meta)
    player._harvest = spy
    frame, metrics = player.read(150)
    player.stop()
    assert len(frame) >= 150 and metrics["game_error"] == 0
    rows, meta = seen[0]
    games = by_game(rows, meta)
    assert sorted(games) == list(range(32))                   # the first chunk: 2 * n_games games
    for u, g in games.items():
        op = BOOK5[u % len(BOOK5)]
        assert np.array_equal(g["board"][0], position(n, op).state.board), u
        assert g["color"].tolist() == [(len(op) + r) & 1 for r in range(len(g["color"]))], u
        assert g["nlegal"][0] == n * n - len(op) and g["metrics"][0, 3] == 1.0 and not g["metrics"][1:, 3].any(), u
        assert g["reward"][-1] == 1.0 and (g["reward"][::-1][::2] == 1.0).all() and (g["reward"][::-1][1::2] == -1.0).all(), u
    # the frame's games start from the openings' positions as well
    stones = [int((s.board != 0).sum()) for s in frame.state]
    assert stones[0] == len(BOOK5[int(rows["game_uid"][0]) % len(BOOK5)])


# ---- 6. nothing changes without a book ------------------------------------------------------------------------------
def test_nothing_changes_without_a_book(eng):
    n, G, n_games, first_game = 5, 16, 40, 7
    a, b = pair(eng, n, G, "hash")
    never = eng.Match(a, b)
    r0 = never.play(n_games, first_game=first_game, moves=True, collect=True)
    never.close()
    m = eng.Match(a, b)
    m.set_openings(BOOK5)
    m.set_openings(None)
    r1 = m.play(n_games, first_game=first_game, moves=True, collect=True)
    booked = m.play(n_games, first_game=first_game, moves=True, collect=True, openings=BOOK5)
    r2 = m.play(n_games, first_game=first_game, moves=True, collect=True, openings=[])      # cleared through play()
    r3 = m.play(n_games, first_game=first_game, moves=True, collect=True, openings=[[]])    # one empty opening
    m.close()
    a.close()
    b.close()
    assert "opening" not in r0 and "opening" not in r1 and "opening" not in r2
    assert r3["opening"].tolist() == [0] * n_games
    assert not np.array_equal(booked["moves"], r0["moves"])
    tgm.check_games(r0, n, n_games, first_game)
    for r in (r1, r2, r3):
        for k in ("outcome", "length", "moves"):
            assert np.array_equal(r[k], r0[k]), k
        st, s0 = dict(r["stats"]), dict(r0["stats"])
        st.pop("seconds"), s0.pop("seconds")
        assert st == s0 and r["n_rows"] == r0["n_rows"]
        same_games(by_game(r["rows"], r["row_metrics"]), by_game(r0["rows"], r0["row_metrics"]))


# ---- 7. refusals on a live handle -----------------------------------------------------------------------------------
def test_a_refused_book_leaves_the_previous_one_in_place(eng):
    n, G = 7, 16
    a, b = pair(eng, n, G, "hash")
    m = eng.Match(a, b)
    m.set_openings(BOOK7)
    decided = [1, 2, 8, 3, 15, 4, 22, 5, 29, 6, 36, 7, 43]     # X down the first column: won at ply 12
    for bad, why in (([[25], decided], r"opening 1, ply 12: move 43 decides the game for colour 1"),
                     ([[25, 18, 25]], r"opening 0, ply 2: tile 24 is played twice"),
                     ([[], [50]], r"opening 1, ply 0: move 50 outside \[1, 49\]"),
                     ([[0]], r"opening 0, ply 0: move 0 outside \[1, 49\]")):
        with pytest.raises(ValueError, match=why):
            m.set_openings(bad)
        with pytest.raises(ValueError, match=why):
            m.play(4, openings=bad)
    res = m.play(2 * G + 4, first_game=2, moves=True)         # the book set before is still the one played
    check_games(res, n, 2 * G + 4, 2, BOOK7)
    m.close()
    t = eng.Tournament([a, b])
    t.set_openings(BOOK7)
    with pytest.raises(ValueError, match="played twice"):
        t.set_openings([[3, 3]])
    out = t.play([(0, 1)], 8, first_game=2, moves=True)
    check_games(out[(0, 1)], n, 8, 2, BOOK7)
    t.close()
    a.close()
    b.close()
    # a book that is fine on 7x7 has tiles a 5x5 board lacks
    a, b = pair(eng, 5, G, "hash")
    m = eng.Match(a, b)
    with pytest.raises(ValueError, match=r"opening 3, ply 1: move 40 outside \[1, 25\]"):
        m.set_openings(BOOK7)
    res = m.play(G, moves=True)
    assert "opening" not in res
    tgm.check_games(res, 5, G)
    m.close()
    a.close()
    b.close()
