"""Resignation of device self-play with no-resign calibration games (azx_set_resign; NOT the reference's behaviour, off
by default).  Every game case plays 5x5 boards with 64 slots, 16 simulations and search batch 4, as
tests/test_gpu_playout_cap.py does.  The mirror of the per-game exemption draw is azx_resign_is_exempt, the kernels' own
function on the host (tests/test_resign_api.py holds its distribution).

A row's reward is the final result seen by the player to move at that row, so the rows of a game resigned at ply p
carry -1 where the ply has p's parity and +1 elsewhere."""
import logging
import os
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N, CELLS, G = 5, 25, 64
EINVAL = -1
MIN_PLY = 4
ROWS = 800          # rows of a calibration run: with the uniform evaluator v is 0 until the search meets a finished
                    # game, so only about one game in eight ever has v < 0; some sixty games leave five that do
ROW_KEYS = ("board", "color", "nlegal", "moves_prob", "reward", "game_uid")
KEEP_COLS = [0, 1, 2, 4, 5, 6, 7]           # every row metric but the first-row flag
STAT_KEYS = ("resigned", "played_out", "exempt", "exempt_crossed", "false_positives", "sum_resign_ply",
             "sum_plies_saved")


def make(evaluator, G=G, sims=16, bs=4, seed=4242, **kw):
    from azalea_amd import engine as eng
    cfg = dict(board_size=N, n_games=G, simulations=sims, search_batch_size=bs, exploration_coef=0.5,
               exploration_depth=4, noise_alpha=0.3, noise_scale=0.25, temperature=1.0, seed=seed)
    cfg.update(kw)
    return eng.Engine(evaluator=evaluator, **cfg)


def net_weights(blocks=1, chans=64, seed=3):
    from azalea_amd.network import HexNetwork
    torch.manual_seed(seed)
    net = HexNetwork(board_size=N, num_blocks=blocks, base_chans=chans).eval()
    return {k: v.detach().numpy() for k, v in net.state_dict().items()}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stones(board):
    return (np.asarray(board).reshape(len(board), N * N) != 0).sum(1)


def by_game(rows):
    """{uid: row indices}, each game's rows contiguous with plies ascending (asserted)."""
    uid = rows["game_uid"]
    ply = stones(rows["board"])
    out = {}
    if len(uid) == 0:
        return out
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
    for s, e in zip(starts, np.r_[starts[1:], len(uid)]):
        assert int(uid[s]) not in out                         # contiguous: a uid opens one run only
        assert (np.diff(ply[s:e]) > 0).all()
        out[int(uid[s])] = np.arange(s, e)
    return out


class Run:
    """One play call's rows, metrics and statistics."""

    def __init__(self, E, min_positions, max_plies=0):
        self.rows, self.st = E.play(min_positions, max_plies=max_plies)
        self.m = E.play_row_metrics()
        assert len(self.m) == len(self.rows["reward"])
        self.games = by_game(self.rows)
        self.ply = stones(self.rows["board"])
        self.v = self.m[:, 7]
        self.rs = E.resign_stats()
        # engine steps of the call (None where parked slots sat some of them out)
        self.steps = self.st["plies"] // E.G if self.st["plies"] % E.G == 0 else None
        for i in self.games.values():                         # metric 3 flags each game's first recorded row
            assert np.array_equal(self.m[i, 3], np.r_[1.0, np.zeros(len(i) - 1)].astype(np.float32))

    def crossing(self, uid, t):
        """Index into the game's rows of its first row with ply >= MIN_PLY and v < t, or None."""
        i = self.games[uid]
        hit = np.flatnonzero((self.ply[i] >= MIN_PLY) & (self.v[i] < np.float32(t)))
        return int(hit[0]) if len(hit) else None


def same_rows(a, ia, b, ib, reward=True):
    """Rows ia of run a equal rows ib of run b bit for bit (rewards on request)."""
    for k in ("board", "color", "nlegal", "game_uid"):
        assert np.array_equal(a.rows[k][ia], b.rows[k][ib]), k
    assert np.array_equal(bits(a.rows["moves_prob"][ia]), bits(b.rows["moves_prob"][ib]))
    assert np.array_equal(bits(a.m[ia][:, KEEP_COLS]), bits(b.m[ib][:, KEEP_COLS]))
    if reward:
        assert np.array_equal(bits(a.rows["reward"][ia]), bits(b.rows["reward"][ib]))


def resigned_rewards(ply, p_star):
    return np.where((ply & 1) == (p_star & 1), -1.0, 1.0).astype(np.float32)


def choose_threshold(P, need_both=True):
    """The median over P's games of the minimum v at plies >= MIN_PLY: about half the games then cross."""
    mins = []
    for i in P.games.values():
        late = P.v[i][P.ply[i] >= MIN_PLY]
        if len(late):
            mins.append(late.min())
    mins = np.array(mins, np.float32)
    if (mins == mins[0]).all():           # (random network weights may give one value everywhere)
        t, need_both = np.nextafter(mins[0], np.float32(2.0)), False
    else:
        t = np.float32(np.median(mins))
    cross, stay = int((mins < t).sum()), int((mins >= t).sum())
    print("threshold %r: %d of %d games cross, %d do not (min v from %r to %r)"
          % (float(t), cross, len(mins), stay, float(mins.min()), float(mins.max())))
    assert cross >= 5
    if need_both:
        assert stay >= 5
    assert -1.0 <= float(t) <= 1.0
    return float(t)


def exempt_expectation(run, uids, t):
    """(games with a crossing, false positives, plies saved) of the exempt games `uids`, from the run's own rows."""
    crossed = fp = saved = 0
    for uid in uids:
        i = run.games[uid]
        assert np.array_equal(run.ply[i], np.arange(len(i)))          # every ply recorded, from the empty board
        c = run.crossing(uid, t)
        if c is not None:
            crossed += 1
            fp += int(run.rows["reward"][i[c]] == 1.0)                # the would-be resigner went on to win
            saved += len(i) - c                                       # final length - crossing ply
    return crossed, fp, saved


def check_resigning_run(R, P, t, exempt_of, st_games):
    """Every game of R that P finished too follows P: whole if exempt or never crossing, cut after the crossing row
    otherwise.  Returns the statistics the rows of R imply."""
    want = dict.fromkeys(STAT_KEYS, 0)
    length = compared = cut = 0
    for uid, ir in R.games.items():
        ex = exempt_of(uid)
        last = ir[-1]
        gave_up = (not ex) and R.ply[last] >= MIN_PLY and R.v[last] < np.float32(t)
        if not ex:                                                    # a row that meets the rule is a game's last row
            assert not ((R.ply[ir[:-1]] >= MIN_PLY) & (R.v[ir[:-1]] < np.float32(t))).any(), uid
        if gave_up:
            want["resigned"] += 1
            want["sum_resign_ply"] += int(R.ply[last])
            length += int(R.ply[last])
            assert np.array_equal(R.rows["reward"][ir], resigned_rewards(R.ply[ir], int(R.ply[last]))), uid
        else:
            want["exempt" if ex else "played_out"] += 1
            length += len(ir)
        if uid in P.games:
            compared += 1
            ip = P.games[uid]
            c = None if ex else P.crossing(uid, t)
            if c is None:
                assert len(ir) == len(ip), uid
                same_rows(R, ir, P, ip)
                assert not gave_up
            else:
                cut += 1
                assert len(ir) == c + 1 and gave_up, (uid, len(ir), c)
                same_rows(R, ir, P, ip[:c + 1], reward=False)
    ex_uids = [u for u in R.games if exempt_of(u)]
    want["exempt_crossed"], want["false_positives"], want["sum_plies_saved"] = exempt_expectation(R, ex_uids, t)
    assert R.rs == want, (R.rs, want)
    assert st_games == len(R.games) == want["resigned"] + want["played_out"] + want["exempt"]
    assert R.st["sum_game_length"] == length
    return compared, cut


# ---- 1. the statistic ------------------------------------------------------------------------------------------------
def test_the_statistic_is_one_float32_division_of_the_roots_numbers():
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM_HASH, seed=17)
    rng = np.random.RandomState(5)
    prefixes = [[int(c) + 1 for c in rng.permutation(CELLS)[: g % 7]] for g in range(G)]
    E.reset(moves=prefixes)
    assert np.isnan(E.resign_values()).all()                           # no root is evaluated yet
    E.search()
    root = E.get_root()
    assert (root["root_visits"] > 0).all()
    want = root["root_value"].astype(np.float32) / root["root_visits"].astype(np.float32)
    got = E.resign_values()
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert len(np.unique(got)) > 8 and (np.abs(got) <= 1).all()
    E.set_resign(-0.5, 2, 0.5)                                         # whatever the setting
    assert np.array_equal(bits(E.resign_values()), bits(want))
    E.reset()
    assert np.isnan(E.resign_values()).all()
    E.close()


def test_the_statistic_is_the_movers_view():
    """3x3, uniform evaluator, 64 simulations.  Won: positions with two stones each in which the mover has a move that
    wins at once.  Lost: positions one ply on, the other side to move, in which every move leaves the opponent a move
    that wins at once.  Both are proven here with azx_advance and azx_get_games; v > 0 in the first, v < 0 in the
    second."""
    from azalea_amd import engine as eng
    n, cells = 3, 9
    E = eng.Engine(board_size=n, n_games=G, simulations=64, search_batch_size=4, exploration_coef=0.5,
                   evaluator=eng.EVAL_UNIFORM, seed=1)
    rng = np.random.RandomState(11)
    perms = [rng.permutation(cells) + 1 for _ in range(G)]

    def outcomes(prefixes, replies):
        """result[g] after prefix g and then the child indices replies[g] (a list per slot), 0 while it goes on."""
        E.reset(moves=prefixes)
        assert (E.get_games()["result"] == 0).all()
        for step in range(max(len(r) for r in replies)):
            E.advance(np.array([r[step] if step < len(r) else -1 for r in replies], np.int32))
        return E.get_games()["result"]

    # won: 4 stones, 5 legal moves, one of which ends the game
    pre4 = [[int(c) for c in p[:4]] for p in perms]
    wins = np.zeros((G, 5), bool)
    for j in range(5):
        wins[:, j] = outcomes(pre4, [[j]] * G) != 0
    won = np.flatnonzero(wins.any(1))
    assert len(won) >= 5
    E.reset(moves=pre4)
    E.search()
    v = E.resign_values()
    print("won positions:", v[won])
    assert (v[won] > 0).all()
    # lost: 5 stones (no winner yet), 4 legal moves, none of which wins, each answered by a winning move
    pre5 = [[int(c) for c in p[:5]] for p in perms]
    E.reset(moves=pre5)
    alive = E.get_games()["result"] == 0
    pre5 = [p if alive[g] else [] for g, p in enumerate(pre5)]           # (finished prefixes: play from the empty board)
    lost = alive.copy()
    for i in range(4):
        lost &= outcomes(pre5, [[i]] * G) == 0                         # the mover cannot win at once ...
        answered = np.zeros(G, bool)
        for j in range(3):
            answered |= outcomes(pre5, [[i, j]] * G) != 0              # ... and the opponent then can
        lost &= answered
    lost = np.flatnonzero(lost)
    assert len(lost) >= 3
    E.reset(moves=pre5)
    E.search()
    v = E.resign_values()
    print("lost positions:", v[lost])
    assert (v[lost] < 0).all()
    E.close()


# ---- 2. resigned games are prefixes of the played-out games ---------------------------------------------------------
@pytest.mark.parametrize("case", ["persistent", "per_move_hash", "no_persistent", "resnet"])
def test_resigned_games_are_prefixes_of_the_played_out_games(case, monkeypatch):
    from azalea_amd import engine as eng
    seed, kw, evaluator, weights = 4242, {}, eng.EVAL_UNIFORM, None
    if case == "per_move_hash":
        evaluator = eng.EVAL_UNIFORM_HASH
    elif case == "no_persistent":
        monkeypatch.setenv("AZX_NO_PERSISTENT", "1")          # (read by azx_create)
    elif case == "resnet":
        evaluator, kw, weights = eng.EVAL_RESNET, dict(num_blocks=1, base_chans=64), net_weights()

    def engine():
        E = make(evaluator, seed=seed, **kw)
        if weights is not None:
            E.set_weights(weights)
        return E
    E = engine()
    info = E.kernel_info()
    assert ("k_play<2> (persistent)" in info) == (case == "persistent"), info
    assert "resign=off" in info
    # run P: every game exempt, and v < -1 never holds
    E.set_resign(-1.0, MIN_PLY, keep_prob=1.0)
    assert "resign=-1/4/1" in E.kernel_info()
    P = Run(E, ROWS)
    E.close()
    assert P.steps is not None and len(P.rows["reward"]) >= ROWS and len(P.games) >= 10
    assert np.isfinite(P.v).all() and (np.abs(P.v) <= 1).all() and (P.v != 0).any()     # every row carries v
    assert P.rs == dict(dict.fromkeys(STAT_KEYS, 0), exempt=P.st["games"]) and P.st["games"] == len(P.games)
    t = choose_threshold(P, need_both=True)
    # run C: every game exempt at the threshold t -- the same bytes as P, and the crossings counted
    E = engine()
    E.set_resign(t, MIN_PLY, 1.0)
    Cx = Run(E, P.steps * G + 1, max_plies=P.steps)
    E.close()
    assert Cx.steps == P.steps and set(Cx.games) == set(P.games)
    for uid, i in Cx.games.items():
        same_rows(Cx, i, P, P.games[uid])
    crossed, fp, saved = exempt_expectation(P, list(P.games), t)
    assert crossed >= 5
    assert Cx.rs == dict(resigned=0, played_out=0, exempt=len(P.games), exempt_crossed=crossed, false_positives=fp,
                         sum_resign_ply=0, sum_plies_saved=saved), Cx.rs
    # run R: nobody exempt, as many engine steps
    E = engine()
    E.set_resign(t, MIN_PLY, 0.0)
    R = Run(E, P.steps * G + 1, max_plies=P.steps)
    E.close()
    assert R.steps == P.steps
    compared, cut = check_resigning_run(R, P, t, lambda uid: False, R.st["games"])
    print("%s: %d games compared, %d of them cut; stats %r" % (case, compared, cut, R.rs))
    assert compared >= 10 and cut >= 5
    assert R.rs["exempt"] == R.rs["exempt_crossed"] == R.rs["false_positives"] == R.rs["sum_plies_saved"] == 0
    assert R.rs["resigned"] + R.rs["played_out"] == R.st["games"] and R.rs["resigned"] >= 5


# ---- 3. mixed exemption, strided uids ---------------------------------------------------------------------------------
def test_mixed_exemption_follows_the_uid():
    from azalea_amd import engine as eng
    seed, kw = 777, dict(game_index_stride=3, game_index_offset=1)
    E = make(eng.EVAL_UNIFORM_HASH, seed=seed, **kw)
    E.set_resign(-1.0, MIN_PLY, 1.0)
    P = Run(E, ROWS)
    E.close()
    assert all(u % 3 == 1 for u in P.games)
    t = choose_threshold(P)
    E = make(eng.EVAL_UNIFORM_HASH, seed=seed, **kw)
    E.set_resign(t, MIN_PLY, 0.5)
    assert "resign=%.6g/4/0.5" % t in E.kernel_info()
    M = Run(E, P.steps * G + 1, max_plies=P.steps)
    E.close()
    exempt_of = lambda uid: eng.resign_is_exempt(seed, uid, 0.5)
    compared, cut = check_resigning_run(M, P, t, exempt_of, M.st["games"])
    assert compared >= 10 and cut >= 2
    assert M.rs["exempt"] >= 5 and M.rs["resigned"] >= 2 and M.rs["resigned"] + M.rs["played_out"] >= 5
    # the key is the uid, not the slot or the game's index in the pool
    uids = sorted(M.games)
    assert [exempt_of(u) for u in uids] != [eng.resign_is_exempt(seed, (u - 1) // 3, 0.5) for u in uids]


# ---- 4. parking ------------------------------------------------------------------------------------------------------
def test_resigned_games_that_find_the_queue_full_are_parked_and_handed_over():
    from azalea_amd import engine as eng
    seed = 99
    E = make(eng.EVAL_UNIFORM, seed=seed)
    E.set_resign(-1.0, MIN_PLY, 1.0)
    P = Run(E, ROWS)
    E.close()
    t = choose_threshold(P)
    E = make(eng.EVAL_UNIFORM, seed=seed)
    E.set_resign(t, MIN_PLY, 0.0)
    free = Run(E, P.steps * G + 1, max_plies=P.steps)             # the unbounded run
    E.close()
    assert free.rs["resigned"] >= 5
    E = make(eng.EVAL_UNIFORM, seed=seed)
    E.set_resign(t, MIN_PLY, 0.0)
    E.debug_set_queue_cap(24)                                     # three or four games fill it
    got, calls = {}, []
    for call in range(40):
        calls.append(Run(E, 200, max_plies=8))                    # (a call may well come back empty-handed)
        if sum(len(r.games) for r in calls) >= 24:
            break
    assert max(len(r.rows["reward"]) for r in calls) <= 24
    E.debug_set_queue_cap(0)
    calls.append(Run(E, 1, max_plies=1))                          # the slots still parked hand their games over first
    assert len(calls[-1].games) >= 3
    for r in calls:
        for uid, i in r.games.items():
            assert uid not in got
            got[uid] = (r, i)
    assert len(got) >= 27
    resigned = 0
    both = sorted(set(got) & set(free.games))
    assert len(both) >= 20
    for uid in both:
        r, i = got[uid]
        j = free.games[uid]
        assert len(i) == len(j), uid
        same_rows(r, i, free, j)
        last = j[-1]
        resigned += int(free.ply[last] >= MIN_PLY and free.v[last] < np.float32(t))
    assert resigned >= 5
    rs = E.resign_stats()
    assert rs["resigned"] + rs["played_out"] == len(got) and rs["exempt"] == 0
    E.close()


# ---- 5. with a playout cap -------------------------------------------------------------------------------------------
def test_under_a_playout_cap_recorded_rows_are_a_prefix_of_the_cap_only_run():
    from azalea_amd import engine as eng
    seed = 2024
    E = make(eng.EVAL_UNIFORM_HASH, seed=seed)
    E.set_playout_cap(0.5, 4)
    E.set_resign(-1.0, MIN_PLY, 1.0)                               # exempt everywhere: the cap-only games, with v in metric 7
    P = Run(E, ROWS)
    E.close()
    t = choose_threshold(P)
    E = make(eng.EVAL_UNIFORM_HASH, seed=seed)
    E.set_playout_cap(0.5, 4)
    E.set_resign(t, MIN_PLY, 0.0)
    info = E.kernel_info()
    assert "cap=0.5/4" in info and "resign=" in info and "resign=off" not in info
    R = Run(E, P.steps * G + 1, max_plies=P.steps)
    cap = E.playout_cap_stats()
    E.close()
    assert cap["full_plies"] + cap["fast_plies"] == R.st["plies"]
    assert R.rs["resigned"] + R.rs["played_out"] + R.rs["exempt"] == R.st["games"]
    assert R.rs["resigned"] >= 1 and R.rs["exempt"] == 0
    shorter = compared = 0
    for uid, ir in R.games.items():
        if uid not in P.games:
            continue
        compared += 1
        ip = P.games[uid]
        assert len(ir) <= len(ip), uid
        same_rows(R, ir, P, ip[:len(ir)], reward=False)
        shorter += len(ir) < len(ip)
    assert compared >= 10 and shorter >= 1
    assert R.st["games"] >= len(R.games)                          # (a game resigned before its first full ply has no row)


# ---- 6. a registered external evaluator ------------------------------------------------------------------------------
def test_a_registered_external_evaluator_resigns_at_min_ply():
    from azalea_amd import engine as eng
    inv = torch.tensor((np.float32(1.0) / np.arange(0, CELLS + 1).clip(1).astype(np.float32)).astype(np.float32),
                       device=DEV)

    def evaluate(board, legal):                                   # uniform priors, value 0
        k = (legal != 0).sum(1)
        prior = torch.where(legal != 0, inv[k][:, None], torch.zeros((), device=DEV))
        return torch.zeros(len(board), dtype=torch.float32, device=DEV), prior
    E = make(eng.EVAL_EXTERNAL, sims=8, bs=4, seed=99, noise_scale=0.0)
    E.set_external_evaluator(evaluate)
    E.set_resign(0.5, MIN_PLY, 0.0)                               # v is 0 until the search finds a win: far below +0.5
    R = Run(E, 150)
    E.close()
    assert len(R.games) >= 20
    lengths = np.array([len(i) for i in R.games.values()])
    assert (lengths == MIN_PLY + 1).all(), np.bincount(lengths)
    for uid, i in R.games.items():
        assert np.array_equal(R.ply[i], np.arange(MIN_PLY + 1))
        assert np.array_equal(R.rows["reward"][i], resigned_rewards(R.ply[i], MIN_PLY))
    assert R.rs["resigned"] == R.st["games"] == len(R.games)
    assert R.rs["sum_resign_ply"] == MIN_PLY * R.rs["resigned"] == R.st["sum_game_length"]


# ---- 7. off means off ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "hash"])
def test_resignation_never_set_or_cleared_leaves_no_trace(kind):
    from azalea_amd import engine as eng
    evaluator = eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH
    A, B, Cc = (make(evaluator, seed=11) for _ in range(3))
    B.set_resign(0.9, 0, 0.0)
    assert "resign=0.9/0/0" in B.kernel_info()
    B.clear_resign()
    out = []
    for E in (A, B, Cc):
        first = Run(E, 200)
        if E is Cc:
            E.set_resign(0.9, 0, 0.5)
            E.clear_resign()
        assert "resign=off" in E.kernel_info() and E.kernel_info() == A.kernel_info()
        second = Run(E, 200)
        out.append((first, second, E.debug_counters_raw().tobytes()))
    for other in out[1:]:
        for a, b in zip(out[0][:2], other[:2]):
            # finished games enter the harvest queue in the order the GPU finished them: compare game by game
            ia = np.argsort(a.rows["game_uid"], kind="stable")
            ib = np.argsort(b.rows["game_uid"], kind="stable")
            for k in ROW_KEYS:
                assert a.rows[k][ia].tobytes() == b.rows[k][ib].tobytes(), k
            assert a.m[ia].tobytes() == b.m[ib].tobytes()
            assert (b.m[:, 7] == 0).all() and (a.m[:, 7] == 0).all()
            for k in a.st:
                if not k.endswith("seconds"):
                    assert a.st[k] == b.st[k], k
        assert out[0][2] == other[2]
    assert A.resign_stats() == dict.fromkeys(STAT_KEYS, 0)
    for E in (A, B, Cc):
        E.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_einval_and_change_nothing():
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM, seed=1)
    L = E.L
    E.set_resign(-0.9, 10, 0.1)
    said = "resign=-0.9/10/0.1"
    assert said in E.kernel_info()
    nan, inf = float("nan"), float("inf")
    for thr, ply, keep, word in ((-1.5, 4, 0.1, b"threshold"), (1.0001, 4, 0.1, b"threshold"), (nan, 4, 0.1, b"threshold"),
                                 (inf, 4, 0.1, b"threshold"), (-inf, 4, 0.1, b"threshold"), (-0.5, -1, 0.1, b"min_ply"),
                                 (-0.5, 4, -0.1, b"keep_prob"), (-0.5, 4, 1.5, b"keep_prob"), (-0.5, 4, nan, b"keep_prob"),
                                 (-0.5, 4, inf, b"keep_prob")):
        assert L.azx_set_resign(E.h, thr, ply, keep) == EINVAL, (thr, ply, keep)
        assert word in L.azx_last_error(), (thr, ply, keep, L.azx_last_error())
        assert said in E.kernel_info()                        # the previous setting is left in place
    with pytest.raises(ValueError, match="threshold"):
        E.set_resign(-2.0)
    assert L.azx_resign_stats(E.h, None) == EINVAL and L.azx_resign_value(E.h, None) == EINVAL
    for thr, ply, keep in ((-1.0, 0, 0.0), (1.0, 0, 1.0), (0.0, 10 ** 6, 0.5)):   # the corners are accepted
        E.set_resign(thr, ply, keep)
    E.close()


def test_matches_and_tournaments_refuse_a_resigning_engine_before_touching_any():
    from azalea_amd import engine as eng
    from azalea_amd._lib import AzxError
    a, b = make(eng.EVAL_UNIFORM_HASH, seed=6), make(eng.EVAL_UNIFORM_HASH, seed=7)
    for e in (a, b):
        e.play(40)                                            # rows in both harvest queues, games under way in the slots
    m, t = eng.Match(a, b), eng.Tournament([a, b])

    def state():
        out = []
        for e in (a, b):
            g = e.get_games()
            n = e._last_rows
            out.append((g["board"].tobytes(), g["ply"].tobytes(), e.get_root()["root_visits"].tobytes(),
                        {k: v.tobytes() for k, v in e.rows_read(0, n).items()}))
        return out
    before = state()
    b.set_resign(-0.9, 4, 0.1)
    with pytest.raises(AzxError, match=r"azx error -1: engine b has resignation set"):
        m.play(4)
    with pytest.raises(AzxError, match=r"azx error -1: engine 1 has resignation set"):
        t.play([(0, 1)], 4)
    assert state() == before                                  # both engines' slots and queues are as they were
    b.clear_resign()
    a.set_resign(-0.9, 4, 0.1)
    with pytest.raises(AzxError, match=r"azx error -1: engine a has resignation set"):
        m.play(4)
    with pytest.raises(AzxError, match=r"azx error -1: engine 0 has resignation set"):
        t.play([(0, 1)], 4)
    assert state() == before
    a.clear_resign()
    res = m.play(8)                                           # after clearing, it plays
    assert (res["outcome"] != 0).all() and (res["length"] >= 9).all()
    m.close()
    t.close()
    a.close()
    b.close()


def test_search_and_advance_never_resign():
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM_HASH, seed=5)
    E.set_resign(1.0, 0, 0.0)                                 # every judged ply would resign
    E.reset()
    for ply in range(3):
        E.search()
        E.advance(np.zeros(G, np.int32))
    g = E.get_games()
    assert (g["ply"] == 3).all() and (g["result"] == 0).all()
    assert E.resign_stats() == dict.fromkeys(STAT_KEYS, 0)
    E.close()


# ---- 9. the Python surface -------------------------------------------------------------------------------------------
SEARCH = dict(simulations=20, search_batch_size=5, exploration_coef=1.0, exploration_depth=4,
              exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0)
RESIGN = (0.0, 2, 0.25)                                           # a random network's values sit near 0: about half the plies


def cuda_policy():
    from azalea_amd.policy import Policy
    torch.manual_seed(1)
    policy = Policy()
    policy.initialize(dict(device="cuda:0", network="HexNetwork", board_size=N, num_blocks=1, base_chans=16, seed=1,
                           **SEARCH))
    return policy


def test_player_resigns_and_counts():
    from azalea_amd import parallel_player
    from azalea_amd.azalea_agent import AzaleaAgent
    from azalea_amd.game.hex import HexGame
    from azalea_amd import engine as eng
    agent = AzaleaAgent(partial(HexGame, board_size=N), policy=cuda_policy(), device="cuda:0")
    # AzaleaAgent() seeds its policy from the operating system (azalea_agent.py:41-44), and the Player draws the
    # engine's seed from the policy: without this line every run plays other games with other exempt ones
    agent.seed(1)
    player = parallel_player.Player(None, [agent], n_games=G, resign=RESIGN)
    assert player.resign_stats() is None
    # An exempt game plays to the end while its neighbours resign: a read of 200 rows returns after some twelve engine
    # steps, most often before any exempt game is over.  A step hands over at most G rows and a 5x5 game is over after
    # CELLS plies, so G * CELLS rows take at least CELLS steps: every slot's first game, the exempt ones included, is
    # finished and counted by then.
    frame, metrics = player.read(G * CELLS)
    assert len(frame) >= G * CELLS
    assert "resign=0/2/0.25" in player._engine.kernel_info()
    rs = player.resign_stats()
    exempt_first = sum(eng.resign_is_exempt(player._engine.cfg.seed, uid, RESIGN[2]) for uid in range(G))
    assert exempt_first > 0                                     # a condition on the input: the seed above meets it
    # (the engine may have finished more games than this read handed out)
    assert rs["resigned"] + rs["played_out"] + rs["exempt"] >= metrics["games"] > 0
    assert rs["resigned"] > 0 and rs["exempt"] >= exempt_first and rs["sum_resign_ply"] >= 2 * rs["resigned"]
    player.stop()


class Lines(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_a_two_step_train_runs_with_resignation(tmp_path, monkeypatch):
    from azalea_amd.parallel_player import Player
    from azalea_amd.policy_trainer import train
    config = dict(seed=1, device="cuda:0", game="azalea_amd.game.hex.HexGame", board_size=N, replaybuf_size=256,
                  replaybuf_oversampling=1.0, batch_size=64, lr_initial=0.05, lr_decay=0.1, lr_decay_epochs=1,
                  momentum=0.9, l2_regularization=1e-4, total_epochs=2, selfplay_games=64, log_interval=1,
                  model_checkpoint_interval=0, resign=dict(threshold=RESIGN[0], min_ply=RESIGN[1], keep_prob=RESIGN[2]))
    log = Lines()
    root = logging.getLogger()
    level = root.level
    root.addHandler(log)
    root.setLevel(logging.INFO)
    infos, players = [], []
    stop = Player.stop

    def stop_and_tell(player):                  # train() stops its players at the end: ask their engines first
        players.append(player.resign)
        if player.resign is not None:           # (not the random-mover player that fills the first buffer)
            infos.append((player.device_engine().kernel_info(), player.resign_stats()))
        stop(player)
    monkeypatch.setattr(Player, "stop", stop_and_tell)
    try:
        path = train(cuda_policy(), config, str(tmp_path))
    finally:
        root.removeHandler(log)
        root.setLevel(level)
    assert os.path.exists(path)
    assert players.count(None) >= 1 and players.count(RESIGN) == 1, players
    assert len(infos) == 1 and "resign=0/2/0.25" in infos[0][0], infos
    rs = infos[0][1]
    assert rs["resigned"] > 0 and rs["resigned"] + rs["played_out"] + rs["exempt"] > rs["resigned"]
    said = [l for l in log.lines if "config['resign']" in l]
    assert len(said) == 1 and "NOT the reference's behaviour" in said[0] and "0.25" in said[0], said
    refills = [l for l in log.lines if l.startswith("resign: false-positive rate")]
    assert len(refills) >= 1 and "games resigned" in refills[-1], log.lines
