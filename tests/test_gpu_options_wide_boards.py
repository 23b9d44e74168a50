"""The self-play options (forced playouts and pruning, early stop, playout cap, resignation, training targets) on 9x9 to
13x13 boards, where a root spans two or three 64-lane words of children and 12x12 / 13x13 run the three-word kernels
(k_play<3>, k_mcts<3,FAST>, k_mcts<3,generic>).  Every exact test of these options elsewhere plays 5x5: one word, so
each "across words" loop of the options' code runs once there.  The references are those of the 5x5 tests, taking the
board as a parameter: tests/forced_playouts_reference.py (the numpy restatement of the oracle's search with the forcing
rule, and the prune) and tests/early_stop_reference.py (the unmodified oracle batch by batch), on the position families
of tests/option_positions.py, whose conditions tests/test_options_wide_boards_api.py asserts on the CPU.

One ply of a set is at most 128 slots.  first_rows() ends every game right after its first ply by resignation at
threshold 1 (every judged ply resigns), so the harvest hands the first ply's row over without 160 more searches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import early_stop_reference as es  # noqa: E402
import forced_playouts_reference as fp  # noqa: E402
import option_positions as op  # noqa: E402
import train_targets_reference as tt  # noqa: E402
from test_gpu_early_stop import bits, selects, stones  # noqa: E402
from test_gpu_forced_playouts import check_decided, raw_sum, sorted_rows  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
K = op.K_FORCED
ROW_KEYS = ("board", "color", "nlegal", "moves_prob", "reward", "game_uid")
PATHS = ["persistent", "no_persistent", "generic"]
# every board with "uniform" on each of the three inline paths and with "hash" on the generic kernel
CASES = ([(n, "uniform", path) for n in op.BOARDS for path in PATHS] + [(n, "hash", "generic") for n in op.BOARDS]
         + [(n, "hash_wider", "generic") for n in op.WIDER_BOARDS])
STOP_CASES = [(n, "uniform", path) for n in op.BOARDS for path in PATHS] + [(n, "hash", "generic") for n in op.BOARDS]
ZERO_FP = dict.fromkeys(("full_plies", "forced_selects", "rows_pruned", "visits_removed"), 0)
ZERO_ES = dict.fromkeys(("t0_plies", "stopped_plies", "batches_skipped"), 0)


def make(evaluator, G, cfg, seed=4242, **kw):
    from azalea_amd import engine as eng
    c = dict(board_size=cfg.n, n_games=G, simulations=cfg.sims, search_batch_size=cfg.bs, exploration_coef=cfg.c_puct,
             exploration_depth=0, noise_alpha=0.3, noise_scale=0.0, temperature=1.0, seed=seed)
    c.update(kw)
    return eng.Engine(evaluator=evaluator, **c)


def engine_on_path(kind, path, monkeypatch, G, cfg, **kw):
    """An engine of `kind` ("uniform": the inline evaluator's three paths; "hash...": values leave the wave, so the tree
    kernel is the generic one) created under the diagnostic switch of `path`; the instantiation kernel_info names is
    the two-word one up to 11x11 and the three-word one on 12x12 and 13x13."""
    from azalea_amd import engine as eng
    if path == "no_persistent":
        monkeypatch.setenv("AZX_NO_PERSISTENT", "1")          # (read by azx_create)
    elif path == "generic":
        monkeypatch.setenv("AZX_MCTS_GENERIC", "1")
    S = 2 if cfg.cells <= 128 else 3
    E = make(eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH, G, cfg, **kw)
    if kind != "uniform":
        E.set_prior_table(cfg.table)
        assert path == "generic" and "tree=k_mcts<%d,generic>" % S in E.kernel_info(), E.kernel_info()
    else:
        info = E.kernel_info()
        assert ("k_play<%d> (persistent)" % S in info) == (path == "persistent"), info
        assert ("tree=k_mcts<%d,FAST" % S in info) == (path != "generic"), info
        assert ("tree=k_mcts<%d,generic>" % S in info) == (path == "generic"), info
    return E


def first_rows(E, prefixes, cfg):
    """Reset the slots to the prefixes and play one ply (the statistics are read there); then resignation at threshold
    1 ends every game at its next ply, so that the harvest hands over the row the first ply recorded.  Returns (per
    slot: that row's moves_prob and metrics, azx_forced_playouts_stats after the one ply)."""
    G = len(prefixes)
    E.reset(moves=[list(p) for p in prefixes])
    never = 4 * G * cfg.cells                                   # more rows than these plies can record: max_plies ends the calls
    parts = []
    rows, _ = E.play(never, max_plies=1)
    parts.append((rows, E.play_row_metrics()))
    stats = E.forced_playouts_stats()
    E.set_resign(1.0, 0, 0.0)                                   # v < 1 at every judged ply, no game exempt
    rows, _ = E.play(never, max_plies=1)
    parts.append((rows, E.play_row_metrics()))
    E.clear_resign()
    rows = {k: np.concatenate([p[0][k] for p in parts]) for k in ROW_KEYS}
    m = np.concatenate([p[1] for p in parts])
    assert len(m) == len(rows["reward"])
    out = []
    for g, prefix in enumerate(prefixes):
        mine = np.flatnonzero(rows["game_uid"] % G == g)
        mine = mine[rows["game_uid"][mine] == rows["game_uid"][mine].min()]      # the slot's first game: the prefix's
        r = mine[np.argmin(stones(rows["board"][mine]))]
        assert np.array_equal(rows["board"][r], es.game_at(prefix, cfg).board), (g, prefix)
        assert rows["nlegal"][r] == cfg.cells - len(prefix)
        out.append((rows["moves_prob"][r], m[r][:7]))
    return out, stats


# ---- 1. forced selects and pruning: one ply of every position, exact -----------------------------------------------------
@pytest.mark.parametrize("n,kind,path", CASES)
def test_one_ply_of_every_position_forces_where_the_restatement_does(n, kind, path, monkeypatch):
    cfg, refs = op.forced_set(n, kind)
    E = engine_on_path(kind, path, monkeypatch, len(refs), cfg)
    assert "forced=off" in E.kernel_info()
    E.set_train_targets("visits")
    E.set_forced_playouts(K, False)
    assert "forced=2/noprune" in E.kernel_info() and E.forced_playouts() == (2.0, False)
    got, stats = first_rows(E, [r["prefix"] for r in refs], cfg)
    E.close()
    for (row, m), r in zip(got, refs):
        k = len(r["n"])
        S = raw_sum(m)
        assert S == int(r["n"].sum()), (r["prefix"], S)
        assert np.array_equal(np.rint(row[:k].astype(np.float64) * S), r["n"]), (r["prefix"], row[:k] * S, r["n"])
        assert np.array_equal(bits(row[:k]), bits(fp.shares(r["n"]))) and (row[k:] == 0).all(), r["prefix"]
        assert m[1] == (r["n"] > 0).sum()
    print(n, kind, path, "forced selects", stats["forced_selects"])
    assert stats == dict(full_plies=len(refs), forced_selects=sum(r["forced"] for r in refs), rows_pruned=0,
                         visits_removed=0)


@pytest.mark.parametrize("n,kind,path", CASES)
def test_one_ply_of_every_position_prunes_what_the_restatement_prunes(n, kind, path, monkeypatch):
    cfg, refs = op.forced_set(n, kind)
    E = engine_on_path(kind, path, monkeypatch, len(refs), cfg)
    E.set_train_targets("visits")
    E.set_forced_playouts(K, True)
    assert "forced=2/prune" in E.kernel_info() and E.forced_playouts() == (2.0, True)
    got, stats = first_rows(E, [r["prefix"] for r in refs], cfg)
    E.close()
    for (row, m), r in zip(got, refs):                          # no position is dropped: IEEE arithmetic on both sides
        k = len(r["n"])
        assert np.array_equal(bits(row[:k]), bits(fp.shares(r["r"]))) and (row[k:] == 0).all(), (r["prefix"], row[:k], r["r"])
        # the row's metrics stay on the raw counts
        assert raw_sum(m) == int(r["n"].sum()) and m[1] == (r["n"] > 0).sum(), r["prefix"]
    print(n, kind, path, stats)
    assert stats == dict(full_plies=len(refs), forced_selects=sum(r["forced"] for r in refs),
                         rows_pruned=sum(r["removed"] > 0 for r in refs), visits_removed=sum(r["removed"] for r in refs))


# ---- 2. early stop: one ply of every position against the oracle ---------------------------------------------------------
def one_ply(E, prefixes, cfg):
    """reset to the prefixes, play one ply: (selects of the ply per slot, games after, roots after, play statistics,
    {slot: the row a game that ended with this ply handed over})."""
    G = len(prefixes)
    E.reset(moves=[list(p) for p in prefixes])
    before = selects(E)
    rows, st = E.play(4 * G * cfg.cells, max_plies=1)
    ended = {}
    for i, uid in enumerate(rows["game_uid"]):
        g = int(uid) % G
        assert g not in ended                                   # one ply: one row of the slot's game at the most
        ended[g] = (rows["moves_prob"][i], int(rows["nlegal"][i]), rows["board"][i])
    return selects(E) - before, E.get_games(), E.get_root(), st, ended


def check_against_oracle(refs, cfg, sel, games, root, ended, key_b, key_leader, key_root):
    """Per slot: the ply's select count; where the move does not end the game the stone placed and the carried root,
    bit for bit; where it does, the recorded (greedy) row is one-hot at the reference's leader."""
    for g, r in enumerate(refs):
        b = r[key_b] if key_b else cfg.nb
        assert sel[g] == b * cfg.bs, (g, r["prefix"], sel[g], b)
        h = es.game_at(r["prefix"], cfg)
        before = h.board
        leader = r[key_leader]
        tile = int(h.legal_moves()[leader])
        h.step(tile)
        k0 = cfg.cells - len(r["prefix"])
        if h.result:
            row, k, board = ended[g]
            want = np.zeros(cfg.cells, np.float32)
            want[leader] = 1.0
            assert k == k0 and np.array_equal(board, before) and np.array_equal(bits(row), bits(want)), (g, r["prefix"], leader)
            continue
        assert g not in ended
        assert np.array_equal(games["board"][g], h.board), (g, r["prefix"], tile)
        nv, tv, rv, rw = r[key_root]
        k = int(root["k"][g])
        assert k == k0 - 1
        want_nv, want_tv = np.zeros(k, np.float32), np.zeros(k, np.float32)
        want_nv[:len(nv)], want_tv[:len(tv)] = nv, tv          # (an unexpanded new root has no children yet)
        assert np.array_equal(bits(root["child_visits"][g, :k]), bits(want_nv)), (g, r["prefix"])
        assert np.array_equal(bits(root["child_value"][g, :k]), bits(want_tv)), (g, r["prefix"])
        assert bits(root["root_visits"][g:g + 1])[0] == bits([rv])[0] and bits(root["root_value"][g:g + 1])[0] == bits([rw])[0]


@pytest.mark.parametrize("n,kind,path", STOP_CASES)
def test_one_ply_of_every_position_stops_where_the_oracle_rule_does(n, kind, path, monkeypatch):
    cfg, refs = op.stop_set(n, kind)
    prefixes = [r["prefix"] for r in refs]
    E = engine_on_path(kind, path, monkeypatch, len(refs), cfg)
    assert "estop=off" in E.kernel_info()
    E.set_early_stop(True)
    assert "estop=on" in E.kernel_info() and "cap=off" in E.kernel_info() and "resign=off" in E.kernel_info()
    sel, games, root, st, ended = one_ply(E, prefixes, cfg)
    print(n, kind, path, "selects per slot under the option:", sel.tolist())
    check_against_oracle(refs, cfg, sel, games, root, ended, "b_star", "leader", "stop_root")
    want = es.counts_of(refs, cfg)
    assert E.early_stop_stats() == want and want["stopped_plies"] >= 3
    assert st["selects"] == sel.sum() == cfg.bs * (cfg.nb * len(refs) - want["batches_skipped"])
    # control: the same engine with the option off runs every batch and carries the full search's subtree
    E.set_early_stop(False)
    assert "estop=off" in E.kernel_info()
    sel, games, root, st, ended = one_ply(E, prefixes, cfg)
    assert (sel == cfg.nb * cfg.bs).all()
    check_against_oracle(refs, cfg, sel, games, root, ended, None, "full_leader", "full_root")
    assert E.early_stop_stats() == ZERO_ES
    E.close()


# ---- 3. whole games ------------------------------------------------------------------------------------------------------
def check_games(rows, cfg, every_ply=True):
    """Every game's rows: contiguous, from the empty board, plies ascending (one row per ply with `every_ply`; under a
    playout cap the fast plies record none); a valid distribution each (non-negative, zero beyond k, sum 1 within
    1e-6); each board holds the stones of the row before it, the colours alternate and no recorded position is
    decided; with `every_ply` each row gives positive probability to the move the next row's board shows and the game
    replays as a legal game under the oracle's rules.  Returns the number of games."""
    from oracle import oracle as orc
    uid, ply = rows["game_uid"], stones(rows["board"])
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
    seen = set()
    for s, e in zip(starts, np.r_[starts[1:], len(uid)]):
        assert int(uid[s]) not in seen
        seen.add(int(uid[s]))
        if every_ply:
            assert np.array_equal(ply[s:e], np.arange(e - s))
        else:
            assert (np.diff(ply[s:e]) > 0).all()
        h = es.game_at([], cfg)
        for r in range(s, e):
            k = int(rows["nlegal"][r])
            p = rows["moves_prob"][r]
            board = rows["board"][r]
            assert (p >= 0).all() and (p[k:] == 0).all() and abs(float(p[:k].astype(np.float64).sum()) - 1.0) <= 1e-6, (r, p)
            assert k == cfg.cells - ply[r] and rows["color"][r] == ply[r] % 2
            assert (board == 1).sum() == (ply[r] + 1) // 2 and (board == 2).sum() == ply[r] // 2
            if r > s:
                prev = rows["board"][r - 1]
                assert (board[prev != 0] == prev[prev != 0]).all()
            if not every_ply:                                   # no stone on it has won: an unfinished position
                assert not any(orc.check_win(board, int(c) + 1) for c in np.flatnonzero(board.ravel() != 0)), r
                continue
            assert h.result == 0 and np.array_equal(h.board, board)
            legal = h.legal_moves()
            assert len(legal) == k
            if r + 1 < e:
                new = np.flatnonzero((rows["board"][r + 1] != board).ravel())
                assert len(new) == 1
                tile = int(new[0]) + 1
                assert p[int(np.flatnonzero(legal == tile)[0])] > 0, (r, tile, p[:k])
                h.step(tile)
    return len(starts)


@pytest.mark.parametrize("n", [13, 11])
def test_the_draw_uses_the_pruned_counts(n):
    from azalea_amd import engine as eng
    cfg = es.Settings(n=n, sims=60, bs=10, c_puct=0.5)
    E = make(eng.EVAL_UNIFORM_HASH, 32, cfg, seed=5, exploration_depth=cfg.cells, noise_scale=0.25)    # T = 1 at every ply
    E.set_prior_table(cfg.table)
    E.set_forced_playouts(K, True)
    rows, st = E.play(300)
    m = E.play_row_metrics()
    stats = E.forced_playouts_stats()
    E.close()
    assert st["games"] >= 2 and len(rows["reward"]) >= 300
    assert check_games(rows, cfg) == st["games"]
    check_decided(rows)
    assert (rows["nlegal"] > 128).any() if n == 13 else (rows["nlegal"] > 64).any()
    # the rows are the pruned distribution: some visited children (the raw width, metric 1) have no weight in them
    support = (rows["moves_prob"] > 0).sum(1)
    assert (support <= m[:, 1]).all() and (support < m[:, 1]).any()
    print("%dx%d: rows %d, of those with a child pruned to nothing %d; statistics %s"
          % (n, n, len(support), (support < m[:, 1]).sum(), stats))
    assert stats["rows_pruned"] >= (support < m[:, 1]).sum() > 0 and stats["visits_removed"] >= stats["rows_pruned"]
    assert stats["forced_selects"] > 0 and stats["full_plies"] == st["plies"]
    # metric 2 is the log-probability of the drawn move under the pruned distribution
    uid = rows["game_uid"]
    for r in np.flatnonzero(uid[1:] == uid[:-1])[:300]:
        new = np.flatnonzero((rows["board"][r + 1] != rows["board"][r]).ravel())
        h = es.game_at([], cfg)
        h.set_board(rows["board"][r], 1 + int(rows["color"][r]))
        idx = int(np.flatnonzero(h.legal_moves() == int(new[0]) + 1)[0])
        assert abs(float(m[r, 2]) - np.log(float(rows["moves_prob"][r][idx]))) <= 1e-4


ALL_SIMS, ALL_FAST, ALL_P, ALL_MIX, ALL_DEPTH = 60, 20, 0.5, 0.5, 4
ALL_RESIGN = (0.0, 4, 0.25)                                     # hash values sit around 0: many judged plies resign


def set_all(E):
    E.set_playout_cap(ALL_P, ALL_FAST)
    E.set_forced_playouts(K, True)
    E.set_early_stop(True)
    E.set_resign(*ALL_RESIGN)
    E.set_train_targets("visits", ALL_MIX)


def clear_all(E):
    E.clear_playout_cap()
    E.clear_forced_playouts()
    E.set_early_stop(False)
    E.clear_resign()
    E.clear_train_targets()


@pytest.mark.parametrize("n", [13, 11])
def test_all_five_options_together(n):
    from azalea_amd import engine as eng
    cfg = es.Settings(n=n, sims=ALL_SIMS, bs=10, c_puct=0.5)
    nb_full, nb_fast = ALL_SIMS // cfg.bs + 1, ALL_FAST // cfg.bs + 1
    out = []
    for _ in range(2):
        E = make(eng.EVAL_UNIFORM_HASH, 64, cfg, seed=8, exploration_depth=ALL_DEPTH, noise_scale=0.25)
        E.set_prior_table(cfg.table)
        set_all(E)
        info = E.kernel_info()
        assert all(s in info for s in ("cap=0.5/20", "estop=on", "forced=2/prune")) and "resign=off" not in info and "targets=off" not in info, info
        rows, st = E.play(400)
        m = E.play_row_metrics()
        cap, fps, ess, rs, tts = (E.playout_cap_stats(), E.forced_playouts_stats(), E.early_stop_stats(), E.resign_stats(),
                                  E.train_targets_stats())
        E.close()
        out.append((sorted_rows(rows, m), cap, fps, ess, rs, tts, {k: v for k, v in st.items() if not k.endswith("seconds")}))
    assert out[0] == out[1]                                     # the same seed gives the same bytes
    print("%dx%d: %s %s %s %s %s" % (n, n, cap, fps, ess, rs, tts))
    # legal prefix-consistent chains (the fast plies record no row)
    games = check_games(rows, cfg, every_ply=False)
    assert games == st["games"] - cap["empty_games"] > 0 and len(rows["reward"]) >= 400
    assert (rows["nlegal"] > (128 if n == 13 else 64)).any()
    # the reward is the blend of the game's outcome z, one sign per game, and the root's value (metric 7)
    uid = rows["game_uid"]
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
    v = m[:, 7]
    assert np.isfinite(v).all() and (np.abs(v) <= 1).all()
    blended = 0
    for s, e in zip(starts, np.r_[starts[1:], len(uid)]):
        first = np.where(rows["color"][s:e] == 0, 1.0, -1.0).astype(np.float32)
        got = bits(rows["reward"][s:e])
        fits = [np.array_equal(got, bits(tt.blend(z, v[s:e], ALL_MIX))) for z in (first, -first)]
        assert any(fits), (int(uid[s]), rows["reward"][s:e], v[s:e])
        blended += int((rows["reward"][s:e] != first).any() and (rows["reward"][s:e] != -first).any())
    assert blended > 0
    # the statistics add up
    assert cap["full_plies"] + cap["fast_plies"] == st["plies"] and cap["full_plies"] > 0 and cap["fast_plies"] > 0
    assert fps["full_plies"] == cap["full_plies"] and 0 < fps["forced_selects"] <= cfg.bs * nb_full * cap["full_plies"]
    assert fps["rows_pruned"] > 0 and fps["visits_removed"] >= fps["rows_pruned"]
    assert ess["stopped_plies"] > 0 and ess["batches_skipped"] >= ess["stopped_plies"] and ess["t0_plies"] <= st["plies"]
    assert st["selects"] == cfg.bs * (nb_full * cap["full_plies"] + nb_fast * cap["fast_plies"] - ess["batches_skipped"])
    assert rs["resigned"] > 0 and rs["resigned"] + rs["played_out"] + rs["exempt"] == st["games"]
    assert tts["rows"] >= len(rows["reward"]) and tts["greedy_rows"] > 0


def test_the_options_never_set_or_set_and_cleared_leave_no_trace():
    from azalea_amd import engine as eng
    cfg = es.Settings(n=13, sims=40, bs=4, c_puct=0.5)
    out, infos = [], []
    for cleared in (False, True):
        E = make(eng.EVAL_UNIFORM_HASH, 32, cfg, seed=11, exploration_depth=2, noise_scale=0.25)
        E.set_prior_table(cfg.table)
        if cleared:
            set_all(E)
            assert "forced=2/prune" in E.kernel_info() and "estop=on" in E.kernel_info()
            clear_all(E)
        infos.append(E.kernel_info())
        rows, st = E.play(200)
        out.append((sorted_rows(rows, E.play_row_metrics()), {k: v for k, v in st.items() if not k.endswith("seconds")},
                    E.debug_counters_raw().tobytes(), E.debug_counters().tobytes()))
        assert E.forced_playouts_stats() == ZERO_FP and E.early_stop_stats() == ZERO_ES
        assert E.forced_playouts() == (0.0, False) and E.train_targets() == ("reference", 0.0)
        assert (rows["nlegal"] > 128).any() and st["games"] > 0
        E.close()
    assert out[0] == out[1]
    assert all(s in infos[0] for s in ("cap=off", "resign=off", "estop=off", "targets=off", "forced=off")) and infos[0] == infos[1]


# ---- 4. the resign statistic -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [13, 11])
def test_the_resign_statistic_is_one_float32_division_of_the_roots_numbers(n):
    from azalea_amd import engine as eng
    G = 64
    cfg = es.Settings(n=n, sims=16, bs=4, c_puct=0.5)
    E = make(eng.EVAL_UNIFORM_HASH, G, cfg, seed=17, exploration_depth=4, noise_scale=0.25)
    rng = np.random.RandomState(5)
    # mid-game prefixes of 10 to 32 plies: k > 128 on 13x13, k > 64 on 11x11
    prefixes = [list(op.random_prefix(rng, cfg, 10 + g % 23)) for g in range(G)]
    E.reset(moves=prefixes)
    assert np.isnan(E.resign_values()).all()                           # no root is evaluated yet
    E.search()
    root = E.get_root()
    assert (root["root_visits"] > 0).all() and (root["k"] > (128 if n == 13 else 64)).all()
    want = root["root_value"].astype(np.float32) / root["root_visits"].astype(np.float32)
    got = E.resign_values()
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert len(np.unique(got)) > 8 and (np.abs(got) <= 1).all()
    E.set_resign(-0.5, 2, 0.5)                                         # whatever the setting
    assert np.array_equal(bits(E.resign_values()), bits(want))
    E.reset()
    assert np.isnan(E.resign_values()).all()
    E.close()


# ---- 5. beyond the sqrt table ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["persistent", "generic"])
def test_a_root_whose_visit_sum_passes_the_sqrt_table(path, monkeypatch):
    """5x5 at 4600 simulations: past a visit sum of 4096 (AZX_SQRT_TAB) the select takes sqrtf in place of the table,
    and the forcing rule's S = (float)sum is that large.  Rule off: root counts and values of azx_search against the
    oracle (the restatement's off_* are the oracle's, tests/test_options_wide_boards_api.py).  Forcing on: counts, row
    and statistics of one ply against the restatement."""
    cfg, refs = op.LONG, op.long_refs()
    prefixes = [r["prefix"] for r in refs]
    E = engine_on_path("uniform", path, monkeypatch, len(refs), cfg)
    E.reset(moves=prefixes)
    E.search()
    root = E.get_root()
    for g, r in enumerate(refs):
        k = len(r["off_n"])
        assert root["k"][g] == k and r["off_n"].sum() > 4096
        assert np.array_equal(bits(root["child_visits"][g, :k]), bits(r["off_n"])), r["prefix"]
        assert np.array_equal(bits(root["child_value"][g, :k]), bits(r["off_w"])), r["prefix"]
    E.set_train_targets("visits")
    E.set_forced_playouts(K, False)
    got, stats = first_rows(E, prefixes, cfg)
    E.close()
    for (row, m), r in zip(got, refs):
        k = len(r["n"])
        S = raw_sum(m)
        assert S == int(r["n"].sum()) > 4096, (r["prefix"], S)
        assert np.array_equal(np.rint(row[:k].astype(np.float64) * S), r["n"]), (r["prefix"], row[:k] * S, r["n"])
        assert np.array_equal(bits(row[:k]), bits(fp.shares(r["n"]))) and (row[k:] == 0).all(), r["prefix"]
    assert stats == dict(full_plies=len(refs), forced_selects=sum(r["forced"] for r in refs), rows_pruned=0, visits_removed=0)
