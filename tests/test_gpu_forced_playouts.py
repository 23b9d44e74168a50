"""Forced playouts at the root and policy target pruning (azx_set_forced_playouts; NOT the reference's behaviour, off
by default) on the device.  The rule's reference is tests/forced_playouts_reference.py: a numpy float32 restatement of
the oracle's search with the rule as a parameter, pinned to the unmodified oracle with the rule off
(tests/test_forced_playouts_api.py).  Every case plays 5x5 boards, one slot per reference position."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forced_playouts_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N, CELLS, NB, BS, K = ref.N, ref.CELLS, ref.NB, ref.BS, ref.K_FORCED
EINVAL = -1
ROW_KEYS = ("board", "color", "nlegal", "moves_prob", "reward", "game_uid")
CTR_SELECTS, CTR_PLIES, CTR_CAP_FULL, CTR_CAP_FAST = 0, 8, 13, 14
STAT_KEYS = ("full_plies", "forced_selects", "rows_pruned", "visits_removed")
ZERO_STATS = dict.fromkeys(STAT_KEYS, 0)
PATHS = ["persistent", "no_persistent", "generic"]


def make(evaluator, G, sims=ref.SIMS, bs=BS, seed=4242, **kw):
    from azalea_amd import engine as eng
    cfg = dict(board_size=N, n_games=G, simulations=sims, search_batch_size=bs, exploration_coef=ref.C_PUCT,
               exploration_depth=0, noise_alpha=0.3, noise_scale=0.0, temperature=1.0, seed=seed)
    cfg.update(kw)
    return eng.Engine(evaluator=evaluator, **cfg)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stones(board):
    return (np.asarray(board).reshape(len(board), -1) != 0).sum(1)


def engine_on_path(kind, path, monkeypatch, G, **kw):
    """An engine of `kind` ("uniform": the inline evaluator's three paths; "hash": values leave the wave, so the tree
    kernel is the generic one whatever the switch) created under the diagnostic switch of `path`."""
    from azalea_amd import engine as eng
    if path == "no_persistent":
        monkeypatch.setenv("AZX_NO_PERSISTENT", "1")          # (read by azx_create)
    elif path == "generic":
        monkeypatch.setenv("AZX_MCTS_GENERIC", "1")
    E = make(eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH, G, **kw)
    if kind == "hash":
        E.set_prior_table(ref.TABLE)
    else:
        info = E.kernel_info()
        assert ("k_play<2> (persistent)" in info) == (path == "persistent"), info
        assert ("FAST" in info) == (path != "generic"), info
    return E


def first_rows(E, prefixes):
    """Reset the slots to the prefixes and play: one ply (the statistics are read there), then every slot's game to its
    end, so that the harvest hands over the row the first ply recorded.  Returns (per slot: that row's moves_prob and
    metrics, azx_forced_playouts_stats after the one ply)."""
    G = len(prefixes)
    E.reset(moves=[list(p) for p in prefixes])
    never = 4 * G * CELLS                                       # more rows than these plies can record: max_plies ends the calls
    parts = []
    rows, _ = E.play(never, max_plies=1)
    parts.append((rows, E.play_row_metrics()))
    stats = E.forced_playouts_stats()
    rows, _ = E.play(never, max_plies=CELLS)                    # a 5x5 game is over after 25 plies
    parts.append((rows, E.play_row_metrics()))
    rows = {k: np.concatenate([p[0][k] for p in parts]) for k in ROW_KEYS}
    m = np.concatenate([p[1] for p in parts])
    assert len(m) == len(rows["reward"])
    out = []
    for g, prefix in enumerate(prefixes):
        mine = np.flatnonzero(rows["game_uid"] % G == g)
        mine = mine[rows["game_uid"][mine] == rows["game_uid"][mine].min()]      # the slot's first game: the prefix's
        r = mine[np.argmin(stones(rows["board"][mine]))]
        assert np.array_equal(rows["board"][r], ref.game_at(prefix).board), (g, prefix)
        assert rows["nlegal"][r] == CELLS - len(prefix)
        out.append((rows["moves_prob"][r], m[r]))
    return out, stats


def raw_sum(metrics):
    """The raw visit sum of a row: metric 4 (mean root-child visits) times metric 6 (root children)."""
    return int(np.rint(float(metrics[4]) * float(metrics[6])))


# ---- 1. one ply of every reference position, exact ---------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ref.KINDS)
def test_one_ply_of_every_position_forces_where_the_restatement_does(kind, path, monkeypatch):
    refs = ref.positions(kind)
    E = engine_on_path(kind, path, monkeypatch, len(refs))
    assert "forced=off" in E.kernel_info()
    E.set_train_targets("visits")
    E.set_forced_playouts(K, False)
    assert "forced=2/noprune" in E.kernel_info() and E.forced_playouts() == (2.0, False)
    got, stats = first_rows(E, [r["prefix"] for r in refs])
    E.close()
    for (row, m), r in zip(got, refs):
        k = len(r["n"])
        S = raw_sum(m)
        assert S == int(r["n"].sum()), (r["prefix"], S)
        assert np.array_equal(np.rint(row[:k].astype(np.float64) * S), r["n"]), (r["prefix"], row[:k] * S, r["n"])
        assert np.array_equal(bits(row[:k]), bits(ref.shares(r["n"]))) and (row[k:] == 0).all(), r["prefix"]
        assert m[1] == (r["n"] > 0).sum()
    print(kind, path, "forced selects", stats["forced_selects"])
    assert stats == dict(full_plies=len(refs), forced_selects=sum(r["forced"] for r in refs), rows_pruned=0,
                         visits_removed=0)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", ref.KINDS)
def test_one_ply_of_every_position_prunes_what_the_restatement_prunes(kind, path, monkeypatch):
    refs = ref.positions(kind)
    E = engine_on_path(kind, path, monkeypatch, len(refs))
    E.set_train_targets("visits")
    E.set_forced_playouts(K, True)
    assert "forced=2/prune" in E.kernel_info() and E.forced_playouts() == (2.0, True)
    got, stats = first_rows(E, [r["prefix"] for r in refs])
    E.close()
    for (row, m), r in zip(got, refs):                          # no position is dropped: IEEE arithmetic on both sides
        k = len(r["n"])
        assert np.array_equal(bits(row[:k]), bits(ref.shares(r["r"]))) and (row[k:] == 0).all(), (r["prefix"], row[:k], r["r"])
        # the row's metrics stay on the raw counts
        assert raw_sum(m) == int(r["n"].sum()) and m[1] == (r["n"] > 0).sum(), r["prefix"]
    print(kind, path, stats)
    assert stats == dict(full_plies=len(refs), forced_selects=sum(r["forced"] for r in refs),
                         rows_pruned=sum(r["removed"] > 0 for r in refs), visits_removed=sum(r["removed"] for r in refs))


def test_reference_rows_at_temperature_one_are_the_pruned_shares():
    """exploration_depth beyond the game, training targets off: the reference's row at T = 1 is counts / sum(counts), one
    division; under the option the counts are the pruned ones."""
    from azalea_amd import engine as eng
    refs = ref.positions("hash")
    E = make(eng.EVAL_UNIFORM_HASH, len(refs), exploration_depth=CELLS)
    E.set_prior_table(ref.TABLE)
    E.set_forced_playouts(K, True)
    got, stats = first_rows(E, [r["prefix"] for r in refs])
    E.close()
    for (row, m), r in zip(got, refs):
        k = len(r["n"])
        assert np.array_equal(bits(row[:k]), bits(ref.shares(r["r"]))) and (row[k:] == 0).all(), (r["prefix"], row[:k], r["r"])
        assert raw_sum(m) == int(r["n"].sum())
    assert stats["rows_pruned"] == sum(r["removed"] > 0 for r in refs) > 0
    assert stats["visits_removed"] == sum(r["removed"] for r in refs)


@pytest.mark.parametrize("prune", [False, True], ids=["noprune", "prune"])
def test_exact_zeros_among_the_priors(prune):
    """A registered external evaluator hands out rows with exact zeros (tests/gumbel_reference.py's "pow2z"): the forced set
    compares n * n < (k * P) * S, which no child with P = 0 passes, and the prune's f = sqrt((k * P) * S) is 0 there.  The
    counts, the pruned row and the statistics against the restatement under the same priors, exactly as above."""
    from azalea_amd import engine as eng
    import gumbel_reference as gref
    refs = gref.forced_positions_pow2z(K)
    assert all((r["p"] == 0).any() and all(r["p"][j] > 0 for j in r["forced_at"]) for r in refs)
    assert any(((r["p"] == 0) & (r["n"] > 0)).any() for r in refs)
    E = make(eng.EVAL_EXTERNAL, len(refs))
    E.set_external_evaluator(gref.pow2z_device_evaluator(N, DEV))
    E.set_train_targets("visits")
    E.set_forced_playouts(K, prune)
    got, stats = first_rows(E, [r["prefix"] for r in refs])
    E.close()
    for (row, m), r in zip(got, refs):
        k = len(r["n"])
        want = r["r"] if prune else r["n"]
        assert raw_sum(m) == int(r["n"].sum()) and m[1] == (r["n"] > 0).sum(), r["prefix"]
        assert np.array_equal(bits(row[:k]), bits(ref.shares(want))) and (row[k:] == 0).all(), (r["prefix"], row[:k], want)
    print("pow2z", "prune" if prune else "noprune", stats)
    assert stats == dict(full_plies=len(refs), forced_selects=sum(r["forced"] for r in refs),
                         rows_pruned=sum(r["removed"] > 0 for r in refs) if prune else 0,
                         visits_removed=sum(r["removed"] for r in refs) if prune else 0)


# ---- 2. whole games --------------------------------------------------------------------------------------------------
def check_games(rows, m=None):
    """Every game's rows: contiguous, one per ply from the empty board; a valid distribution each (non-negative, zero
    beyond k, sum 1 within 1e-6); each row gives positive probability to the move the next row's board shows; the game
    replays as a legal game under the oracle's rules.  Returns the number of games."""
    uid, ply = rows["game_uid"], stones(rows["board"])
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
    seen = set()
    for s, e in zip(starts, np.r_[starts[1:], len(uid)]):
        assert int(uid[s]) not in seen
        seen.add(int(uid[s]))
        assert np.array_equal(ply[s:e], np.arange(e - s))
        h = ref.game_at([])
        for r in range(s, e):
            k = int(rows["nlegal"][r])
            p = rows["moves_prob"][r]
            assert (p >= 0).all() and (p[k:] == 0).all() and abs(float(p[:k].astype(np.float64).sum()) - 1.0) <= 1e-6, (r, p)
            assert h.result == 0 and np.array_equal(h.board, rows["board"][r])
            legal = h.legal_moves()
            assert len(legal) == k and rows["color"][r] == ply[r] % 2
            if r + 1 < e:
                new = np.flatnonzero((rows["board"][r + 1] != rows["board"][r]).ravel())
                assert len(new) == 1
                tile = int(new[0]) + 1
                assert p[int(np.flatnonzero(legal == tile)[0])] > 0, (r, tile, p[:k])
                h.step(tile)
    return len(starts)


def check_decided(rows):
    """The last mover of a finished Hex game has won it: +1 on the rows of its colour, -1 on the others."""
    uid = rows["game_uid"]
    ends = np.flatnonzero(np.r_[uid[1:] != uid[:-1], True])
    starts = np.r_[0, ends[:-1] + 1]
    for s, e in zip(starts, ends):
        want = np.where(rows["color"][s:e + 1] == rows["color"][e], 1.0, -1.0).astype(np.float32)
        assert np.array_equal(rows["reward"][s:e + 1], want)


def test_the_draw_uses_the_pruned_counts():
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM_HASH, 64, sims=100, seed=5, exploration_depth=CELLS, noise_scale=0.25)    # T = 1 at every ply
    E.set_prior_table(ref.TABLE)
    E.set_forced_playouts(K, True)
    rows, st = E.play(6000)
    m = E.play_row_metrics()
    stats = E.forced_playouts_stats()
    E.close()
    assert st["games"] >= 256
    assert check_games(rows) == st["games"]
    check_decided(rows)
    # the rows are the pruned distribution: some visited children (the raw width, metric 1) have no weight in them
    support = (rows["moves_prob"] > 0).sum(1)
    assert (support <= m[:, 1]).all() and (support < m[:, 1]).any()
    print("rows %d, of those with a child pruned to nothing %d; statistics %s" % (len(support), (support < m[:, 1]).sum(), stats))
    assert stats["rows_pruned"] >= (support < m[:, 1]).sum() > 0 and stats["visits_removed"] >= stats["rows_pruned"]
    assert stats["forced_selects"] > 0 and stats["full_plies"] == st["plies"]
    # metric 2 is the log-probability of the drawn move under the pruned distribution
    uid = rows["game_uid"]
    for r in np.flatnonzero(uid[1:] == uid[:-1])[:500]:
        new = np.flatnonzero((rows["board"][r + 1] != rows["board"][r]).ravel())
        h = ref.game_at([])
        h.set_board(rows["board"][r], 1 + int(rows["color"][r]))
        idx = int(np.flatnonzero(h.legal_moves() == int(new[0]) + 1)[0])
        assert abs(float(m[r, 2]) - np.log(float(rows["moves_prob"][r][idx]))) <= 1e-4


# ---- 3. beside the siblings --------------------------------------------------------------------------------------------
def test_a_playout_caps_fast_plies_neither_force_nor_count():
    from azalea_amd import engine as eng
    seed, G, steps, p = 4242, 64, 8, 0.5
    E = make(eng.EVAL_UNIFORM_HASH, G, sims=100, seed=seed, exploration_depth=2, noise_scale=0.25)
    E.set_prior_table(ref.TABLE)
    E.set_playout_cap(p, 40)
    E.set_forced_playouts(K, True)
    st = E.play_steps(steps)
    raw = E.debug_counters_raw().astype(np.int64)
    stats = E.forced_playouts_stats()
    full = np.array([[eng.playout_cap_is_full(seed, g, q, p) for q in range(steps)] for g in range(G)], bool)
    assert st["games"] == 0 and np.array_equal(raw[:, CTR_CAP_FULL], full.sum(1))
    assert stats["full_plies"] == full.sum() == E.playout_cap_stats()["full_plies"]
    # forced selects are selects of full searches only: all fast would count none
    assert 0 < stats["forced_selects"] <= BS * (100 // BS + 1) * full.sum()
    E.set_playout_cap(1e-9, 40)                                 # (practically) every ply fast; the call keeps the forced setting
    E.set_forced_playouts(K, True)                              # zeroes the statistics
    E.play_steps(4)
    assert E.playout_cap_stats()["full_plies"] == 0
    assert E.forced_playouts_stats() == ZERO_STATS
    E.close()


@pytest.mark.parametrize("sibling", ["early_stop", "resign"])
def test_whole_games_beside_early_stop_and_resignation(sibling):
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM_HASH, 64, sims=100, seed=8, exploration_depth=2, noise_scale=0.25)
    E.set_prior_table(ref.TABLE)
    if sibling == "early_stop":
        E.set_early_stop(True)
    else:
        E.set_resign(0.0, 4, 0.0)                               # hash values sit around 0: about half the judged plies resign
    E.set_forced_playouts(K, True)
    rows, st = E.play(400)
    stats = E.forced_playouts_stats()
    other = E.early_stop_stats() if sibling == "early_stop" else E.resign_stats()
    E.close()
    print(sibling, other, stats)
    assert st["games"] >= 20 and stats["forced_selects"] > 0 and stats["rows_pruned"] > 0
    check_games(rows)                                           # prefix-consistent legal chains from the empty board
    if sibling == "early_stop":
        assert other["stopped_plies"] > 0
        check_decided(rows)
    else:
        assert other["resigned"] > 0
        assert (np.abs(rows["reward"]) == 1).all()


# ---- 4. a network through the half-pools, a registered external evaluator ----------------------------------------------
def sorted_rows(rows, m):
    i = np.argsort(rows["game_uid"], kind="stable")       # finished games enter the queue in the order the GPU finished them
    return {k: rows[k][i].tobytes() for k in ROW_KEYS}, m[i].tobytes()


def run_twice(engine, positions):
    out = []
    for _ in range(2):
        E = engine()
        E.set_forced_playouts(K, True)
        rows, st = E.play(positions)
        stats = E.forced_playouts_stats()
        out.append((sorted_rows(rows, E.play_row_metrics()), stats))
        E.close()
        assert stats["forced_selects"] > 0 and stats["full_plies"] == st["plies"] and stats["rows_pruned"] > 0
        assert check_games(rows) == st["games"] > 0
    assert out[0] == out[1]                                     # the same seed gives the same rows


def test_the_two_half_pools_of_a_network():
    from azalea_amd import engine as eng
    from azalea_amd.network import HexNetwork
    torch.manual_seed(3)
    net = HexNetwork(board_size=N, num_blocks=1, base_chans=64).eval()
    w = {k: v.detach().numpy() for k, v in net.state_dict().items()}

    def engine():
        E = make(eng.EVAL_RESNET, 1024, sims=50, seed=2024, exploration_depth=2, noise_scale=0.25, num_blocks=1,
                 base_chans=64)
        E.set_weights(w)
        assert "two half-pools" in E.kernel_info(), E.kernel_info()
        return E
    run_twice(engine, 2000)


def test_a_registered_external_evaluator():
    from azalea_amd import engine as eng
    inv = torch.tensor(ref.TABLE, device=DEV)

    def evaluate(board, legal):                                   # uniform priors, a value from the stones' positions
        k = (legal != 0).sum(1)
        prior = torch.where(legal != 0, inv[k][:, None], torch.zeros((), device=DEV))
        wts = torch.arange(1, CELLS + 1, dtype=torch.float32, device=DEV)
        value = torch.tanh(((board.reshape(len(board), -1) == 1).float() * wts).sum(1) * 0.37 - 3.0)
        return value.to(torch.float32), prior

    def engine():
        E = make(eng.EVAL_EXTERNAL, 64, sims=50, seed=99, exploration_depth=2, noise_scale=0.25)
        E.set_external_evaluator(evaluate)
        return E
    run_twice(engine, 200)


# ---- 5. never set, or set then cleared ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
def test_the_option_never_set_or_cleared_leaves_no_trace(kind):
    from azalea_amd import engine as eng
    evaluator = eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH
    out, infos = [], []
    for cleared in (False, True):
        E = make(evaluator, 64, sims=40, bs=4, seed=11, exploration_depth=2, noise_scale=0.25)
        if cleared:
            E.set_forced_playouts(K, True)
            assert "forced=2/prune" in E.kernel_info()
            E.set_forced_playouts(0, False)
        infos.append(E.kernel_info())
        rows, st = E.play(200)
        out.append((sorted_rows(rows, E.play_row_metrics()), {k: v for k, v in st.items() if not k.endswith("seconds")},
                    E.debug_counters_raw().tobytes(), E.debug_counters().tobytes()))
        assert E.forced_playouts_stats() == ZERO_STATS and E.forced_playouts() == (0.0, False)
        E.close()
    assert out[0] == out[1]
    assert "forced=off" in infos[0] and infos[0] == infos[1]


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_bad_calls_are_einval_and_change_nothing():
    import ctypes as C
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM, 16, sims=40, bs=4)
    L = E.L
    E.set_forced_playouts(3.0, True)
    for k, prune in ((-1.0, 0), (64.5, 1), (float("nan"), 1), (float("inf"), 0), (2.0, 2), (2.0, -1), (0.0, 1)):
        assert L.azx_set_forced_playouts(E.h, k, prune) == EINVAL and b"forced playouts" in L.azx_last_error()
        assert "forced=3/prune" in E.kernel_info() and E.forced_playouts() == (3.0, True)      # the setting before is left in place
    assert L.azx_set_forced_playouts(None, 2.0, 1) == EINVAL
    assert L.azx_forced_playouts_stats(E.h, None) == EINVAL
    kk, pp = C.c_float(0), C.c_int(0)
    assert L.azx_get_forced_playouts(E.h, None, C.byref(pp)) == EINVAL and L.azx_get_forced_playouts(E.h, C.byref(kk), None) == EINVAL
    for bad in ((-1.0, False), (100.0, True), (0.0, True), (2.0, 2)):
        with pytest.raises(ValueError, match="forced playouts"):
            E.set_forced_playouts(*bad)
    assert E.forced_playouts() == (3.0, True)
    assert L.azx_set_forced_playouts(E.h, 64.0, 0) == 0 and "forced=64/noprune" in E.kernel_info()
    E.clear_forced_playouts()
    assert "forced=off" in E.kernel_info()
    E.close()


def test_matches_and_tournaments_refuse_the_option_before_touching_any_engine():
    from azalea_amd import engine as eng
    from azalea_amd._lib import AzxError
    a, b = (make(eng.EVAL_UNIFORM_HASH, 64, sims=16, bs=4, seed=s, exploration_depth=4, noise_scale=0.25) for s in (6, 7))
    for e in (a, b):
        e.play(40)                                            # rows in both harvest queues, games under way in the slots
    m, t = eng.Match(a, b), eng.Tournament([a, b])

    def state():
        out = []
        for e in (a, b):
            g = e.get_games()
            out.append((g["board"].tobytes(), g["ply"].tobytes(), e.get_root()["root_visits"].tobytes(),
                        {k: v.tobytes() for k, v in e.rows_read(0, e._last_rows).items()}))
        return out
    before = state()
    for on, name, idx in ((b, "b", 1), (a, "a", 0)):
        on.set_forced_playouts(K, False)
        with pytest.raises(AzxError, match=r"azx error -1: engine %s has forced playouts set" % name):
            m.play(4)
        with pytest.raises(AzxError, match=r"azx error -1: engine %d has forced playouts set" % idx):
            t.play([(0, 1)], 4)
        assert state() == before                              # both engines' slots and queues are as they were
        on.clear_forced_playouts()
    res = m.play(8)                                           # after clearing, it plays
    assert (res["outcome"] != 0).all() and (res["length"] >= 9).all()
    m.close()
    t.close()
    a.close()
    b.close()


# ---- 7. training smoke -------------------------------------------------------------------------------------------------
SEARCH = dict(simulations=40, search_batch_size=5, exploration_coef=1.0, exploration_depth=2,
              exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0)


def cuda_policy():
    from azalea_amd.policy import Policy
    torch.manual_seed(1)
    policy = Policy()
    policy.initialize(dict(device="cuda:0", network="HexNetwork", board_size=N, num_blocks=1, base_chans=16, seed=1,
                           **SEARCH))
    return policy


class Lines(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_a_two_step_train_runs_under_the_option(tmp_path, monkeypatch):
    from azalea_amd.parallel_player import Player
    from azalea_amd.policy_trainer import train
    config = dict(seed=1, device="cuda:0", game="azalea_amd.game.hex.HexGame", board_size=N, replaybuf_size=256,
                  replaybuf_oversampling=1.0, batch_size=64, lr_initial=0.05, lr_decay=0.1, lr_decay_epochs=1,
                  momentum=0.9, l2_regularization=1e-4, total_epochs=2, selfplay_games=64, log_interval=1,
                  model_checkpoint_interval=0, forced_playouts={"k": 2.0, "prune": True})
    log = Lines()
    root = logging.getLogger()
    level = root.level
    root.addHandler(log)
    root.setLevel(logging.INFO)
    infos, players = [], []
    stop = Player.stop

    def stop_and_tell(player):                  # train() stops its players at the end: ask their engines first
        players.append(player.forced_playouts)
        if player.forced_playouts is not None:  # (not the random-mover player that fills the first buffer)
            infos.append((player.device_engine().kernel_info(), player.forced_playouts_stats()))
        stop(player)
    monkeypatch.setattr(Player, "stop", stop_and_tell)
    try:
        path = train(cuda_policy(), config, str(tmp_path))
    finally:
        root.removeHandler(log)
        root.setLevel(level)
    assert os.path.exists(path)
    assert players.count(None) >= 1 and players.count((2.0, True)) == 1, players
    assert len(infos) == 1 and "forced=2/prune" in infos[0][0], infos
    fs = infos[0][1]
    assert fs["full_plies"] > 0 and fs["forced_selects"] > 0
    said = [l for l in log.lines if "config['forced_playouts']" in l]
    assert len(said) == 1 and "NOT the reference's behaviour" in said[0], said
