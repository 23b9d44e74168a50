"""Early stop of a search whose move can no longer change (azx_set_early_stop; NOT the reference's behaviour, off by
default) on the device.  The rule's reference is tests/early_stop_reference.py: the unmodified CPU oracle run batch by
batch.  Every case plays 5x5 boards."""
import logging
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import early_stop_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N, CELLS, NB, BS = ref.N, ref.CELLS, ref.NB, ref.BS
EINVAL = -1
ROW_KEYS = ("board", "color", "nlegal", "moves_prob", "reward", "game_uid")
CTR_SELECTS, CTR_PLIES, CTR_CAP_FULL, CTR_CAP_FAST = 0, 8, 13, 14
STAT_KEYS = ("t0_plies", "stopped_plies", "batches_skipped")


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


def selects(E):
    return E.debug_counters_raw()[:, CTR_SELECTS].astype(np.int64)


def board_of(prefix):
    return ref.game_at(prefix).board


def one_ply(E, prefixes):
    """reset to the prefixes, play one ply: (selects of the ply per slot, games after, roots after, play statistics)."""
    E.reset(moves=[list(p) for p in prefixes])
    before = selects(E)
    st = E.play_steps(1)
    return selects(E) - before, E.get_games(), E.get_root(), st


def check_against_oracle(refs, sel, games, root, key_b, key_leader, key_root):
    """Per slot: the ply's select count, and where the move does not end the game the stone placed and the carried
    root, bit for bit."""
    for g, r in enumerate(refs):
        b = r[key_b] if key_b else NB
        assert sel[g] == b * BS, (g, r["prefix"], sel[g], b)
        h = ref.game_at(r["prefix"])
        tile = int(h.legal_moves()[r[key_leader]])
        h.step(tile)
        if h.result:
            continue                                           # the game was harvested and the slot restarted
        assert np.array_equal(games["board"][g], h.board), (g, r["prefix"], tile)
        nv, tv, rv, rw = r[key_root]
        k = int(root["k"][g])
        assert k == CELLS - len(r["prefix"]) - 1
        want_nv, want_tv = np.zeros(k, np.float32), np.zeros(k, np.float32)
        want_nv[:len(nv)], want_tv[:len(tv)] = nv, tv          # (an unexpanded new root has no children yet)
        assert np.array_equal(bits(root["child_visits"][g, :k]), bits(want_nv)), (g, r["prefix"])
        assert np.array_equal(bits(root["child_value"][g, :k]), bits(want_tv)), (g, r["prefix"])
        assert bits(root["root_visits"][g:g + 1])[0] == bits([rv])[0] and bits(root["root_value"][g:g + 1])[0] == bits([rw])[0]


# ---- 1. exact against the oracle ------------------------------------------------------------------------------------
def test_one_ply_of_every_position_stops_where_the_oracle_rule_does():
    from azalea_amd import engine as eng
    refs, dropped = ref.positions("hash")
    stopping = [r for r in refs if r["b_star"] < NB]
    assert dropped <= ref.MAX_DROPPED_SHARE * (len(refs) + dropped) and len(stopping) >= ref.MIN_STOPPING
    assert len(refs) <= 128
    E = make(eng.EVAL_UNIFORM_HASH, len(refs))
    E.set_prior_table(ref.TABLE)
    prefixes = [r["prefix"] for r in refs]
    assert "estop=off" in E.kernel_info()
    E.set_early_stop(True)
    assert "estop=on" in E.kernel_info() and "cap=off" in E.kernel_info() and "resign=off" in E.kernel_info()
    sel, games, root, st = one_ply(E, prefixes)
    print("selects per slot under the option:", sel.tolist())
    check_against_oracle(refs, sel, games, root, "b_star", "leader", "stop_root")
    assert E.early_stop_stats() == ref.counts_of(refs)
    assert st["selects"] == sel.sum() == BS * (NB * len(refs) - ref.counts_of(refs)["batches_skipped"])
    # control: the same engine with the option off runs every batch and carries the full search's subtree
    E.set_early_stop(False)
    assert "estop=off" in E.kernel_info()
    sel, games, root, st = one_ply(E, prefixes)
    assert (sel == NB * BS).all()
    check_against_oracle(refs, sel, games, root, None, "full_leader", "full_root")
    assert E.early_stop_stats() == dict.fromkeys(STAT_KEYS, 0)
    E.close()


# ---- 2. every path of the inline evaluator --------------------------------------------------------------------------
def uniform_positions():
    """Value 0 everywhere spreads the visits: most mid-game positions tie, so these are the last prefixes of more
    games (no cap on the dropped share here; enough of them must stop)."""
    refs, _ = ref.positions("uniform", n_games=16, seed=7, tail=5)
    assert sum(r["b_star"] < NB for r in refs) >= 10 and any(r["b_star"] == NB for r in refs)
    return refs


@pytest.mark.parametrize("path", ["persistent", "no_persistent", "generic"])
def test_every_inline_path_stops_where_the_oracle_rule_does(path, monkeypatch):
    from azalea_amd import engine as eng
    if path == "no_persistent":
        monkeypatch.setenv("AZX_NO_PERSISTENT", "1")          # (read by azx_create)
    elif path == "generic":
        monkeypatch.setenv("AZX_MCTS_GENERIC", "1")
    refs = uniform_positions()
    E = make(eng.EVAL_UNIFORM, len(refs))
    info = E.kernel_info()
    assert ("k_play<2> (persistent)" in info) == (path == "persistent"), info
    assert ("FAST" in info) == (path != "generic"), info
    E.set_early_stop(True)
    sel, games, root, st = one_ply(E, [r["prefix"] for r in refs])
    print(path, "selects per slot under the option:", sel.tolist())
    check_against_oracle(refs, sel, games, root, "b_star", "leader", "stop_root")
    assert E.early_stop_stats() == ref.counts_of(refs)
    E.close()


# ---- 3. network and external paths: not bit-comparable to the oracle ------------------------------------------------
def net_weights(blocks=1, chans=64, seed=3):
    from azalea_amd.network import HexNetwork
    torch.manual_seed(seed)
    net = HexNetwork(board_size=N, num_blocks=blocks, base_chans=chans).eval()
    return {k: v.detach().numpy() for k, v in net.state_dict().items()}


def check_on_against_off(A, B, prefixes, nb):
    """Engines A (off) and B (on), same seed, reset to the same prefixes, one ply each."""
    sa, ga, ra, sta = one_ply(A, prefixes)
    sb, gb, rb, stb = one_ply(B, prefixes)
    assert (sa == nb * BS).all()
    assert np.array_equal(ga["board"], gb["board"]) and np.array_equal(ga["ply"], gb["ply"])     # every slot makes the same move
    assert (sb <= sa).all() and (sb % BS == 0).all()
    stopped = sb < sa
    es = B.early_stop_stats()
    print("stopped %d of %d slots, batches skipped %d" % (stopped.sum(), len(sb), es["batches_skipped"]))
    assert es["t0_plies"] == len(prefixes) and es["stopped_plies"] == stopped.sum() > 0
    assert es["batches_skipped"] * BS == (sa - sb).sum()
    # a stopped slot's leader was ahead by more than the selects left: n1 - n2 > 0, and since n2 >= 0 the carried
    # root (the leader itself, where the game goes on) holds more visits than the selects skipped
    went_on = stopped & (gb["ply"] > 0)
    assert went_on.any()
    assert (rb["root_visits"][went_on] > (sa - sb)[went_on]).all()
    assert stb["evals"] < sta["evals"]
    assert A.early_stop_stats() == dict.fromkeys(STAT_KEYS, 0)


def test_the_half_pools_of_a_network_make_the_same_moves_with_fewer_selects():
    from azalea_amd import engine as eng
    refs, _ = ref.positions("hash")
    G, sims = 1024, 100
    prefixes = [refs[g % len(refs)]["prefix"] for g in range(G)]
    w = net_weights()
    pair = []
    for _ in range(2):
        E = make(eng.EVAL_RESNET, G, sims=sims, seed=2024, noise_scale=0.25, num_blocks=1, base_chans=64)
        E.set_weights(w)
        assert "two half-pools" in E.kernel_info(), E.kernel_info()
        pair.append(E)
    pair[1].set_early_stop(True)
    check_on_against_off(pair[0], pair[1], prefixes, sims // BS + 1)
    for E in pair:
        E.close()


def test_a_registered_external_evaluator_makes_the_same_moves_with_fewer_selects():
    from azalea_amd import engine as eng
    refs, _ = ref.positions("hash")
    G, sims = 64, 100
    prefixes = [refs[g % len(refs)]["prefix"] for g in range(G)]
    inv = torch.tensor(ref.TABLE, device=DEV)

    def evaluate(board, legal):                                   # uniform priors, a value from the stones' positions
        k = (legal != 0).sum(1)
        prior = torch.where(legal != 0, inv[k][:, None], torch.zeros((), device=DEV))
        wts = torch.arange(1, CELLS + 1, dtype=torch.float32, device=DEV)
        value = torch.tanh(((board.reshape(len(board), -1) == 1).float() * wts).sum(1) * 0.37 - 3.0)
        return value.to(torch.float32), prior
    pair = []
    for _ in range(2):
        E = make(eng.EVAL_EXTERNAL, G, sims=sims, seed=99, noise_scale=0.25)
        E.set_external_evaluator(evaluate)
        pair.append(E)
    pair[1].set_early_stop(True)
    check_on_against_off(pair[0], pair[1], prefixes, sims // BS + 1)
    for E in pair:
        E.close()


# ---- 4. the temperature gate ----------------------------------------------------------------------------------------
def sorted_rows(rows, m):
    i = np.argsort(rows["game_uid"], kind="stable")       # finished games enter the queue in the order the GPU finished them
    return {k: rows[k][i].tobytes() for k in ROW_KEYS}, m[i].tobytes()


@pytest.mark.parametrize("kind", ["uniform", "hash"])
def test_plies_drawn_at_a_temperature_are_untouched(kind):
    from azalea_amd import engine as eng
    evaluator = eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH
    out = []
    for on in (False, True):
        E = make(evaluator, 64, sims=40, bs=4, seed=11, exploration_depth=CELLS, noise_scale=0.25)     # no ply reaches the depth
        if on:
            E.set_early_stop(True)
        rows, st = E.play(200)
        out.append((sorted_rows(rows, E.play_row_metrics()), {k: v for k, v in st.items() if not k.endswith("seconds")},
                    E.debug_counters_raw().tobytes(), E.get_games()["board"].tobytes()))
        if on:
            assert E.early_stop_stats() == dict.fromkeys(STAT_KEYS, 0)
        E.close()
    assert out[0] == out[1]


# ---- 5. whole games under the option --------------------------------------------------------------------------------
def check_games(rows, depth, chain=True):
    """Every game's rows: contiguous, plies ascending; a T = 0 row is uniform over the most-visited children (one-hot
    unless the search ended in a tie, which a stopped search cannot); with `chain` each row's stone leads to the next
    row's board (the argmax's on a T = 0 row) and the game replays as a legal decided game under the oracle's rules.
    Returns (T = 0 rows, of those not one-hot)."""
    uid, ply = rows["game_uid"], stones(rows["board"])
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
    t0 = ties = 0
    seen = set()
    for s, e in zip(starts, np.r_[starts[1:], len(uid)]):
        assert int(uid[s]) not in seen
        seen.add(int(uid[s]))
        assert (np.diff(ply[s:e]) > 0).all()
        for r in range(s, e):
            k = int(rows["nlegal"][r])
            p = rows["moves_prob"][r]
            assert (p[k:] == 0).all()
            if ply[r] >= depth:
                t0 += 1
                nz = p[:k][p[:k] > 0]
                assert len(nz) >= 1 and (nz == np.float32(1.0) / np.float32(len(nz))).all(), (r, p[:k])
                ties += len(nz) > 1
        if not chain:
            continue
        assert np.array_equal(ply[s:e], np.arange(ply[s], ply[s] + e - s))
        h = ref.game_at([])
        h.set_board(rows["board"][s], 1 + int(ply[s]) % 2)
        for r in range(s, e):
            assert h.result == 0 and np.array_equal(h.board, rows["board"][r])
            k = int(rows["nlegal"][r])
            legal = h.legal_moves()
            assert len(legal) == k and rows["color"][r] == ply[r] % 2
            if r + 1 < e:
                new = np.flatnonzero((rows["board"][r + 1] != rows["board"][r]).ravel())
                assert len(new) == 1
                tile = int(new[0]) + 1
                idx = int(np.flatnonzero(legal == tile)[0])
                assert rows["moves_prob"][r][idx] > 0
                if ply[r] >= depth:
                    assert rows["moves_prob"][r][idx] == rows["moves_prob"][r][:k].max()
                h.step(tile)
    return t0, ties


def test_whole_games_under_the_option_are_legal_decided_games():
    from azalea_amd import engine as eng
    depth = 2
    E = make(eng.EVAL_UNIFORM_HASH, 64, sims=100, seed=5, exploration_depth=depth, noise_scale=0.25)
    E.set_prior_table(ref.TABLE)
    E.set_early_stop(True)
    rows, st = E.play(400)
    m = E.play_row_metrics()
    es = E.early_stop_stats()
    E.close()
    assert st["games"] >= 20 and len(rows["reward"]) >= 400
    t0, ties = check_games(rows, depth)
    print("T = 0 rows %d, not one-hot (a full search that ended in a tie) %d; statistics %s" % (t0, ties, es))
    assert es["stopped_plies"] > 0 and es["t0_plies"] >= t0 > 0
    assert ties <= es["t0_plies"] - es["stopped_plies"]       # a stopped ply's leader is unique: its row is one-hot
    # the last mover of a finished Hex game has won it: +1 on the rows of its colour, -1 on the others
    uid = rows["game_uid"]
    ends = np.flatnonzero(np.r_[uid[1:] != uid[:-1], True])
    starts = np.r_[0, ends[:-1] + 1]
    for s, e in zip(starts, ends):
        want = np.where(rows["color"][s:e + 1] == rows["color"][e], 1.0, -1.0).astype(np.float32)
        assert np.array_equal(rows["reward"][s:e + 1], want)
        h = ref.game_at([])
        h.set_board(rows["board"][e], 1 + int(rows["color"][e]))
        k = int(rows["nlegal"][e])
        if (rows["moves_prob"][e][:k] > 0).sum() == 1:         # (a tie's move is drawn: the row does not name it)
            h.step(int(h.legal_moves()[int(np.argmax(rows["moves_prob"][e][:k]))]))
            assert h.result != 0                               # the last row's move decides the game
    # search_value is the mean over the selects the ply made: finite and within the value range
    assert np.isfinite(m[:, 0]).all() and (np.abs(m[:, 0]) <= 1.0).all()
    assert st["selects"] == BS * ((100 // BS + 1) * st["plies"] - es["batches_skipped"])


# ---- 6. with a playout cap and with resignation ---------------------------------------------------------------------
def test_a_playout_cap_keeps_its_schedule_and_its_fast_plies_stop_too():
    from azalea_amd import engine as eng
    seed, G, steps, depth, p = 4242, 64, 8, 2, 0.5
    E = make(eng.EVAL_UNIFORM_HASH, G, sims=100, seed=seed, exploration_depth=depth, noise_scale=0.25)
    E.set_prior_table(ref.TABLE)
    E.set_playout_cap(p, 40)
    E.set_early_stop(True)
    st = E.play_steps(steps)
    raw = E.debug_counters_raw().astype(np.int64)
    full = np.array([[eng.playout_cap_is_full(seed, g, q, p) for q in range(steps)] for g in range(G)], bool)
    nb_full, nb_fast = 100 // BS + 1, 40 // BS + 1
    bound = BS * np.where(full, nb_full, nb_fast).sum(1)
    assert np.array_equal(raw[:, CTR_PLIES], np.full(G, steps)) and st["games"] == 0
    assert np.array_equal(raw[:, CTR_CAP_FULL], full.sum(1)) and np.array_equal(raw[:, CTR_CAP_FAST], (~full).sum(1))
    assert (raw[:, CTR_SELECTS] <= bound).all() and (raw[:, CTR_SELECTS] % BS == 0).all()
    # the plies drawn at a temperature run their whole schedule: the bound less the T = 0 plies' is a floor
    floor = BS * np.where(full, nb_full, nb_fast)[:, :depth].sum(1)
    assert (raw[:, CTR_SELECTS] >= floor).all()
    es = E.early_stop_stats()
    assert es["t0_plies"] == G * (steps - depth) and es["stopped_plies"] > 0
    assert bound.sum() - raw[:, CTR_SELECTS].sum() == BS * es["batches_skipped"] > 0
    assert E.playout_cap_stats() == dict(full_plies=int(full.sum()), fast_plies=int((~full).sum()), empty_games=0)
    E.close()


def test_a_resigned_game_is_still_a_prefix_consistent_game():
    from azalea_amd import engine as eng
    depth = 2
    E = make(eng.EVAL_UNIFORM_HASH, 64, sims=100, seed=8, exploration_depth=depth, noise_scale=0.25)
    E.set_prior_table(ref.TABLE)
    E.set_resign(0.0, 4, 0.0)                                # hash values sit around 0: about half the judged plies resign
    E.set_early_stop(True)
    rows, st = E.play(300)
    rs, es = E.resign_stats(), E.early_stop_stats()
    E.close()
    print("resign statistics %s, early stop statistics %s" % (rs, es))
    assert rs["resigned"] > 0 and es["stopped_plies"] > 0
    check_games(rows, depth)                                   # legal chains from the empty board, T = 0 rows at the argmax
    uid = rows["game_uid"]
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
    assert (stones(rows["board"][starts]) == 0).all()


# ---- 7. cleared leaves no trace -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "hash"])
def test_the_option_never_set_or_cleared_leaves_no_trace(kind):
    from azalea_amd import engine as eng
    evaluator = eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH
    out, infos = [], []
    for cleared in (False, True):
        E = make(evaluator, 64, sims=40, bs=4, seed=11, exploration_depth=2, noise_scale=0.25)
        if cleared:
            E.set_early_stop(True)
            assert "estop=on" in E.kernel_info()
            E.set_early_stop(False)
        infos.append(E.kernel_info())
        rows, st = E.play(200)
        out.append((sorted_rows(rows, E.play_row_metrics()), {k: v for k, v in st.items() if not k.endswith("seconds")},
                    E.debug_counters_raw().tobytes()))
        assert E.early_stop_stats() == dict.fromkeys(STAT_KEYS, 0)
        E.close()
    assert out[0] == out[1]
    assert "estop=off" in infos[0] and infos[0] == infos[1]


# ---- 8. refusals ----------------------------------------------------------------------------------------------------
def test_bad_calls_are_einval_and_change_nothing():
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM, 16, sims=40, bs=4)
    L = E.L
    E.set_early_stop(True)
    for bad in (2, -1, 7):
        assert L.azx_set_early_stop(E.h, bad) == EINVAL and b"early stop" in L.azx_last_error()
        assert "estop=on" in E.kernel_info()                  # the setting before is left in place
    assert L.azx_set_early_stop(None, 1) == EINVAL
    assert L.azx_early_stop_stats(E.h, None) == EINVAL
    with pytest.raises(ValueError, match="early stop"):
        E.set_early_stop(2)
    E.set_early_stop(False)
    assert "estop=off" in E.kernel_info()
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
        on.set_early_stop(True)
        with pytest.raises(AzxError, match=r"azx error -1: engine %s has early stop set" % name):
            m.play(4)
        with pytest.raises(AzxError, match=r"azx error -1: engine %d has early stop set" % idx):
            t.play([(0, 1)], 4)
        assert state() == before                              # both engines' slots and queues are as they were
        on.set_early_stop(False)
    res = m.play(8)                                           # after clearing, it plays
    assert (res["outcome"] != 0).all() and (res["length"] >= 9).all()
    m.close()
    t.close()
    a.close()
    b.close()


# ---- 9. training smoke ----------------------------------------------------------------------------------------------
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
                  model_checkpoint_interval=0, early_stop=True)
    log = Lines()
    root = logging.getLogger()
    level = root.level
    root.addHandler(log)
    root.setLevel(logging.INFO)
    infos, players = [], []
    stop = Player.stop

    def stop_and_tell(player):                  # train() stops its players at the end: ask their engines first
        players.append(player.early_stop)
        if player.early_stop:                   # (not the random-mover player that fills the first buffer)
            infos.append((player.device_engine().kernel_info(), player.early_stop_stats()))
        stop(player)
    monkeypatch.setattr(Player, "stop", stop_and_tell)
    try:
        path = train(cuda_policy(), config, str(tmp_path))
    finally:
        root.removeHandler(log)
        root.setLevel(level)
    assert os.path.exists(path)
    assert players.count(False) >= 1 and players.count(True) == 1, players
    assert len(infos) == 1 and "estop=on" in infos[0][0], infos
    es = infos[0][1]
    assert es["t0_plies"] > 0 and es["stopped_plies"] > 0 and es["batches_skipped"] >= es["stopped_plies"]
    said = [l for l in log.lines if "config['early_stop']" in l]
    assert len(said) == 1 and "NOT the reference's behaviour" in said[0], said
