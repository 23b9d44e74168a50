"""The weighted opening book of device self-play (azx_set_selfplay_openings) on the GPU.

The reference for a game under the book is the EXISTING prefix path: game u must equal, row for row and bit for bit
(board, colour, nlegal, moves_prob, reward and every row metric), the first game a second engine plays in a slot after
Engine.reset(moves=[book[index(u)]]), that engine's seed + uid for the slot being this engine's seed + u.  The uids of
one generation are consecutive over the slots, and Engine.reset hands slot g of a fresh engine of G slots the uid
G + g: a reference engine of the same G with the seed shifted by (t - 1) * G reproduces generation t whole.

The inline evaluators are the uniform-hash one with a prior table (per-move launches, the generic tree kernel) and the
plain uniform one with the default table (the persistent k_play loop, which the hash evaluator never enters)."""
import re
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
EINVAL = -1
ROW_KEYS = ("board", "color", "nlegal", "moves_prob", "reward")
# lengths 0, 1, 2 and 3 (both parities), one zero-weight entry, weighted
BOOK5 = [[], [13], [7, 19], [1, 25, 12], [3], [24, 2]]
WEIGHTS5 = [1.0, 2.0, 2.0, 3.0, 0.0, 1.5]


def table(cells):
    return (np.float32(1.0) / np.arange(0, cells + 1).clip(1).astype(np.float32)).astype(np.float32)


def make(kind, n=5, G=16, sims=16, bs=4, seed=20261020, **kw):
    from azalea_amd import engine as eng
    evaluator = dict(hash=eng.EVAL_UNIFORM_HASH, uniform=eng.EVAL_UNIFORM, resnet=eng.EVAL_RESNET,
                     external=eng.EVAL_EXTERNAL)[kind]
    cfg = dict(board_size=n, n_games=G, simulations=sims, search_batch_size=bs, exploration_coef=0.5,
               exploration_depth=4, noise_alpha=0.3, noise_scale=0.25, temperature=1.0, seed=seed)
    cfg.update(kw)
    E = eng.Engine(evaluator=evaluator, **cfg)
    if kind == "hash":
        E.set_prior_table(table(n * n))
    return E


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stones(board):
    return (np.asarray(board).reshape(len(board), -1) != 0).sum(1)


def position(n, moves):
    """The board azx_get_games / a row shows after `moves` (tile + 1, colour 1 first)."""
    b = np.zeros(n * n, np.int32)
    for p, m in enumerate(moves):
        b[m - 1] = 1 + (p & 1)
    return b.reshape(n, n)


def collect(rows, met, games):
    """The whole games of one Engine.play call into {uid: dict(rows..., metrics)}."""
    uid = rows["game_uid"]
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]]) if len(uid) else []
    for s, e in zip(starts, np.r_[starts[1:], len(uid)]):
        u = int(uid[s])
        assert u not in games                                      # a game is harvested once, its rows contiguous
        games[u] = dict({k: rows[k][s:e].copy() for k in ROW_KEYS}, metrics=met[s:e].copy())
    return games


def harvest(E, want, games=None, limit=400):
    """Play until every uid in `want` is harvested.  {uid: dict(rows..., metrics)}, whole games only."""
    games = {} if games is None else games
    want = set(int(u) for u in want)
    for _ in range(limit):
        if want <= set(games):
            return games
        rows, st = E.play(1)
        collect(rows, E.play_row_metrics(), games)
    raise AssertionError("games %r were never harvested" % sorted(want - set(games))[:8])


def same_game(a, b, what):
    assert len(a["reward"]) == len(b["reward"]), what
    for k in ("board", "color", "nlegal"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("moves_prob", "reward", "metrics"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def index_of(seed, uids, weights_or_n):
    from azalea_amd import engine as eng
    return eng.selfplay_opening_index(seed, np.asarray(uids, np.int64), eng.selfplay_openings_bounds(weights_or_n))


def check_generations(kind, book, weights, gens, options=None, n=5, G=16, seed=20261020, setup=None, **kw):
    """Generations `gens` of an engine under the book against the prefix path.  `options(E)` sets the same self-play
    options on both engines, `setup(E)` the evaluator's weights or callback.  Returns the engine under the book and
    its games."""
    options = options or (lambda E: None)
    setup = setup or (lambda E: None)
    A = make(kind, n=n, G=G, seed=seed, **kw)
    setup(A)
    A.set_selfplay_openings(book, weights)
    options(A)
    assert "book=%d" % len(book) in A.kernel_info()
    uids = np.concatenate([np.arange(t * G, (t + 1) * G) for t in gens])
    games = harvest(A, uids)
    idx = index_of(seed, uids, len(book) if weights is None else weights)
    cells = n * n
    for u, o in zip(uids.tolist(), idx.tolist()):
        g, L = games[u], len(book[o])
        assert weights is None or weights[o] > 0
        assert np.array_equal(g["board"][0], position(n, book[o])), (u, o)     # the first row is the opening's position
        assert np.array_equal(stones(g["board"]), L + np.arange(len(g["reward"]))), u
        assert g["nlegal"][0] == cells - L and np.array_equal(g["color"], stones(g["board"]) & 1), u
        assert g["metrics"][0, 3] == 1.0 and (g["metrics"][1:, 3] == 0.0).all(), u
    equal_the_prefix_path(games, kind, book, weights, gens, options, n, G, seed, setup, **kw)
    return A, games


def equal_the_prefix_path(games, kind, book, weights, gens, options, n, G, seed, setup, **kw):
    """Every game of generations `gens` in `games` equals the first game a reference engine plays from its opening."""
    for t in gens:
        B = make(kind, n=n, G=G, seed=seed + (t - 1) * G, **kw)
        setup(B)
        options(B)
        gu = np.arange(t * G, (t + 1) * G)
        B.reset(moves=[book[o] for o in index_of(seed, gu, len(book) if weights is None else weights)])
        assert (B.selfplay_openings_slots() == -1).all()
        ref = harvest(B, np.arange(G, 2 * G))
        for g in range(G):
            same_game(games[t * G + g], ref[G + g], (t, g))
        B.close()


# ---- 1. three generations on 5x5: the re-seating kernel (generation 0) and the restart branch (1 and 2) ----------------
@pytest.mark.parametrize("kind, env, path", [
    ("hash", {}, "k_mcts + k_choose + k_advance per move"),
    ("uniform", {}, "k_play<2> (persistent)"),
    ("uniform", {"AZX_NO_PERSISTENT": "1"}, "k_mcts + k_choose + k_advance per move"),
    ("uniform", {"AZX_MCTS_GENERIC": "1"}, "k_mcts + k_choose + k_advance per move"),
])
def test_three_generations_equal_the_prefix_path(kind, env, path, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)                                   # read once per engine, at its creation
    A, games = check_generations(kind, BOOK5, WEIGHTS5, (0, 1, 2))
    info = A.kernel_info()
    assert path in info, info
    for k, v in env.items():
        assert "%s=%s" % (k, v) in info
    idx = index_of(20261020, sorted(games), WEIGHTS5)
    assert len(set(idx.tolist())) >= 4 and 4 not in idx            # several openings were drawn; the zero weight never
    A.close()


@pytest.mark.parametrize("kind", ["uniform", "hash"])
def test_parked_slots_rejoin_under_the_book(kind):
    """The unpark path: with the harvest queue forced small for one call (azx_debug_set_queue_cap, as
    tests/test_gpu_round2.py does) finished games park their slots; the next call hands their rows over and restarts
    those slots through k_advance's unpark mode -- under the book."""
    seed, G = 909, 16
    A = make(kind, seed=seed, G=G)
    A.set_selfplay_openings(BOOK5, WEIGHTS5)
    A.debug_set_queue_cap(40)                                      # two or three games fill it
    rows, st = A.play(200, 40)                                     # ~every slot finishes its game
    games = collect(rows, A.play_row_metrics(), {})
    A.debug_set_queue_cap(0)
    g = A.get_games()
    parked = np.flatnonzero(g["result"] != 0)                      # a parked slot still holds its finished game
    assert 0 < len(rows["reward"]) <= 40 and len(parked) >= 4, (len(rows["reward"]), parked)
    harvest(A, np.arange(2 * G), games)
    slots = A.selfplay_openings_slots()
    assert (slots >= 0).all()
    none = lambda E: None
    equal_the_prefix_path(games, kind, BOOK5, WEIGHTS5, (0, 1), none, 5, G, seed, none)
    idx = index_of(seed, np.arange(2 * G), WEIGHTS5)
    for u in range(2 * G):
        assert np.array_equal(games[u]["board"][0], position(5, BOOK5[idx[u]])), u
    A.close()


# ---- 2. the 3-slot instantiation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, path", [("uniform", "k_play<3> (persistent)"), ("hash", "k_mcts<3,generic>")])
def test_the_three_slot_kernels_on_12x12(kind, path):
    book = [[], [70], [1, 144], [133, 12, 77], [140, 5, 66, 67]]
    A, _ = check_generations(kind, book, [1, 1, 2, 2, 2], (0, 1), n=12, G=8, sims=8, seed=77)
    assert path in A.kernel_info(), A.kernel_info()
    A.close()


# ---- 3. the resnet engine: the two half-pools (from 1024 slots on) and one stream ----------------------------------------
def net_weights(n=5, blocks=1, chans=64, seed=3):
    from azalea_amd.network import HexNetwork
    torch.manual_seed(seed)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).eval()
    return {k: v.detach().numpy() for k, v in net.state_dict().items()}


@pytest.mark.parametrize("pipeline", ["1", "0"])
def test_the_resnet_engine_and_both_half_pools_follow_the_book(pipeline, monkeypatch):
    monkeypatch.setenv("AZX_PIPELINE", pipeline)
    w = net_weights()
    G = 1024                                                       # the pool splits in two from 1024 slots on
    A, games = check_generations("resnet", BOOK5, WEIGHTS5, (0, 1), G=G, sims=8, seed=4096,
                                 setup=lambda E: E.set_weights(w), num_blocks=1, base_chans=64)
    assert ("two half-pools" in A.kernel_info()) == (pipeline == "1"), A.kernel_info()
    # both halves of the pool hold book games now, and both have restarted from it
    slots = A.selfplay_openings_slots()
    assert (slots[:G // 2] >= 0).all() and (slots[G // 2:] >= 0).all()
    st = A.selfplay_openings_stats()
    assert st["started"].sum() >= 2 * G and st["started"][4] == 0
    A.close()


# ---- 4. a registered external evaluator ---------------------------------------------------------------------------------
P4 = pow(0x01000193, 4, 1 << 32)


def uniform_hash_evaluator(cells=25):
    """The AZX_EVAL_UNIFORM_HASH stub on the device (tests/test_gpu_external_eval.py): value from the fnv1a of the
    board, priors 1/k."""
    inv = torch.tensor(table(cells), device=DEV)

    def evaluate(board, legal):
        b = board.reshape(len(board), -1).to(torch.int64)
        h = torch.full((len(b),), 0x811C9DC5, dtype=torch.int64, device=board.device)
        for c in range(b.shape[1]):
            h = ((h ^ b[:, c]) * P4) & 0xFFFFFFFF
        value = ((h & 0xFFFF).to(torch.float64) / 32768.0 - 1.0).to(torch.float32)
        k = (legal != 0).sum(1)
        prior = torch.where(legal != 0, inv[k][:, None], torch.zeros((), device=DEV))
        return value, prior
    return evaluate


def test_external_evaluator_self_play_follows_the_book():
    fn = uniform_hash_evaluator()
    A, _ = check_generations("external", BOOK5, WEIGHTS5, (0, 1), sims=8, seed=99,
                             setup=lambda E: E.set_external_evaluator(fn))
    A.close()


# ---- 5. no book: the same bytes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "hash"])
def test_no_book_a_cleared_book_and_the_empty_opening_play_the_same_bytes(kind):
    out = {}
    for name in ("never", "cleared", "empty"):
        E = make(kind, seed=5)
        if name == "cleared":
            E.set_selfplay_openings(BOOK5, WEIGHTS5)
            assert "book=6" in E.kernel_info()
            E.clear_selfplay_openings()
        if name == "empty":
            E.set_selfplay_openings([[]])
        assert ("book=1" if name == "empty" else "book=off") in E.kernel_info(), E.kernel_info()
        rows, st = E.play(300)
        met = E.play_row_metrics()
        out[name] = (rows, met, E.debug_counters_raw().copy(), st["plies"], E.get_games())
        assert (E.selfplay_openings_slots() == (0 if name == "empty" else -1)).all()
        E.close()
    base = out["never"]
    assert len(base[0]["reward"]) >= 300
    # finished games enter the harvest queue in the order the GPU finished them: compare game by game
    ib = np.argsort(base[0]["game_uid"], kind="stable")
    for name in ("cleared", "empty"):
        rows, met, ctr, plies, games = out[name]
        i = np.argsort(rows["game_uid"], kind="stable")
        for k in ROW_KEYS + ("game_uid",):
            assert rows[k][i].tobytes() == base[0][k][ib].tobytes(), (name, k)
        assert met[i].tobytes() == base[1][ib].tobytes() and ctr.tobytes() == base[2].tobytes() and plies == base[3], name
        for k in ("board", "color", "result", "ply"):
            assert np.array_equal(games[k], base[4][k]), (name, k)


# ---- 6. who is seated when ------------------------------------------------------------------------------------------------
def test_seating_semantics():
    seed, G, n = 31, 16, 5
    E = make("hash", seed=seed, G=G)
    mask = np.zeros(G, np.int32)
    mask[3] = 1
    E.set_active(mask)
    E.play_steps(1)                                                # slot 3 alone plays a ply: its game has begun
    E.set_active(np.ones(G, np.int32))
    before = E.get_games()
    assert before["ply"][3] == 1 and before["ply"].sum() == 1
    E.set_selfplay_openings(BOOK5, WEIGHTS5)
    idx = index_of(seed, np.arange(G), WEIGHTS5)

    def check(slot_uid, skip=()):
        g, s = E.get_games(), E.selfplay_openings_slots()
        for slot, u in slot_uid.items():
            if slot in skip:
                continue
            o = int(index_of(seed, [u], WEIGHTS5)[0])
            assert s[slot] == o, (slot, u)
            assert np.array_equal(g["board"][slot], position(n, BOOK5[o])) and g["ply"][slot] == len(BOOK5[o]), slot
            assert g["color"][slot] == (len(BOOK5[o]) & 1) and g["result"][slot] == 0, slot     # (0: colour 1 to move)
        return g, s
    uid = {g: g for g in range(G)}                                 # re-seating keeps the uid: generation 0
    g, s = check(uid, skip=(3,))
    assert s[3] == -1 and np.array_equal(g["board"][3], before["board"][3]) and g["ply"][3] == 1   # in progress: kept
    started = np.bincount(np.delete(idx, 3), minlength=len(BOOK5))
    assert np.array_equal(E.selfplay_openings_stats()["started"], started)
    # reset with a table wins for that game; reset without one seats under the book (both take the slot's next uid)
    E.reset(slots=[5], moves=[[9, 10]])
    E.reset(slots=[6])
    uid[5], uid[6] = G + 5, G + 6
    g, s = check(uid, skip=(3, 5))
    assert s[5] == -1 and np.array_equal(g["board"][5], position(n, [9, 10])) and g["ply"][5] == 2
    # replacing the book seats the fresh slots again (slot 5's table too: the last call wins) and zeroes the tallies
    book2 = [[2], [4, 6]]
    E.set_selfplay_openings(book2)
    s = E.selfplay_openings_slots()
    g = E.get_games()
    assert s[3] == -1 and g["ply"][3] == 1
    for slot in range(G):
        if slot != 3:
            o = int(index_of(seed, [uid[slot]], 2)[0])
            assert s[slot] == o and np.array_equal(g["board"][slot], position(n, book2[o])), slot
    st = E.selfplay_openings_stats()
    assert st["started"].sum() == G - 1 and st["finished"].sum() == 0 and st["plies"].sum() == 0
    # the games in slots 3 (begun before any book), 5 and 6 finish; their next games follow the book
    games = harvest(E, [3, G + 3, G + 5, 2 * G + 5, G + 6, 2 * G + 6])
    assert stones(games[3]["board"])[0] == 0                        # played from the empty board, as it began
    for u in (G + 3, G + 5, 2 * G + 5, G + 6, 2 * G + 6):
        o = int(index_of(seed, [u], 2)[0])
        assert np.array_equal(games[u]["board"][0], position(n, book2[o])), u
    E.close()


# ---- 7. the per-opening tallies ---------------------------------------------------------------------------------------------
def tally(games, idx_of, n_openings):
    fin, won, plies = (np.zeros(n_openings, np.int64) for _ in range(3))
    for u, g in games.items():
        o = idx_of(u)
        fin[o] += 1
        plies[o] += stones(g["board"])[-1] + 1                      # the last row's move ends the game
        mover1 = g["color"][-1] == 0                                # colour 1 moves at the even plies
        won[o] += int((g["reward"][-1] > 0) == mover1)
    return fin, won, plies


def test_the_tallies_are_what_the_harvested_games_imply():
    seed, G = 20261020, 16
    E = make("uniform", seed=seed, G=G)
    E.set_selfplay_openings(BOOK5, WEIGHTS5)
    games = {}
    total = 0.0
    for _ in range(6):
        before = set(games)
        rows, st = E.play(200)
        total += st["sum_game_length"]
        uid = rows["game_uid"]
        starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
        for s, e in zip(starts, np.r_[starts[1:], len(uid)]):
            games[int(uid[s])] = {k: rows[k][s:e] for k in ROW_KEYS}
        assert st["games"] == len(set(games) - before)
    fin, won, plies = tally(games, lambda u: int(index_of(seed, [u], WEIGHTS5)[0]), len(BOOK5))
    st = E.selfplay_openings_stats()
    assert np.array_equal(st["finished"], fin) and np.array_equal(st["wins_color1"], won)
    assert np.array_equal(st["plies"], plies) and plies.sum() == total      # plies count from the empty board
    live = E.selfplay_openings_slots()
    assert (live >= 0).all()
    assert np.array_equal(st["started"], fin + np.bincount(live, minlength=len(BOOK5)))
    assert fin.sum() >= 60 and fin[4] == 0 and 0 < won.sum() < fin.sum()
    E.close()


def test_a_game_dropped_for_search_tree_full_counts_as_started_only():
    """Arenas around the size of a first 7x7 search make SOME games overflow in the ordinary course of play, as in
    tests/test_gpu_round2.py (a game from a one-ply opening needs a little less: 48 legal moves)."""
    from azalea_amd import engine as eng
    n, G, sims = 7, 64, 30
    book = eng.all_openings(n, 1)
    st = None
    for cap in (1950, 1935, 1920, 1905, 1890, 1875, 1860, 1845):
        E = eng.Engine(board_size=n, n_games=G, simulations=sims, search_batch_size=10, exploration_depth=4,
                       evaluator=eng.EVAL_UNIFORM, nodes_per_game=cap, seed=77)
        E.set_selfplay_openings(book)
        rows, st = E.play(600, max_plies=400)
        bs = E.selfplay_openings_stats()
        live = E.selfplay_openings_slots()
        E.close()
        if st["game_errors"] > 0 and st["games"] > 0:
            break
    assert st["game_errors"] > 0 and st["games"] > 0, (cap, st["game_errors"], st["games"])
    assert bs["finished"].sum() == st["games"]
    assert bs["started"].sum() == st["games"] + st["game_errors"] + (live >= 0).sum()
    assert (live >= 0).all()


# ---- 8. composition with the other self-play options --------------------------------------------------------------------------
def cap_resign_gumbel(E):
    E.set_playout_cap(0.6, 8)
    E.set_resign(-0.6, 4, 0.25)
    E.set_gumbel(4, 50.0, 1.0, True)


def estop_forced_targets(E):
    E.set_early_stop(True)
    E.set_forced_playouts(2.0, True)
    E.set_train_targets("visits", 0.5)


@pytest.mark.parametrize("options", [cap_resign_gumbel, estop_forced_targets])
@pytest.mark.parametrize("kind", ["uniform", "hash"])
def test_the_book_composes_with_the_other_options(kind, options):
    """The rows of a capped game are its full plies only, and a resigned game is short: the generic checks of
    check_generations on row counts do not hold under a cap, so the comparison is made here directly."""
    seed, G = 1234, 16
    A = make(kind, seed=seed, G=G, sims=32)
    A.set_selfplay_openings(BOOK5, WEIGHTS5)
    options(A)
    uids = np.arange(0, 2 * G)
    games = harvest_any(A, uids)
    for t in (0, 1):
        B = make(kind, seed=seed + (t - 1) * G, G=G, sims=32)
        options(B)
        gu = np.arange(t * G, (t + 1) * G)
        B.reset(moves=[BOOK5[o] for o in index_of(seed, gu, WEIGHTS5)])
        ref = harvest_any(B, np.arange(G, 2 * G))
        for g in range(G):
            a, b = games.get(t * G + g), ref.get(G + g)
            assert (a is None) == (b is None), (t, g)               # (a capped game may record no row at all)
            if a is not None:
                same_game(a, b, (t, g))
                o = int(index_of(seed, [t * G + g], WEIGHTS5)[0])
                assert stones(a["board"])[0] >= len(BOOK5[o]), (t, g)
        B.close()
    assert len(games) >= G
    A.close()


def harvest_any(E, want, limit=400):
    """harvest() for runs in which a game may be harvested without a row (a playout cap): play until the slots have
    moved past the wanted uids -- every slot's games come in uid order -- and return what was recorded."""
    games = {}
    want = np.asarray(want, np.int64)
    G = E.G
    for _ in range(limit):
        rows, st = E.play(1)
        met = E.play_row_metrics()
        uid = rows["game_uid"]
        starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]]) if len(uid) else []
        for s, e in zip(starts, np.r_[starts[1:], len(uid)]):
            assert int(uid[s]) not in games
            games[int(uid[s])] = dict({k: rows[k][s:e].copy() for k in ROW_KEYS}, metrics=met[s:e].copy())
        last = {}                                                  # per slot, the newest uid seen harvested
        for u in games:
            last[u % G] = max(last.get(u % G, -1), u)
        if all(last.get(int(u) % G, -1) > int(u) for u in want):
            return {u: g for u, g in games.items() if u in set(want.tolist())}
    raise AssertionError("the slots never moved past the wanted games")


# ---- 9. sharding ------------------------------------------------------------------------------------------------------------
def test_two_shards_play_the_games_of_one_engine():
    seed = 555
    one = make("hash", seed=seed, G=16)
    one.set_selfplay_openings(BOOK5, WEIGHTS5)
    whole = harvest(one, np.arange(32))
    one.close()
    for offset in (0, 1):
        E = make("hash", seed=seed, G=8, game_index_stride=2, game_index_offset=offset)
        E.set_selfplay_openings(BOOK5, WEIGHTS5)
        uids = np.arange(offset, 32, 2)
        assert np.array_equal(E.selfplay_openings_slots(), index_of(seed, uids[:8], WEIGHTS5))
        part = harvest(E, uids)
        for u in uids.tolist():
            same_game(part[u], whole[u], u)
        E.close()


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------
def test_matches_and_tournaments_refuse_an_engine_with_a_book():
    from azalea_amd import engine as eng
    a, b = make("hash", seed=6), make("hash", seed=7)
    b.set_selfplay_openings(BOOK5)
    m = eng.Match(a, b)
    with pytest.raises(Exception, match="engine b has a self-play opening book set"):
        m.play(4)
    t = eng.Tournament([a, b])
    with pytest.raises(Exception, match="engine 1 has a self-play opening book set"):
        t.play([(0, 1)], 2)
    b.clear_selfplay_openings()
    assert m.play(4)["stats"]["games"] == 4                                  # cleared: the match plays
    m.close()
    t.close()
    a.close()
    b.close()


def test_a_bad_book_leaves_the_previous_one_playing():
    seed, G = 808, 16
    E = make("hash", seed=seed, G=G)
    E.set_selfplay_openings(BOOK5, WEIGHTS5)
    for bad, w, word in (([[1, 1]], None, "tile 0 is played twice"), ([[26]], None, "outside [1, 25]"),
                         ([[1, 2, 6, 3, 11, 4, 16, 7, 21]], None, "decides the game"),
                         ([[1], [2]], [0.0, 0.0], "all zero"), ([[1], [2]], [1.0, -1.0], "is negative"),
                         ([[1], [2]], [1.0, float("nan")], "is not finite")):
        with pytest.raises(ValueError, match=re.escape(word)):
            E.set_selfplay_openings(bad, w)
        assert "book=6" in E.kernel_info()
    with pytest.raises(ValueError, match="1 weights for 2 openings"):
        E.set_selfplay_openings([[1], [2]], [1.0])
    assert np.array_equal(E.selfplay_openings_slots(), index_of(seed, np.arange(G), WEIGHTS5))
    games = harvest(E, np.arange(2 * G))
    for u, g in games.items():
        o = int(index_of(seed, [u], WEIGHTS5)[0])
        assert np.array_equal(g["board"][0], position(5, BOOK5[o])), u
    E.close()


# ---- 11. the Player -------------------------------------------------------------------------------------------------------------
SEARCH = dict(simulations=8, search_batch_size=4, exploration_coef=0.5, exploration_depth=3,
              exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0)


def test_player_reads_games_that_start_at_book_positions(monkeypatch):
    from azalea_amd import parallel_player
    from azalea_amd.azalea_agent import AzaleaAgent
    from azalea_amd.game.hex import HexGame
    from azalea_amd.policy import Policy
    seen = []
    to_frame = parallel_player.rows_to_frame

    def spy(rows):
        seen.append(rows)
        return to_frame(rows)
    monkeypatch.setattr(parallel_player, "rows_to_frame", spy)
    torch.manual_seed(1)
    policy = Policy()
    policy.initialize(dict(device="cuda:0", network="HexNetwork", board_size=5, num_blocks=1, base_chans=16, seed=1,
                           **SEARCH))
    agent = AzaleaAgent(partial(HexGame, board_size=5), policy=policy, device="cuda:0")
    player = parallel_player.Player(None, [agent], n_games=64, selfplay_openings=BOOK5,
                                    selfplay_opening_weights=WEIGHTS5)
    assert player.opening_stats() is None                          # no engine yet
    frame, metrics = player.read(300)
    assert len(seen) == 1 and len(frame) == len(seen[0]["reward"]) >= 300
    rows = seen[0]
    assert "book=6" in player._engine.kernel_info()
    seed = player._seed_base
    uid = rows["game_uid"]
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
    fin = np.zeros(len(BOOK5), np.int64)
    for s in starts:
        o = int(index_of(seed, [uid[s]], WEIGHTS5)[0])
        assert np.array_equal(rows["board"][s], position(5, BOOK5[o])), uid[s]
        fin[o] += 1
    assert (fin > 0).sum() >= 4 and fin[4] == 0 and fin.sum() == metrics["games"]
    # the tallies cover the frame's games and the whole games the player holds for the next read
    for held, _ in player._games:
        fin[int(index_of(seed, [held["game_uid"][0]], WEIGHTS5)[0])] += 1
    st = player.opening_stats()
    assert np.array_equal(st["finished"], fin)
    assert st["started"].sum() == fin.sum() + 64
    player.stop()
