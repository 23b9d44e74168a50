"""Training targets of the recorded self-play rows on the device (azx_set_train_targets: visit-share policy rows and
z/q-blended rewards; NOT the reference's behaviour, off by default).  The numpy twins are
tests/train_targets_reference.py's.  Every case plays 5x5 boards; the main cases 16 slots, 40 simulations in batches of
5, exploration_depth 3, temperature 1 and device noise, until about 40 games are harvested: the smallest shape at
which plies drawn at T = 1 (ply < 3) and greedy plies both occur in every game.

The option never touches the move draw, so an engine with the option on plays the games of its twin with the option
off, move for move: every case compares such a pair row by row, the rows sorted by game uid (finished games enter the
queue in the order the GPU finished them)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_targets_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N, CELLS, G = 5, 25, 16
SIMS, BS, DEPTH = 40, 5, 3
NB = SIMS // BS + 1
ROWS = 600                                  # about 40 games of 15 rows
EINVAL = -1
STAT_KEYS = ("rows", "greedy_rows", "greedy_rows_wide")
# The share of greedy rows with more than one visited child, below which the visit-share cases would pass vacuously (a
# one-child row IS the reference's one-hot row).  A 45-select search with Dirichlet noise on a root of two or more
# children visits a second child unless one move decides the game, which on 5x5 holds only in a game's last plies:
# half of the greedy rows is a floor far below what such games give, and far above nothing.  It is asserted on the OFF
# engine's root widths (row metric 1), which the option does not touch.
MIN_WIDE_SHARE = 0.5


def make(evaluator, n_games=G, sims=SIMS, bs=BS, seed=4242, **kw):
    from azalea_amd import engine as eng
    cfg = dict(board_size=N, n_games=n_games, simulations=sims, search_batch_size=bs, exploration_coef=1.0,
               exploration_depth=DEPTH, noise_alpha=0.3, noise_scale=0.25, temperature=1.0, seed=seed)
    cfg.update(kw)
    return eng.Engine(evaluator=evaluator, **cfg)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def stones(board):
    return (np.asarray(board).reshape(len(board), CELLS) != 0).sum(1)


class Run:
    """Rows and row metrics of one call, sorted by game uid (stable: a game's rows stay in ply order)."""

    def __init__(self, rows, m, st=None):
        assert len(m) == len(rows["reward"])
        i = np.argsort(rows["game_uid"], kind="stable")
        self.rows = {k: v[i] for k, v in rows.items()}
        self.m = m[i]
        self.st = st
        self.ply = stones(self.rows["board"])
        self.k = self.rows["nlegal"].astype(np.int64)
        uid = self.rows["game_uid"]
        self.starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
        self.ends = np.r_[self.starts[1:], len(uid)]
        for s, e in zip(self.starts, self.ends):            # plies ascending inside a game, metric 3 flags its first row
            assert (np.diff(self.ply[s:e]) > 0).all()
            assert self.m[s, 3] == 1.0 and (self.m[s + 1:e, 3] == 0.0).all()

    @classmethod
    def play(cls, E, min_positions=ROWS, max_plies=0):
        rows, st = E.play(min_positions, max_plies=max_plies)
        return cls(rows, E.play_row_metrics(), st)

    def __len__(self):
        return len(self.ply)


def counts_of(run):
    """The root children's visit counts recovered from visit-share rows: (n int64[rows, CELLS], S int64[rows])."""
    S = np.rint(run.m[:, 4].astype(np.float64) * run.k).astype(np.int64)        # metric 4 = sum(counts) / k in float32
    n = np.rint(run.rows["moves_prob"].astype(np.float64) * S[:, None]).astype(np.int64)
    return n, S


def stats_of(run, greedy=None):
    greedy = run.ply >= DEPTH if greedy is None else greedy
    return dict(rows=len(run), greedy_rows=int(greedy.sum()), greedy_rows_wide=int((greedy & (run.m[:, 1] > 1)).sum()))


def check_pair(A, B, visits, mix, a_metric7_zero=True, metric0=True):
    """A: the run with the option off, B: its twin with (policy_rows, value_mix) = ("visits" if visits else
    "reference", mix).  Everything the issue lists, row for row."""
    assert len(A) == len(B) > 0
    for key in ("board", "color", "nlegal", "game_uid"):
        assert np.array_equal(A.rows[key], B.rows[key]), key            # the games are the same games
    cols = [0, 1, 2, 3, 4, 5, 6] if metric0 else [1, 2, 3, 4, 5, 6]
    assert np.array_equal(bits(A.m[:, cols]), bits(B.m[:, cols]))
    z = A.rows["reward"]
    if a_metric7_zero:
        assert (bits(A.m[:, 7]) == 0).all() and (np.abs(z) == 1).all()
    greedy = B.ply >= DEPTH
    assert greedy.any() and (~greedy).any()
    # ---- the policy rows ----
    if visits:
        early = ~greedy
        assert np.array_equal(bits(A.rows["moves_prob"][early]), bits(B.rows["moves_prob"][early]))     # T = 1 plies: as they were
        n, S = counts_of(B)
        assert (S > 0).all() and np.array_equal(n.sum(1), S)
        assert (n[np.arange(CELLS)[None, :] >= B.k[:, None]] == 0).all()                       # nothing beyond the k children
        assert np.array_equal((n > 0).sum(1), B.m[:, 1].astype(np.int64))                      # metric 1: the root's width
        assert np.array_equal(bits(ref.visit_rows(n)), bits(B.rows["moves_prob"]))             # ONE float32 division
        # the off engine's greedy row is one-hot (uniform over ties) on exactly the most-visited children
        top = n == n.max(1, keepdims=True)
        assert np.array_equal((A.rows["moves_prob"] > 0)[greedy], top[greedy])
    else:
        assert np.array_equal(bits(A.rows["moves_prob"]), bits(B.rows["moves_prob"]))
    # ---- metric 7 and the reward ----
    v = B.m[:, 7]
    assert np.isfinite(v).all() and (np.abs(v) <= 1).all()
    assert np.array_equal(bits(B.rows["reward"]), bits(ref.blend(z, v, mix)))
    if mix == 1.0:
        assert np.array_equal(B.rows["reward"], v)
    if mix > 0:
        assert (B.rows["reward"] != z).any()                   # ... and the blend is not vacuous
    return greedy


# ---- 1. off is the parent's bytes -----------------------------------------------------------------------------------
def test_off_never_set_cleared_or_set_to_off_is_the_same_bytes():
    from azalea_amd import engine as eng
    out = []
    for how in ("never", "cleared", "cleared_by_pair", "set_off"):
        E = make(eng.EVAL_UNIFORM_HASH)
        if how == "cleared":
            E.set_train_targets("visits", 0.5)
            assert "targets=visits/0.5" in E.kernel_info() and E.train_targets() == ("visits", 0.5)
            E.clear_train_targets()
        elif how == "cleared_by_pair":
            E.set_train_targets("reference", 1.0)
            assert "targets=reference/1" in E.kernel_info()
            E.set_train_targets()
        elif how == "set_off":
            E.set_train_targets("reference", 0.0)
        assert E.train_targets() == ("reference", 0.0) and "targets=off" in E.kernel_info()
        info = E.kernel_info()
        R = Run.play(E)
        out.append(({k: v.tobytes() for k, v in R.rows.items()}, R.m.tobytes(),
                    {k: v for k, v in R.st.items() if not k.endswith("seconds")}, E.debug_counters_raw().tobytes(), info))
        assert (bits(R.m[:, 7]) == 0).all()
        assert E.train_targets_stats() == dict.fromkeys(STAT_KEYS, 0)
        E.close()
    assert out[0] == out[1] == out[2] == out[3]


# ---- 2. visit-share rows --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def off_run():
    """The run of the engine with the option off: the reference of cases 2 and 3 (shared, never modified)."""
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM_HASH)
    R = Run.play(E)
    E.close()
    assert len(R.starts) >= 30
    return R


def test_visits_rows_are_the_visit_shares_of_the_same_games(off_run):
    from azalea_amd import engine as eng
    A = off_run
    greedy_a = A.ply >= DEPTH
    share = ((A.m[:, 1] > 1) & greedy_a).sum() / greedy_a.sum()
    print("greedy rows %d of %d, share with more than one visited child %.3f" % (greedy_a.sum(), len(A), share))
    assert share >= MIN_WIDE_SHARE
    E = make(eng.EVAL_UNIFORM_HASH)
    E.set_train_targets("visits")
    B = Run.play(E)
    s1, ply1 = E.train_targets_stats(), E.get_games()["ply"].astype(np.int64)
    # the statistics count every row written, the rows of the games still under way included: those games are the
    # first game of each slot that a second call harvests (uid = slot + G * generation)
    B2 = Run.play(E)
    E.close()
    greedy = check_pair(A, B, visits=True, mix=0.0)
    # with mix 0 the reward is z itself and the rows that differ from the reference's are the wide greedy rows
    differ = (bits(A.rows["moves_prob"]) != bits(B.rows["moves_prob"])).any(1)
    assert np.array_equal(differ, greedy & (B.m[:, 1] > 1))
    want = stats_of(B)
    for g in range(G):
        if ply1[g] == 0:
            continue
        first = min(int(u) for u in B2.rows["game_uid"] if u % G == g)
        assert first not in set(B.rows["game_uid"].tolist())
        i = np.flatnonzero(B2.rows["game_uid"] == first)[:ply1[g]]
        assert np.array_equal(B2.ply[i], np.arange(ply1[g]))               # its first ply1 rows were written in call 1
        gr = B2.ply[i] >= DEPTH
        want["rows"] += len(i)
        want["greedy_rows"] += int(gr.sum())
        want["greedy_rows_wide"] += int((gr & (B2.m[i, 1] > 1)).sum())
    assert s1 == want and s1["rows"] == B.st["plies"]


# ---- 3. the blend ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", [0.5, 1.0, 0.3])
def test_the_reward_is_the_blend_of_z_and_the_roots_value(off_run, mix):
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM_HASH)
    E.set_train_targets("reference", mix)
    C = Run.play(E)
    st = E.train_targets_stats()
    E.close()
    check_pair(off_run, C, visits=False, mix=mix)
    assert C.st["sum_reward_last"] == off_run.st["sum_reward_last"]         # metrics['reward'] keeps summing z
    assert st["rows"] == C.st["plies"] and st["greedy_rows_wide"] <= st["greedy_rows"] < st["rows"]


def test_with_resignation_metric_7_is_the_same_float_and_resigned_games_blend_the_conceded_z():
    from azalea_amd import engine as eng
    runs, rs = [], []
    for mix in (None, 0.5):
        E = make(eng.EVAL_UNIFORM_HASH)
        E.set_resign(0.0, 4, 0.0)                              # hash values sit around 0: many judged plies resign
        if mix is not None:
            E.set_train_targets("reference", mix)
        runs.append(Run.play(E))
        rs.append(E.resign_stats())
        E.close()
    A, C = runs
    assert rs[0] == rs[1] and rs[0]["resigned"] > 0
    assert np.array_equal(bits(A.m[:, 7]), bits(C.m[:, 7]))                # the same float resignation stores there
    check_pair(A, C, visits=False, mix=0.5, a_metric7_zero=False)
    # the last row of a game won on the board belongs to the winner (z = +1); that of a resigned game to the resigner
    last = A.ends - 1
    resigned = A.rows["reward"][last] == -1.0
    assert resigned.sum() == rs[0]["resigned"]
    lr = last[resigned]
    assert (A.m[lr, 7] < 0.0).all() and (A.ply[lr] >= 4).all()
    assert np.array_equal(bits(C.rows["reward"][lr]), bits(ref.blend(np.full(len(lr), -1.0), C.m[lr, 7], 0.5)))


# ---- 4. every play path ---------------------------------------------------------------------------------------------
def pair_on_path(engine, play=Run.play):
    """An off engine and its ("visits", 0.5) twin from the same factory; returns (A, B, statistics of B)."""
    out = []
    for on in (False, True):
        E = engine()
        if on:
            E.set_train_targets("visits", 0.5)
            assert "targets=visits/0.5" in E.kernel_info()
        out.append(play(E))
        st = E.train_targets_stats()
        E.close()
    return out[0], out[1], st


@pytest.mark.parametrize("path", ["persistent", "no_persistent", "generic"])
def test_the_inline_paths(path, monkeypatch):
    from azalea_amd import engine as eng
    if path == "no_persistent":
        monkeypatch.setenv("AZX_NO_PERSISTENT", "1")          # (read by azx_create)
    elif path == "generic":
        monkeypatch.setenv("AZX_MCTS_GENERIC", "1")

    def engine():
        E = make(eng.EVAL_UNIFORM)
        info = E.kernel_info()
        assert ("k_play<2> (persistent)" in info) == (path == "persistent"), info
        assert ("FAST" in info) == (path != "generic"), info
        return E
    A, B, st = pair_on_path(engine)
    check_pair(A, B, visits=True, mix=0.5)
    assert st["rows"] == B.st["plies"] and st["rows"] >= len(B)


def test_replay_fill_hands_the_ring_the_blended_rewards_and_visit_rows():
    from azalea_amd import engine as eng
    ring = {}

    def fill(E):
        E.replay_create(4096)
        rows, st = E.replay_fill(ROWS)
        assert E.replay_state()["size"] == rows
        out = dict(color=torch.empty(rows, dtype=torch.int64, device=DEV),
                   legal_moves=torch.empty((rows, CELLS), dtype=torch.int32, device=DEV),
                   result=torch.empty(rows, dtype=torch.int64, device=DEV),
                   board=torch.empty((rows, CELLS), dtype=torch.int32, device=DEV),
                   moves_prob=torch.empty((rows, CELLS), dtype=torch.float32, device=DEV),
                   reward=torch.empty(rows, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize(DEV)
        E.replay_collate(np.arange(rows), {k: t.data_ptr() for k, t in out.items()})
        q = E.rows_read(0, rows)                               # the harvest queue the ring was filled from, in ring order
        ring[len(ring)] = (q, {k: t.cpu().numpy() for k, t in out.items()})
        return Run(q, E.play_row_metrics(rows), st)
    A, B, st = pair_on_path(lambda: make(eng.EVAL_UNIFORM_HASH), fill)
    check_pair(A, B, visits=True, mix=0.5)
    q, col = ring[1]                                           # what replay_collate hands out of the option's ring
    assert np.array_equal(bits(col["moves_prob"]), bits(q["moves_prob"]))
    assert np.array_equal(bits(col["reward"]), bits(q["reward"]))
    assert np.array_equal(col["board"], q["board"].reshape(-1, CELLS)) and np.array_equal(col["color"], q["color"])


def test_a_registered_external_evaluator():
    from azalea_amd import engine as eng
    inv = torch.tensor(np.float32(1.0) / np.arange(0, CELLS + 1).clip(1).astype(np.float32), device=DEV)

    def evaluate(board, legal):                                   # uniform priors, a value from the stones' positions
        k = (legal != 0).sum(1)
        prior = torch.where(legal != 0, inv[k][:, None], torch.zeros((), device=DEV))
        wts = torch.arange(1, CELLS + 1, dtype=torch.float32, device=DEV)
        value = torch.tanh(((board.reshape(len(board), -1) == 1).float() * wts).sum(1) * 0.37 - 3.0)
        return value.to(torch.float32), prior

    def engine():
        E = make(eng.EVAL_EXTERNAL, seed=99)
        E.set_external_evaluator(evaluate)
        return E
    A, B, st = pair_on_path(engine, lambda E: Run.play(E, 300))
    check_pair(A, B, visits=True, mix=0.5)
    assert st["rows"] == B.st["plies"]


def test_the_two_half_pools_of_a_network():
    from azalea_amd import engine as eng
    from azalea_amd.network import HexNetwork
    torch.manual_seed(3)
    net = HexNetwork(board_size=N, num_blocks=1, base_chans=16).eval()
    w = {k: v.detach().numpy() for k, v in net.state_dict().items()}

    def engine():
        E = make(eng.EVAL_RESNET, n_games=1024, sims=20, seed=2024, num_blocks=1, base_chans=16)
        E.set_weights(w)
        assert "two half-pools" in E.kernel_info(), E.kernel_info()            # the pipeline runs
        return E
    A, B, st = pair_on_path(engine, lambda E: Run.play(E, 4096, max_plies=16))  # a handful of plies: the shortest games
    check_pair(A, B, visits=True, mix=0.5)
    slot = B.rows["game_uid"] % 1024
    assert (slot >= 512).any() and (slot < 512).any()          # rows of both half-pools
    assert st["rows"] == B.st["plies"]


# ---- 5. beside the other options ------------------------------------------------------------------------------------
def test_under_a_playout_cap_fast_plies_record_nothing():
    from azalea_amd import engine as eng
    seed, p = 4242, 0.5

    def engine():
        E = make(eng.EVAL_UNIFORM_HASH, seed=seed)
        E.set_playout_cap(p, 20)
        return E
    A, B, st = pair_on_path(engine)
    check_pair(A, B, visits=True, mix=0.5)
    # a game's recorded plies are exactly its full plies (up to its last recorded one)
    fast_seen = 0
    for s, e in zip(B.starts, B.ends):
        uid, plies = int(B.rows["game_uid"][s]), B.ply[s:e].tolist()
        full = [q for q in range(plies[-1] + 1) if eng.playout_cap_is_full(seed, uid, q, p)]
        assert plies == full
        fast_seen += plies[-1] + 1 - len(full)
    assert fast_seen > 0
    assert st["rows"] >= len(B) and st["rows"] < B.st["plies"]                  # fewer rows than plies


def test_under_early_stop_the_row_is_the_visit_shares_at_the_stop():
    """64 slots start at 4-stone positions with fresh trees, so the first recorded row of each slot's first game is a
    greedy ply whose root children hold exactly the visits of this ply's selects: under early stop a stopped ply's
    counts sum to less than the full search's, and the row is still visit_rows of them."""
    from azalea_amd import engine as eng
    rng = np.random.RandomState(5)
    prefixes = [[int(c) for c in rng.permutation(CELLS)[:4] + 1] for _ in range(64)]
    firsts = {}
    for estop in (False, True):
        runs = []
        for targets in (False, True):
            E = make(eng.EVAL_UNIFORM_HASH, n_games=64, seed=7)
            E.reset(moves=prefixes)
            if estop:
                E.set_early_stop(True)
            if targets:
                E.set_train_targets("visits", 0.5)
            runs.append(Run.play(E, 900))
            es = E.early_stop_stats()
            E.close()
        A, B = runs
        check_pair(A, B, visits=True, mix=0.5)                 # (under early stop too: both engines stop alike)
        n, S = counts_of(B)
        uid = B.rows["game_uid"]
        firsts[estop] = {}
        for g in range(64):                                    # the slot's first game (uid = slot + 64 * generation), if harvested
            mine = uid[uid % 64 == g]
            if len(mine):
                i = np.flatnonzero(uid == mine.min())[0]
                assert B.ply[i] == 4 and B.m[i, 3] == 1.0
                firsts[estop][g] = int(S[i])
        if estop:
            assert es["stopped_plies"] > 0
    both = sorted(set(firsts[False]) & set(firsts[True]))
    assert len(both) >= 32
    full, stopped = (np.array([firsts[e][g] for g in both]) for e in (False, True))
    print("selects behind the first rows: full %s, under early stop %s" % (sorted(set(full.tolist())), sorted(stopped.tolist())))
    assert len(set(full.tolist())) == 1 and full[0] in (NB * BS, NB * BS - 1)   # (less one where the first select expands the root)
    assert (stopped <= full).all() and (stopped < full).sum() >= 1


# ---- 6. refusals ----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_einval_and_leave_the_setting_in_place():
    import ctypes as C
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM)
    L = E.L
    E.set_train_targets("visits", 0.25)
    rows, mix = C.c_int(-1), C.c_float(-1.0)
    for bad in ((2, 0.5), (-1, 0.5), (1, 1.5), (1, -0.01), (0, float("nan")), (1, float("inf"))):
        assert L.azx_set_train_targets(E.h, *bad) == EINVAL and b"train targets" in L.azx_last_error()
        assert L.azx_get_train_targets(E.h, C.byref(rows), C.byref(mix)) == 0
        assert (rows.value, mix.value) == (1, 0.25)
        assert E.train_targets() == ("visits", 0.25) and "targets=visits/0.25" in E.kernel_info()
    assert L.azx_set_train_targets(None, 1, 0.5) == EINVAL
    assert L.azx_get_train_targets(E.h, None, C.byref(mix)) == EINVAL
    assert L.azx_train_targets_stats(E.h, None) == EINVAL
    for bad in (("shares", 0.5), ("visits", 2.0), ("visits", float("nan"))):
        with pytest.raises(ValueError, match="train targets"):
            E.set_train_targets(*bad)
    assert E.train_targets() == ("visits", 0.25)
    E.clear_train_targets()
    assert E.train_targets() == ("reference", 0.0) and "targets=off" in E.kernel_info()
    E.close()


def test_matches_and_tournaments_refuse_the_option_before_touching_any_engine():
    import ctypes as C
    from azalea_amd import engine as eng
    from azalea_amd._lib import MatchStats
    a, b = (make(eng.EVAL_UNIFORM_HASH, n_games=64, sims=16, bs=4, seed=s, exploration_depth=4) for s in (6, 7))
    for e in (a, b):
        e.play(40)                                            # rows in both harvest queues, games under way in the slots
    m, t = eng.Match(a, b), eng.Tournament([a, b])
    L = a.L

    def state():
        out = []
        for e in (a, b):
            g = e.get_games()
            out.append((g["board"].tobytes(), g["ply"].tobytes(), e.get_root()["root_visits"].tobytes(),
                        {k: v.tobytes() for k, v in e.rows_read(0, e._last_rows).items()}))
        return out
    before = state()
    outcome, length = np.zeros(4, np.int8), np.zeros(4, np.int16)
    pa, pb = np.zeros(1, np.int32), np.ones(1, np.int32)
    p8, p16, p32 = (lambda x: x.ctypes.data_as(C.POINTER(C.c_int8)), lambda x: x.ctypes.data_as(C.POINTER(C.c_int16)),
                    lambda x: x.ctypes.data_as(C.POINTER(C.c_int32)))
    for on, name, idx, setting in ((b, "b", 1, ("visits", 0.0)), (a, "a", 0, ("reference", 0.5))):
        on.set_train_targets(*setting)
        st = MatchStats()
        assert L.azx_match_play(m.h, 0, 4, p8(outcome), p16(length), None, C.byref(st)) == EINVAL
        assert ("engine %s has training targets set" % name).encode() in L.azx_last_error()
        sts = (MatchStats * 1)()
        assert L.azx_tournament_play(t.h, 1, p32(pa), p32(pb), 0, 4, 4, p8(outcome), p16(length), None, sts) == EINVAL
        assert ("engine %d has training targets set" % idx).encode() in L.azx_last_error()
        with pytest.raises(ValueError, match="engine %d has training targets" % idx):
            m.play(4)
        with pytest.raises(ValueError, match="engine %d has training targets" % idx):
            t.play([(0, 1)], 4)
        assert state() == before                              # both engines' slots and queues are as they were
        assert on.train_targets() == setting
        on.clear_train_targets()
    res = m.play(8)                                           # after clearing, it plays
    assert (res["outcome"] != 0).all() and (res["length"] >= 9).all()
    m.close()
    t.close()
    a.close()
    b.close()


# ---- 7. Player and train() ------------------------------------------------------------------------------------------
SEARCH = dict(simulations=SIMS, search_batch_size=BS, exploration_coef=1.0, exploration_depth=DEPTH,
              exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0)


def cuda_policy():
    from azalea_amd.policy import Policy
    torch.manual_seed(1)
    policy = Policy()
    policy.initialize(dict(device="cuda:0", network="HexNetwork", board_size=N, num_blocks=1, base_chans=16, seed=1,
                           **SEARCH))
    return policy


def test_player_sets_the_option_on_its_engine():
    from functools import partial
    from azalea_amd import parallel_player
    from azalea_amd.azalea_agent import AzaleaAgent
    from azalea_amd.game.hex import HexGame
    agent = AzaleaAgent(partial(HexGame, board_size=N), policy=cuda_policy(), device="cuda:0")
    player = parallel_player.Player(None, [agent], n_games=64, train_targets={"policy_rows": "visits", "value_mix": 0.5})
    assert player.train_targets_stats() is None
    frame, metrics = player.read(200)
    E = player._engine
    assert E.train_targets() == ("visits", 0.5) and "targets=visits/0.5" in E.kernel_info()
    st = player.train_targets_stats()
    player.stop()
    assert len(frame) >= 200 and st["rows"] >= len(frame) and st["greedy_rows_wide"] > 0


def test_a_two_step_train_runs_under_the_option(tmp_path, monkeypatch):
    from azalea_amd.parallel_player import Player
    from azalea_amd.policy_trainer import train
    config = dict(seed=1, device="cuda:0", game="azalea_amd.game.hex.HexGame", board_size=N, replaybuf_size=256,
                  replaybuf_oversampling=1.0, batch_size=64, lr_initial=0.05, lr_decay=0.1, lr_decay_epochs=1,
                  momentum=0.9, l2_regularization=1e-4, total_epochs=2, selfplay_games=64, log_interval=1,
                  model_checkpoint_interval=0, train_targets=("visits", 0.5))
    infos, players = [], []
    stop = Player.stop

    def stop_and_tell(player):                  # train() stops its players at the end: ask their engines first
        players.append(player.train_targets)
        if player.train_targets is not None:    # (not the random-mover player that fills the first buffer)
            infos.append((player.device_engine().kernel_info(), player.train_targets_stats()))
        stop(player)
    monkeypatch.setattr(Player, "stop", stop_and_tell)
    path = train(cuda_policy(), config, str(tmp_path))
    assert os.path.exists(path)
    assert players.count(None) >= 1 and players.count(("visits", 0.5)) == 1, players
    assert len(infos) == 1 and "targets=visits/0.5" in infos[0][0], infos
    assert infos[0][1]["rows"] > 0 and infos[0][1]["greedy_rows_wide"] > 0
