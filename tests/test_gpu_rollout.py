"""The rollout evaluator on the device (azx_set_rollout_evaluator; NOT the reference's behaviour): the kernel alone
against the host definition, whole searches against the host phase API fed by that definition, registration, a strength
sanity match against a search that only sees terminal nodes, and evaluate_throughput with a RolloutNet agent."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollout_reference as ref  # noqa: E402

SIZES = (2, 3, 5, 8, 9, 11, 13)
SEED = 0x1234_5678_9ABC_DEF1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def boards_of(N):
    """The CPU tests' positions of this size: the random family, then the hand-built full boards."""
    out = [b for _, b in ref.position_family(N)]
    out += [b for _, b, _ in ref.full_boards(N)]
    return np.stack(out).astype(np.int32)


def host(boards, R, seed=SEED):
    from azalea_amd import engine
    res = [engine.rollout_value(seed, b, R) for b in boards]
    return np.array([w for w, _ in res], np.int32), np.array([v for _, v in res], np.float32)


def check_against_host(boards, N, R, seed=SEED):
    from azalea_amd import engine
    n, cells = len(boards), N * N
    wins, value, prior, fills = engine.selftest_rollout(boards, R, seed=seed, fills=True)
    hw, hv = host(boards, R, seed)
    assert np.array_equal(wins, hw), (N, R, np.flatnonzero(wins != hw)[:8])
    assert np.array_equal(bits(value), bits(hv)), (N, R)
    e = (boards == 0).sum(axis=1)
    want_prior = np.zeros((n, cells), np.float32)
    for i in range(n):
        if e[i]:
            want_prior[i, :e[i]] = np.float32(1.0) / np.float32(e[i])
    assert np.array_equal(bits(prior), bits(want_prior)), (N, R)
    assert fills.shape == (n, min(R, 64), cells)
    return fills


@pytest.mark.parametrize("N", SIZES)
def test_selftest_rollout_equals_the_host_definition(N):
    boards = boards_of(N)
    for R in (1, 16, 64, 65, 200):          # lanes idle, exactly one pass, a ragged second and fourth pass
        fills = check_against_host(boards, N, R)
        e = (boards == 0).sum(axis=1)
        for i in range(len(boards)):
            f = fills[i]
            assert set(np.unique(f)) <= {1, 2}, (N, R, i)
            fixed = boards[i] != 0
            assert (f[:, fixed] == boards[i][fixed]).all(), (N, R, i)
            # exactly (e + 1) >> 1 colour-1 cells are added in every returned fill
            assert ((f[:, ~fixed] == 1).sum(axis=1) == (e[i] + 1) >> 1).all(), (N, R, i)
        if R in (16, 65):                   # the fills themselves against the restatement of the definition's text
            for i in (0, len(boards) // 2):
                for r in (0, min(R, 64) - 1):
                    assert fills[i, r].tolist() == ref.fill(SEED, N, boards[i], r), (N, R, i, r)


@pytest.mark.parametrize("n", [1, 3, 257])
def test_selftest_rollout_row_counts(n):
    """One row, a part of a block (four rows to a block) and many blocks with a ragged last one."""
    for N in (5, 11, 13):
        pool = boards_of(N)
        boards = pool[np.arange(n) % len(pool)].copy()
        rng = np.random.RandomState(n + N)
        for i in range(len(pool), n):       # beyond the pool: fresh random positions, every row its own
            boards[i] = ref.random_position(rng, N, int(rng.randint(1, N * N + 1)))
        for R in (16, 65):
            check_against_host(boards, N, R, seed=n)


def test_full_boards_on_the_device():
    from azalea_amd import engine
    for N in SIZES:
        built = ref.full_boards(N)
        boards = np.stack([b for _, b, _ in built]).astype(np.int32)
        wins, value, _ = engine.selftest_rollout(boards, 65, seed=3)
        want = np.array([65 if w else 0 for _, _, w in built], np.int32)
        assert np.array_equal(wins, want), (N, [name for name, _, _ in built], wins)
        assert np.array_equal(value, np.where(want > 0, 1.0, -1.0).astype(np.float32))


# ---- whole searches ---------------------------------------------------------------------------------------------------
def make(evaluator, n, G, **kw):
    from azalea_amd import engine as eng
    cfg = dict(board_size=n, n_games=G, simulations=40, search_batch_size=8, exploration_coef=0.5,
               exploration_depth=0, noise_alpha=0.03, noise_scale=0.0, temperature=0.0, seed=12345)
    cfg.update(kw)
    return eng.Engine(evaluator=evaluator, **cfg)


def move_prefixes(n):
    """Four different move prefixes (tile + 1, colour 1 first) of 0, 3, n and n + 1 random stones -- both colours to
    move, so flipped rows included -- none of which ends the game."""
    rng = np.random.RandomState(n)
    while True:
        perm = rng.permutation(n * n)
        out = [(perm[:length] + 1).tolist() for length in (0, 3, n, n + 1)]
        board = [0] * (n * n)
        for i, c in enumerate(perm[:n + 1]):
            board[c] = 1 + (i & 1)
        turned = [3 - v if v else 0 for v in board]
        if not any(f(b, n) for f in (ref.one_connects, ref.two_connects) for b in (board, turned)):
            return out


@pytest.mark.parametrize("n", [5, 9, 13])
def test_search_with_the_rollout_evaluator_equals_the_host_phase_api(n):
    """Engine A searches with the kernel at its evaluation points; engine B is driven phase by phase with a host
    evaluator built on azx_rollout_value.  The trees must be the same bit for bit."""
    from azalea_amd import engine as eng
    G, R, seed = 4, 8, 77
    prefixes = move_prefixes(n)
    assert len(prefixes) == G and len({tuple(p) for p in prefixes}) == G and len({len(p) % 2 for p in prefixes}) == 2
    A = make(eng.EVAL_EXTERNAL, n, G)
    B = make(eng.EVAL_EXTERNAL, n, G)
    A.set_rollout_evaluator(R, seed)
    assert "eval=rollout(%d)" % R in A.kernel_info() and "eval=rollout" not in B.kernel_info()
    rows = []

    def host_eval(boards, lm, slot, k):
        rows.append(len(k))
        value = np.zeros(len(k), np.float32)
        prior = np.zeros((len(k), n * n), np.float32)
        for i in range(len(k)):
            _, value[i] = eng.rollout_value(seed, boards[i], R)
            prior[i, :k[i]] = np.float32(1.0) / np.float32(k[i])
        return value, prior[:, :int(k.max())]

    for E in (A, B):
        E.reset(moves=prefixes)
    for move in range(2):                   # the second search starts from a reused subtree
        A.search()
        B.search_external(host_eval)
        ra, rb = A.get_root(), B.get_root()
        for key in ra:
            assert np.array_equal(ra[key].view(np.uint32) if ra[key].dtype == np.float32 else ra[key],
                                  rb[key].view(np.uint32) if rb[key].dtype == np.float32 else rb[key]), (move, key)
        for g in range(G):
            da, db = A.tree_dump(g), B.tree_dump(g)
            assert da["num_nodes"] == db["num_nodes"] and da["root_id"] == db["root_id"]
            for key in ("parent", "first_child", "num_children"):
                assert np.array_equal(da[key], db[key]), (move, g, key)
            for key in ("num_visits", "total_value", "prior_prob"):
                assert np.array_equal(bits(da[key]), bits(db[key])), (move, g, key)
        st = A.rollout_stats()
        assert st["rows"] == sum(rows) and st["rollouts"] == R * sum(rows) and st["handovers"] == len(rows)
        assert 0 < st["rollouts_won"] < st["rollouts"]
        pick = np.argmax(ra["child_visits"], axis=1).astype(np.int32)
        A.advance(pick)
        B.advance(pick)
    A.close()
    B.close()


# ---- registration -----------------------------------------------------------------------------------------------------
def test_registration():
    import torch
    from azalea_amd import engine as eng
    n, G = 5, 4
    for evaluator in (eng.EVAL_RESNET, eng.EVAL_UNIFORM):
        E = make(evaluator, n, G, num_blocks=1, base_chans=32)
        with pytest.raises(eng.AzxError, match="AZX_EVAL_EXTERNAL"):
            E.set_rollout_evaluator(8, 1)
        E.close()
    E = make(eng.EVAL_EXTERNAL, n, G, flags=eng.FLAG_RANDOM_REFLECT)
    with pytest.raises(eng.AzxError, match="AZX_FLAG_RANDOM_REFLECT"):
        E.set_rollout_evaluator(8, 1)
    E.close()

    E = make(eng.EVAL_EXTERNAL, n, G)
    U = make(eng.EVAL_UNIFORM, n, G)
    with pytest.raises(ValueError):
        E.set_rollout_evaluator(4097, 1)
    with pytest.raises(eng.AzxError):       # no evaluator yet: a match refuses the engine, search wants the phases
        eng.Match(E, U)
    with pytest.raises(eng.AzxError, match="azx_search_begin"):
        E.search()
    E.set_rollout_evaluator(8, 1)
    E.search()
    assert E.rollout_stats()["rows"] > 0
    m = eng.Match(E, U)
    res = m.play(4)
    assert res["stats"]["games"] == 4 and res["stats"]["voided"] == 0
    E.set_rollout_evaluator(0)              # unregistered: search is AZX_ESTATE again, the made match refuses to play
    assert "eval=rollout" not in E.kernel_info()
    with pytest.raises(eng.AzxError, match="azx_search_begin"):
        E.search()
    with pytest.raises(eng.AzxError):
        m.play(4)
    m.close()
    with pytest.raises(eng.AzxError):
        eng.Match(E, U)
    # an external evaluator afterwards replaces it, and the other way round: the last call wins
    E.set_rollout_evaluator(8, 1)
    calls = []

    def zero(board, legal):
        calls.append(len(board))
        k = (legal != 0).sum(1, keepdim=True).clamp(min=1)
        return torch.zeros(len(board), device=board.device), (legal != 0).float() / k

    E.set_external_evaluator(zero)
    assert "eval=rollout" not in E.kernel_info()
    E.reset()
    before = E.rollout_stats()["rows"]
    E.search()
    assert calls and E.rollout_stats()["rows"] == before
    E.set_rollout_evaluator(16, 2)
    assert "eval=rollout(16)" in E.kernel_info() and E.rollout_stats()["rows"] == 0
    n_calls = len(calls)
    E.reset()
    E.search()
    assert len(calls) == n_calls and E.rollout_stats()["rows"] > 0
    m = eng.Match(E, U)
    m.close()
    E.close()
    U.close()


# ---- strength ---------------------------------------------------------------------------------------------------------
def test_a_rollout_agent_beats_a_search_that_only_sees_terminal_nodes():
    """7x7, 200 simulations a side, temperature 1 for the first 4 plies, no noise, 64 games with the colours shared
    evenly: RolloutNet(32)'s evaluator against AZX_EVAL_UNIFORM.  The bar is 44 wins = 32 + 3 * sqrt(64) / 2, three
    standard deviations above an even match; at least 32 of the games must be distinct move sequences."""
    from azalea_amd import engine as eng
    from azalea_amd.rollout import RolloutNet
    net = RolloutNet(32)
    kw = dict(simulations=200, search_batch_size=10, exploration_depth=4, temperature=1.0, noise_scale=0.0)
    A = make(eng.EVAL_EXTERNAL, 7, 64, seed=1 << 32, **kw)
    B = make(eng.EVAL_UNIFORM, 7, 64, seed=2 << 32, **kw)
    A.set_rollout_evaluator(net.rollouts, net.seed)
    m = eng.Match(A, B)
    res = m.play(64, moves=True)
    st = res["stats"]
    distinct = len({tuple(row[:length]) for row, length in zip(res["moves"].tolist(), res["length"].tolist())})
    print("rollout(32) vs uniform on 7x7 at 200 simulations: wins %s of %d, first player wins %d, %d distinct games, "
          "%.2f s" % (st["wins"], st["games"], st["first_player_wins"], distinct, st["seconds"]))
    assert st["games"] == 64 and st["voided"] == 0
    assert st["wins"][0] >= 44, st
    assert distinct >= 32, distinct
    m.close()
    A.close()
    B.close()


# ---- the evaluation surface ---------------------------------------------------------------------------------------------
def agents_5x5():
    import torch
    from azalea_amd.azalea_agent import AzaleaAgent
    from azalea_amd.game.hex import HexGame
    from azalea_amd.policy import Policy
    from azalea_amd.rollout import RolloutNet
    cfg = dict(board_size=5, simulations=30, search_batch_size=6, exploration_coef=0.5, exploration_depth=4,
               exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0)
    torch.manual_seed(1)
    a = Policy()
    a.initialize(dict(cfg, device="cpu", network="azalea_amd.rollout.RolloutNet", num_blocks=0, base_chans=0))
    a.net = RolloutNet(16, seed=5)
    b = Policy()
    b.initialize(dict(cfg, device="cuda:0", network="HexNetwork", num_blocks=1, base_chans=32))
    for p in (a, b):
        p.settings["move_sampling"] = True
    return [AzaleaAgent(lambda: HexGame(5), policy=p, device="cuda:0") for p in (a, b)]


def test_evaluate_throughput_takes_a_rolloutnet_agent_pooled_or_not():
    from azalea_amd import evaluation
    agents = agents_5x5()
    info, games = {}, {}
    pooled = evaluation.evaluate_throughput(agents, 4, pooled=True, seed=3, info=info, games=games)
    assert "eval=rollout(16)" in info[0] and "eval=rollout" not in info[1]
    assert sum(pooled[(0, 1)]) == 4
    games2 = {}
    plain = evaluation.evaluate_throughput(agents, 4, pooled=False, seed=3, games=games2)
    assert {p: list(v) for p, v in plain.items()} == {p: list(v) for p, v in pooled.items()}
    assert np.array_equal(games[(0, 1)]["moves"], games2[(0, 1)]["moves"])


def test_a_policy_with_a_rolloutnet_searches_on_the_device_and_plays_a_game():
    """Policy.choose_action runs eng.search() with the kernel registered (no host evaluator loop), and play_game
    works as for any custom net."""
    from azalea_amd.play_game import play_game
    agents = [agents_5x5()[0], agents_5x5()[0]]
    for i, a in enumerate(agents):
        a.seed(10 + i)
    result, frame, _ = play_game(agents, collect_data=True)
    assert result != 0 and len(frame) >= 9          # a 5x5 game cannot end before its ninth stone
    for a in agents:
        pol = a.policy
        assert pol._engine is not None and "eval=rollout(16)" in pol._engine.kernel_info()
        assert pol._engine.rollout_stats()["rows"] > 0


def test_players_take_a_rolloutnet_agent():
    """Player(external_batch=True) plays rollout self-play in one engine, and the two-agent device-match Player takes a
    rollout agent beside a HexNetwork one; both register the kernel, neither needs the net on a CUDA device."""
    from azalea_amd.parallel_player import Player
    roll, net = agents_5x5()
    player = Player(None, [roll], n_games=16, external_batch=True, gather=False)
    frame, metrics = player.read(100)
    assert len(frame) >= 100 and metrics["game_error"] == 0
    assert "eval=rollout(16)" in player._engine.kernel_info() and player._engine.rollout_stats()["rows"] > 0
    match = Player(None, [roll, net], n_games=16, device_match=True, gather=False)
    frame, metrics = match.read(100)
    assert len(frame) >= 100 and metrics["game_error"] == 0
    a, b, _ = match._match
    assert "eval=rollout(16)" in a.kernel_info() and "eval=rollout" not in b.kernel_info()
    assert a.rollout_stats()["rows"] > 0
