"""Throughput self-play and whole searches with a caller-supplied evaluator on the device
(azx_set_external_evaluator, Engine.set_external_evaluator, Player(external_batch=True))."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
P4 = pow(0x01000193, 4, 1 << 32)
STAT_KEYS = ("positions", "games", "game_errors", "plies", "selects", "evals", "sum_depth", "sum_k_interior",
             "sum_k_leaf", "sum_search_value", "sum_root_width", "sum_action_logprob", "sum_reward_last",
             "sum_game_length")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def torch_fnv(board):
    """fnv1a over the int32 board as the uniform-hash stub takes it (each cell: its low byte, then three zero
    bytes), int64 arithmetic reduced mod 2^32."""
    b = board.reshape(len(board), -1).to(torch.int64)
    h = torch.full((len(b),), 0x811C9DC5, dtype=torch.int64, device=board.device)
    for c in range(b.shape[1]):
        h = ((h ^ b[:, c]) * P4) & 0xFFFFFFFF
    return h


def uniform_hash_evaluator(cells, seen=None):
    """The AZX_EVAL_UNIFORM_HASH stub on the device: value (h & 0xffff) / 32768 - 1, priors 1/k (the float32 table
    the engine's default prior table holds)."""
    inv = torch.tensor((np.float32(1.0) / np.arange(0, cells + 1).clip(1).astype(np.float32)).astype(np.float32),
                       device=DEV)

    def evaluate(board, legal):
        if seen is not None:
            seen.append(len(board))
        h = torch_fnv(board)
        value = ((h & 0xFFFF).to(torch.float64) / 32768.0 - 1.0).to(torch.float32)
        k = (legal != 0).sum(1)
        prior = torch.where(legal != 0, inv[k][:, None], torch.zeros((), device=DEV))
        return value, prior
    return evaluate


def make(evaluator, n, G, **kw):
    from azalea_amd import engine as eng
    cfg = dict(board_size=n, n_games=G, simulations=20, search_batch_size=5, exploration_coef=0.5,
               exploration_depth=6, noise_alpha=0.03, noise_scale=0.25, temperature=1.0, seed=12345)
    cfg.update(kw)
    return eng.Engine(evaluator=evaluator, **cfg)


@pytest.mark.parametrize("n", [7, 13])
def test_play_with_device_hash_evaluator_equals_uniform_hash_engine(n):
    """Same games, bit for bit: both paths run the generic search kernel and draw their noise from the same
    per-(move, select) streams; only where the evaluations come from differs."""
    from azalea_amd import engine as eng
    G = 256
    A = make(eng.EVAL_UNIFORM_HASH, n, G)
    B = make(eng.EVAL_EXTERNAL, n, G)
    seen = []
    B.set_external_evaluator(uniform_hash_evaluator(n * n, seen))
    plies = 0
    for _ in range(5):
        ra, sa = A.play(50000, max_plies=60)
        rb, sb = B.play(50000, max_plies=60)
        plies += sb["plies"] // G
        assert sa["plies"] == sb["plies"] == 60 * G
        # finished games enter the harvest queue in the order the GPU finished them: compare game by game
        ia = np.argsort(ra["game_uid"], kind="stable")
        ib = np.argsort(rb["game_uid"], kind="stable")
        for key in ("board", "color", "nlegal", "reward", "game_uid"):
            assert np.array_equal(ra[key][ia], rb[key][ib]), key
        assert np.array_equal(bits(ra["moves_prob"][ia]), bits(rb["moves_prob"][ib]))
        assert np.array_equal(bits(A.play_row_metrics()[ia]), bits(B.play_row_metrics()[ib]))
        for key in STAT_KEYS:
            assert sa[key] == sb[key], key
        assert sb["net_launches"] > 0 and sb["net_seconds"] > 0.0
    assert plies == 300
    assert np.array_equal(A.debug_counters()[:10], B.debug_counters()[:10])
    assert max(seen) > 5                 # whole-pool batches, not one game's leaf batch
    A.close()
    B.close()


def hashprior(boards, lm):
    """tests/test_gpu_policy_parity.py's StubNet "hashprior" in numpy: (value[n], prior[n, K])."""
    from oracle import oracle as orc
    boards = np.asarray(boards, np.int32)
    lm = np.asarray(lm)
    B, K = lm.shape
    value = np.zeros(B, np.float32)
    logit = np.zeros((B, K), np.float32)
    for i in range(B):
        h = orc.fnv1a(boards[i].ravel())
        value[i] = np.float32((h & 0xFFFF) / 32768.0 - 1.0)
        for j in range(K):
            t = int(lm[i, j])
            if t:
                x = (h ^ (t * 2654435761)) & 0xFFFFFFFF
                x = (x * 2246822519) & 0xFFFFFFFF
                logit[i, j] = np.float32(((x >> 13) & 0xFF) / 64.0)
    lt = torch.tensor(logit)
    lt.masked_fill_(torch.tensor(lm == 0), -99)
    return value, torch.exp(torch.log_softmax(lt, dim=1)).numpy()


def test_search_device_handover_equals_host_handover():
    """azx_search with the registered evaluator builds the same trees as the host phase API (azx_get_leaves /
    azx_put_evals) with the same non-uniform priors, and hands the evaluator the same rows in the same order."""
    from azalea_amd import engine as eng
    n, G = 9, 48
    prefixes = eng.random_prefixes(n, range(G), 24, seed=7)
    assert len({len(p) % 2 for p in prefixes}) == 2          # both colours to move: flipped rows included
    kw = dict(simulations=30, search_batch_size=6, exploration_depth=0)
    A = make(eng.EVAL_EXTERNAL, n, G, **kw)
    B = make(eng.EVAL_EXTERNAL, n, G, **kw)
    sel = A.selects_per_search
    noise = np.random.RandomState(5).dirichlet([0.03] * (n * n), size=(G, sel)).astype(np.float64)
    got_a, got_b = [], []

    def host_eval(boards, lm, slot, k):
        kmax = int(k.max())
        got_a.append((boards.copy(), lm.copy(), kmax))
        return hashprior(boards, lm[:, :kmax])

    def dev_eval(board, legal):
        b, l = board.cpu().numpy(), legal.cpu().numpy()
        got_b.append((b.copy(), l.copy()))
        v, p = hashprior(b, l)
        return torch.from_numpy(v).to(DEV), torch.from_numpy(p).to(DEV)

    for E in (A, B):
        E.reset(moves=prefixes)
    B.set_external_evaluator(dev_eval)
    for _ in range(2):                      # two moves: the second search starts from a reused subtree
        A.search_external(host_eval, noise=noise, noise_scale=0.25)
        B.search(noise=noise, noise_scale=0.25)
        ra, rb = A.get_root(), B.get_root()
        for key in ra:
            assert np.array_equal(np.asarray(ra[key]).view(np.uint32), np.asarray(rb[key]).view(np.uint32)), key
        for g in range(G):
            ta, tb = A.tree_dump(g), B.tree_dump(g)
            for key in ta:
                assert np.array_equal(np.asarray(ta[key]).view(np.uint32) if isinstance(ta[key], np.ndarray)
                                      else ta[key], np.asarray(tb[key]).view(np.uint32)
                                      if isinstance(tb[key], np.ndarray) else tb[key]), (g, key)
        move = np.where(ra["k"] > 0, np.argmax(ra["child_visits"], axis=1), -1).astype(np.int32)
        A.advance(move)
        B.advance(move)
    assert len(got_a) == len(got_b) > 2
    for (ba, la, kmax), (bb, lb) in zip(got_a, got_b):
        assert np.array_equal(ba, bb)
        assert lb.shape[1] == kmax
        assert np.array_equal(la[:, :kmax], lb) and not la[:, kmax:].any()
    A.close()
    B.close()


class Wrapped(torch.nn.Module):
    """A custom network for the engine: a HexNetwork behind the reference's duck-typed contract, not one itself."""

    def __init__(self, inner, fail=None):
        super().__init__()
        self.inner = inner
        self.fail = fail
        self.batches = []

    def run(self, batch):
        self.batches.append(int(batch["board"].shape[0]))
        if self.fail is not None:
            raise self.fail
        return self.inner.run(batch)


class Boom(RuntimeError):
    pass


def player_for(net_fail=None, n=7, games=64):
    from azalea_amd import AzaleaAgent, HexGame, Player, Policy
    cfg = dict(device="cuda", network="HexNetwork", board_size=n, num_blocks=1, base_chans=16, simulations=16,
               search_batch_size=4, exploration_coef=0.5, exploration_depth=4, exploration_noise_alpha=0.03,
               exploration_noise_scale=0.25, exploration_temperature=1.0, seed=3)
    torch.manual_seed(0)
    pol = Policy()
    pol.initialize(cfg)
    pol.net = Wrapped(pol.net, net_fail)
    pol.settings.update(move_sampling=True, move_exploration=True)
    agent = AzaleaAgent(lambda: HexGame(n), policy=pol, device="cuda")
    return Player(None, [agent], n_games=games, external_batch=True), pol.net


def test_player_external_batch_reads_whole_games():
    player, net = player_for()
    frame, metrics = player.read(200)                 # rows_to_frame checks every row's legal moves
    assert len(frame) >= 200
    assert set(metrics) == {"games", "reward", "moves_per_game", "seconds_per_game", "game_error", "search_value",
                            "search_root_width", "action_logprob", "search_root_visits", "search_tree_nodes",
                            "search_root_children"}
    assert metrics["games"] >= 1 and metrics["moves_per_game"] >= len(frame) - 1e-9
    assert max(net.batches) > 4                       # one call evaluates many games' leaves
    assert not net.training                           # net.eval() before the production
    player.stop()


def test_player_surfaces_the_evaluator_exception():
    player, _ = player_for(net_fail=Boom("custom net failed"))
    with pytest.raises(Boom):
        player.read(50)
    player.stop()


def test_engine_errors_and_recovery():
    from azalea_amd import engine as eng
    from azalea_amd._lib import AzxError
    n, G = 7, 32
    E = make(eng.EVAL_EXTERNAL, n, G)
    with pytest.raises(AzxError, match="azx error -4"):
        E.play(100, max_plies=4)                      # no evaluator registered: still AZX_ESTATE
    with pytest.raises(AzxError, match="azx error -1"):
        make(eng.EVAL_UNIFORM, n, 4).set_external_evaluator(uniform_hash_evaluator(n * n))
    good = uniform_hash_evaluator(n * n)

    def raising(board, legal):
        raise Boom("evaluator failed")
    E.set_external_evaluator(raising)
    with pytest.raises(Boom) as info:
        E.play(100, max_plies=4)
    assert isinstance(info.value.__cause__, AzxError) and "azx error -7" in str(info.value.__cause__)
    E.set_external_evaluator(good)
    with pytest.raises(AzxError, match="azx error -4"):
        E.play(100, max_plies=4)                      # half-done searches: refused until reset
    E.reset()
    E.play(100, max_plies=4)

    def bad_row(kind, row=3):
        def evaluate(board, legal):
            v, p = good(board, legal)
            if len(board) > row:
                if kind == "negative":
                    p[row, 0] = -0.25
                    p[row, 1] += 0.25
                elif kind == "sum":
                    p[row] *= 1.01
                else:
                    v[row] = float("nan")
            return v, p
        return evaluate
    for kind, what in (("negative", "negative"), ("sum", "sum"), ("nan", "not finite")):
        E.set_external_evaluator(bad_row(kind))
        with pytest.raises(AzxError, match="azx error -7.*row 3 .*%s" % what):
            E.play(100, max_plies=4)
        E.set_external_evaluator(good)
        with pytest.raises(AzxError, match="azx error -4"):
            E.search()
        E.reset(slots=np.arange(G // 2))
        with pytest.raises(AzxError, match="azx error -4"):
            E.play(100, max_plies=4)                  # half the slots still hold half-done searches
        E.reset(slots=np.arange(G // 2, G))
        rows, st = E.play(100, max_plies=4)
        assert st["plies"] == 4 * G
    E.set_external_evaluator(None)
    with pytest.raises(AzxError, match="azx error -4"):
        E.play(100, max_plies=4)
    E.close()
