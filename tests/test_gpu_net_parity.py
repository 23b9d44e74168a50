"""GPU parity of the HIP resnet forward (MFMA tower + heads) against the reference's golden
outputs (<= 1e-4 on value and legal-move log-probabilities, network.py:134-152) and of the
resnet-driven search against the CPU oracle replaying the device's own evaluations."""
import os

import numpy as np
import pytest

from forward_accuracy_cases import expected_kernels

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    from azalea_amd import engine
    return engine


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.mark.parametrize("tag", ["5_1x8", "13_2x32", "11_6x64"])
def test_g3_forward_golden(eng, orc, tag):
    z = np.load(os.path.join(GOLDEN, "g3_forward_%s.npz" % tag))
    n, blocks, chans = [int(x) for x in z["cfg"]]
    state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
    E = eng.Engine(board_size=n, n_games=8, simulations=10, search_batch_size=10,
                   evaluator=eng.EVAL_RESNET, num_blocks=blocks, base_chans=chans)
    E.set_weights(state)
    value, logprob = E.forward(z["board"], z["legal_moves"])
    legal = z["legal_moves"] > 0
    assert np.abs(value - z["value"]).max() <= TOL
    assert np.abs(logprob - z["moves_logprob"])[legal].max() <= TOL
    if (~legal).any():
        assert np.abs(logprob - z["moves_logprob"])[~legal].max() <= 1e-3
    ov, olp = orc.Net(n, blocks, chans, state).forward(z["board"], z["legal_moves"])
    assert np.abs(value - ov).max() <= TOL and np.abs(logprob - olp)[legal].max() <= TOL
    E.close()


def test_shipped_checkpoint_weights_forward(eng):
    """The reference's trained 6x64 network (golden G8: tensors and outputs recorded through the
    reference's Policy.load) on the MFMA path: saturated values, peaked policies."""
    z = np.load(os.path.join(GOLDEN, "g8_checkpoint.npz"))
    n, blocks, chans = [int(x) for x in z["cfg"]]
    state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
    E = eng.Engine(board_size=n, n_games=8, simulations=10, search_batch_size=10,
                   evaluator=eng.EVAL_RESNET, num_blocks=blocks, base_chans=chans)
    E.set_weights(state)
    value, logprob = E.forward(z["board"], z["legal_moves"])
    legal = z["legal_moves"] > 0
    assert np.abs(value - z["value"]).max() <= TOL
    assert np.abs(logprob - z["moves_logprob"])[legal].max() <= TOL
    E.close()


def _random_positions(orc, n, count, rng):
    boards, moves = [], []
    while len(boards) < count:
        h = orc.Hex(n)
        for _ in range(int(rng.randint(0, n * n - 2))):
            lm = h.legal_moves()
            h2 = h.copy()
            h2.step(int(lm[rng.randint(len(lm))]))
            if h2.result:
                break
            h = h2
        b, lm = h.board, h.legal_moves()
        if h.color == 1:
            b, lm = orc.flip_board_moves(b, lm)
        boards.append(b)
        moves.append(lm)
    K = max(len(m) for m in moves)
    lm = np.zeros((count, K), np.int32)
    for i, m in enumerate(moves):
        lm[i, :len(m)] = m
    return np.array(boards, np.int32), lm


def test_forward_13x13_64ch_vs_oracle(eng, orc):
    """BASELINE config 5's board with the 64-channel MFMA tiling (6 M-tiles, one board/block)."""
    import torch
    from azalea_amd.network import HexNetwork
    torch.manual_seed(3)
    net = HexNetwork(board_size=13, num_blocks=3, base_chans=64).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.3, 1.7)
    state = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    rng = np.random.RandomState(4)
    boards, lm = _random_positions(orc, 13, 24, rng)
    E = eng.Engine(board_size=13, n_games=4, simulations=10, search_batch_size=10,
                   evaluator=eng.EVAL_RESNET, num_blocks=3, base_chans=64)
    E.set_weights(state)
    value, logprob = E.forward(boards, lm)
    ov, olp = orc.Net(13, 3, 64, state).forward(boards, lm)
    legal = lm > 0
    assert np.abs(value - ov).max() <= TOL and np.abs(logprob - olp)[legal].max() <= TOL
    with torch.no_grad():
        t = net(torch.tensor(boards), torch.tensor(lm))
    assert np.abs(value - t["value"].numpy()).max() <= TOL
    assert np.abs(logprob - t["moves_logprob"].numpy())[legal].max() <= TOL
    E.close()


@pytest.mark.parametrize("n,blocks,chans,count,use_oracle", [(13, 2, 128, 12, True), (11, 1, 128, 8, True),
                                                             (13, 19, 256, 6, False), (5, 0, 128, 4, True)])
def test_wide_tower_forward(eng, orc, n, blocks, chans, count, use_oracle):
    """Channel counts that are multiples of 128 (BASELINE configs[4]: 13x13, 19x256) run one MFMA
    launch per conv layer with activations in HBM (k_conv_wide_f16x3): <= 1e-4 against the torch
    module (and the C oracle where it is quick enough)."""
    import torch
    from azalea_amd.network import HexNetwork
    torch.manual_seed(n * 1000 + chans + blocks)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.3, 1.7)
    state = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    rng = np.random.RandomState(n + blocks)
    boards, lm = _random_positions(orc, n, count, rng)
    E = eng.Engine(board_size=n, n_games=4, simulations=10, search_batch_size=10,
                   evaluator=eng.EVAL_RESNET, num_blocks=blocks, base_chans=chans)
    assert expected_kernels(n, blocks, chans, os.environ) in E.kernel_info(), E.kernel_info()   # which tower this point hit
    E.set_weights(state)
    value, logprob = E.forward(boards, lm)
    legal = lm > 0
    with torch.no_grad():
        t = net(torch.tensor(boards), torch.tensor(lm))
    assert np.abs(value - t["value"].numpy()).max() <= TOL
    assert np.abs(logprob - t["moves_logprob"].numpy())[legal].max() <= TOL
    if use_oracle:
        ov, olp = orc.Net(n, blocks, chans, state).forward(boards, lm)
        assert np.abs(value - ov).max() <= TOL and np.abs(logprob - olp)[legal].max() <= TOL
    E.close()


@pytest.mark.parametrize("n,blocks,chans", [(n, 1 + n % 2, (16, 64, 128, 24, 32, 256, 48, 8, 96)[(n + k) % 9])
                                            for n in range(2, 14) for k in (0, 4)])
def test_forward_every_board_size(eng, orc, n, blocks, chans):
    """Every board size the engine accepts, with channel counts that land on each tower as azx_net_create dispatches
    them (forward_accuracy_cases.expected_kernels, asserted per point): 64 channels on the fused split-f16 tower up to
    11x11 and on the exact-fp32 MFMA tiling <64,6,1,2,2> on 12x12 / 13x13; 32 channels on the exact-fp32 MFMA tiling
    <32,6,2,2,1>; 128 / 256 on the wide per-layer split-f16 pair; 8 / 16 / 24 / 48 / 96 on the exact-fp32 VALU pair.
    Nine positions (an odd count), against the torch module.  (A sweep of all 200 combinations of 2..13 x {8 .. 256} x
    {1, 2} blocks ran clean; this is a diagonal of it.)"""
    test_wide_tower_forward(eng, orc, n, blocks, chans, 9, False)


@pytest.mark.parametrize("n,blocks,chans,count", [(13, 2, 256, 27), (11, 2, 128, 35)])
def test_wide_tower_batch_split_over_streams(eng, orc, n, blocks, chans, count):
    """A wide-tower batch of more than 16 boards is cut into parts that run their layer launches on separate
    streams (fork / join events, e_base > 0, an XCD-remapped grid per part).  A board count that is not a multiple
    of 8, against the torch module (<= 1e-4) and bit for bit against engines created with the batch on one
    stream and on three (AZX_WIDE_STREAMS is read once per engine, at azx_create)."""
    import torch
    from azalea_amd.network import HexNetwork
    torch.manual_seed(n * 77 + chans)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.3, 1.7)
    state = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    rng = np.random.RandomState(count)
    boards, lm = _random_positions(orc, n, count, rng)
    outs = {}
    for streams in ("2", "1", "3"):
        os.environ["AZX_WIDE_STREAMS"] = streams
        try:
            E = eng.Engine(board_size=n, n_games=4, simulations=10, search_batch_size=10,
                           evaluator=eng.EVAL_RESNET, num_blocks=blocks, base_chans=chans)
        finally:
            os.environ.pop("AZX_WIDE_STREAMS", None)
        assert "AZX_WIDE_STREAMS=%s" % streams in E.kernel_info()
        E.set_weights(state)
        outs[streams] = E.forward(boards, lm)
        E.close()
    value, logprob = outs["2"]
    legal = lm > 0
    with torch.no_grad():
        t = net(torch.tensor(boards), torch.tensor(lm))
    assert np.abs(value - t["value"].numpy()).max() <= TOL
    assert np.abs(logprob - t["moves_logprob"].numpy())[legal].max() <= TOL
    for streams in ("1", "3"):
        assert np.array_equal(outs[streams][0], value) and np.array_equal(outs[streams][1], logprob), streams


def test_resnet_search_replayed_by_oracle(eng, orc):
    """Search with the device network; feed the SAME (value, prior) stream to the CPU oracle:
    trees must be identical bit for bit (visit counts, values, priors, topology), and the
    stream itself must match the oracle's own fp32 forward within 1e-4."""
    z = np.load(os.path.join(GOLDEN, "g3_forward_11_6x64.npz"))
    state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
    _resnet_search_replay(eng, orc, 11, 6, 64, state, 6, 60, 80)


@pytest.mark.parametrize("n,blocks,chans", [(2, 1, 16), (3, 1, 64), (5, 1, 32), (7, 2, 128), (9, 1, 24), (12, 1, 256),
                                            (13, 1, 64), (13, 1, 128)])
def test_resnet_search_replay_on_other_shapes(eng, orc, n, blocks, chans):
    """The same replay on the smallest and largest boards and on every tower kind (fused split-f16, wide per-layer,
    exact fp32): flipped leaf boards in, priors written back by original cell, trees identical to the oracle's bit for
    bit when it consumes the device's evaluations."""
    import torch
    from azalea_amd.network import HexNetwork
    torch.manual_seed(n * 100 + chans)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.3, 1.7)
    state = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    _resnet_search_replay(eng, orc, n, blocks, chans, state, 5, 40, max(1, n * n - 2 * n), oracle_net=chans <= 64)


def _resnet_search_replay(eng, orc, n, blocks, chans, state, G, sims, max_prefix, oracle_net=True):
    rng = np.random.RandomState(11)
    prefixes = []
    for g in range(G):
        h, mv = orc.Hex(n), []
        for _ in range(int(rng.randint(0, max_prefix))):
            lm = h.legal_moves()
            m = int(lm[rng.randint(len(lm))])
            h2 = h.copy()
            h2.step(m)
            if h2.result:
                break
            h, mv = h2, mv + [m]
        prefixes.append(mv)
    E = eng.Engine(board_size=n, n_games=G, simulations=sims, search_batch_size=10,
                   exploration_coef=0.5, evaluator=eng.EVAL_RESNET, num_blocks=blocks, base_chans=chans,
                   flags=eng.FLAG_NO_COMPACT, nodes_per_game=1 << 16)
    E.set_weights(state)
    E.reset(moves=prefixes)
    onet = orc.Net(n, blocks, chans, state) if oracle_net else None
    games = []
    for g in range(G):
        h = orc.Hex(n)
        for m in prefixes[g]:
            h.step(m)
        games.append(h)
    trees = [orc.Tree(1 << 16) for _ in range(G)]
    for rnd in range(2):
        tape = E.search_recorded()
        move_ids = np.full(G, -1, np.int32)
        for g in range(G):
            rows = [t for t in tape if t[0] == g]
            off = np.zeros(len(rows) + 1, np.int64)
            off[1:] = np.cumsum([r[1] for r in rows])
            ev = orc.TapeEval([r[2] for r in rows], [r[1] for r in rows],
                              np.concatenate([r[3] for r in rows]), off)
            st = orc.search(trees[g], games[g], ev, sims, 10, 0.5)
            assert st.status == 0 and not ev.mismatch and ev.consumed == len(rows)
            d, o = E.tree_dump(g), trees[g].dump()
            assert d["num_nodes"] == o["num_nodes"] and d["root_id"] == o["root_id"]
            for name in ("parent", "first_child", "num_children"):
                assert np.array_equal(d[name], o[name]), (g, name)
            for name in ("num_visits", "total_value", "prior_prob"):
                assert np.array_equal(bits(d[name]), bits(o[name])), (g, name)
            # the device evaluations themselves vs the oracle network on the same positions
            if rnd == 0 and onet is not None:
                t2 = orc.Tree(1 << 16)
                st2 = orc.search(t2, games[g], onet, sims, 10, 0.5)
                nv_dev = trees[g].root_stats()[0]
                # not bit-exact (1e-4 logits can flip a near-tie) but the root priors must agree
                assert np.abs(trees[g].root_stats()[2] - t2.root_stats()[2]).max() <= TOL
                assert abs(nv_dev.sum() - t2.root_stats()[0].sum()) == 0
            nv = trees[g].root_stats()[0]
            mid = int(np.argmax(nv))
            move_ids[g] = mid
            lm = games[g].legal_moves()
            trees[g].move(mid)
            games[g].step(int(lm[mid]))
        E.advance(move_ids)
        if any(h.result for h in games):        # (tiny boards: a game ended with this move; one round is the test)
            break
    E.close()


def test_resnet_play_mode_runs(eng):
    """Throughput path with the device network: azx_search (no phases) + device move draw."""
    import torch
    from azalea_amd.network import HexNetwork
    torch.manual_seed(0)
    net = HexNetwork(board_size=7, num_blocks=2, base_chans=64).eval()
    state = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    E = eng.Engine(board_size=7, n_games=16, simulations=20, search_batch_size=10,
                   exploration_depth=4, evaluator=eng.EVAL_RESNET, num_blocks=2, base_chans=64)
    E.set_weights(state)
    rows, st = E.play(64)
    assert len(rows["board"]) >= 64 and st["games"] >= 1 and st["evals"] > 0
    assert np.isfinite(rows["moves_prob"]).all()
    E.close()


def test_forward_config5_shape_13x13_256ch_vs_oracle(eng, orc):
    """BASELINE config 5's network shape (13x13, 256 channels; 2 of its 19 blocks to keep the CPU
    oracle quick): the forward must hold the same 1e-4 bound on the wide-channel path."""
    import torch
    from azalea_amd.network import HexNetwork
    torch.manual_seed(5)
    net = HexNetwork(board_size=13, num_blocks=2, base_chans=256).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    state = {k: v.detach().numpy() for k, v in net.state_dict().items()}
    rng = np.random.RandomState(6)
    boards, lm = _random_positions(orc, 13, 6, rng)
    E = eng.Engine(board_size=13, n_games=2, simulations=10, search_batch_size=10,
                   evaluator=eng.EVAL_RESNET, num_blocks=2, base_chans=256)
    E.set_weights(state)
    value, logprob = E.forward(boards, lm)
    ov, olp = orc.Net(13, 2, 256, state).forward(boards, lm)
    legal = lm > 0
    assert np.abs(value - ov).max() <= TOL and np.abs(logprob - olp)[legal].max() <= TOL
    E.close()


def test_full_size_leaf_batch_sampled_against_the_oracle(eng, orc):
    """BASELINE configs[2] at full size: one leaf batch of the 4096-game pool (~40 k positions, the tower's real grid of
    ~20 k blocks, the heads' ~2.5 k tiles) evaluated by the device network inside a search; 160 of its rows -- the first
    and last rows of the batch and a seeded sample in between -- against the CPU oracle's fp32 forward of the same
    boards: value and every legal move's prior within 1e-4.  (The small forward tests never launch more than 5 k
    positions.)"""
    z = np.load(os.path.join(GOLDEN, "g3_forward_11_6x64.npz"))
    state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
    G = 4096
    E = eng.Engine(board_size=11, n_games=G, simulations=400, search_batch_size=10, evaluator=eng.EVAL_RESNET,
                   num_blocks=6, base_chans=64, noise_scale=0.25)
    E.set_weights(state)
    E.reset(moves=eng.random_prefixes(11, np.arange(G), 60, 1234))      # de-synchronised mid-game positions
    n = E.search_begin()
    assert n == G                                                       # the roots
    n, done = E.search_step()                                           # first select batch
    assert not done and 0.8 * G * 10 <= n <= G * 10
    boards, lm, slot, k = E.get_leaves()
    value, prior = E.get_evals()
    assert len(boards) == len(value) == n
    rng = np.random.RandomState(5)
    rows = np.unique(np.r_[np.arange(16), np.arange(n - 16, n), rng.randint(0, n, 128)])
    ov, olp = orc.Net(11, 6, 64, state).forward(boards[rows], lm[rows])
    assert np.abs(value[rows] - ov).max() <= TOL
    for i, r in enumerate(rows):
        kk = int(k[r])
        assert kk == int((lm[r] > 0).sum()) and kk > 0
        assert np.abs(prior[r, :kk] - np.exp(olp[i, :kk])).max() <= TOL
        assert abs(float(prior[r, :kk].sum()) - 1.0) <= 1e-4
    while not done:
        n, done = E.search_step()
    E.close()


def test_tower_variants_selected_by_environment():
    """The alternative tower kernel (exact-fp32 MFMA) and the scalar-FMA heads kernel are chosen by environment
    variables read once per engine: run the golden forward tests under each."""
    import subprocess
    import sys
    here = os.path.abspath(__file__)
    for env in ({"AZX_TOWER": "fp32"}, {"AZX_HEADS": "valu"}):
        r = subprocess.run([sys.executable, "-m", "pytest", here, "-q", "-x", "-k", "g3_forward or shipped_checkpoint"],
                           env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (env, r.stdout[-2000:], r.stderr[-2000:])


def test_second_network_with_a_larger_lds_image_in_one_process(eng, orc):
    """The tower kernels take their LDS image as dynamic shared memory above the 64 KB default, and the opt-in limit
    (hipFuncAttributeMaxDynamicSharedMemorySize) is raised for all of them at every network creation.  A later
    network with a larger image than the first (here the exact-fp32 tower: 29 KB on 5x5, 133 KB on 11x11) must run
    and match the oracle.  (ROCm 7.2 launches the second one even with the limit left at the first size; the test
    pins the behaviour rather than that leniency.)"""
    os.environ["AZX_TOWER"] = "fp32"
    try:
        for n in (5, 11):
            rng = np.random.RandomState(n)
            from azalea_amd.network import HexNetwork
            import torch
            torch.manual_seed(n)
            m = HexNetwork(board_size=n, num_blocks=1, base_chans=64).eval()
            state = {k: v.detach().numpy() for k, v in m.state_dict().items() if v.dtype == torch.float32}
            boards, lm = _random_positions(orc, n, 6, rng)
            E = eng.Engine(board_size=n, n_games=2, simulations=10, search_batch_size=10,
                           evaluator=eng.EVAL_RESNET, num_blocks=1, base_chans=64)
            assert "fp32 MFMA" in E.kernel_info()
            E.set_weights(state)
            value, logprob = E.forward(boards, lm)
            E.close()
            ov, olp = orc.Net(n, 1, 64, state).forward(boards, lm)
            legal = lm > 0
            assert np.abs(value - ov).max() <= TOL and np.abs(logprob - olp)[legal].max() <= TOL
    finally:
        os.environ.pop("AZX_TOWER", None)


def test_heads_mfma_matches_the_scalar_heads_and_does_not_depend_on_the_batch(eng, orc):
    """k_heads_mfma (FC layers as fp32 MFMA GEMMs over tiles of 32 boards) against the scalar-FMA k_heads on the
    same tower output: value and legal log-probabilities within 2e-6; a board's outputs are bit-identical
    whatever else is in its tile (alone, first, last, in a ragged tail tile), which the global-game-index and
    tournament tests rely on."""
    z = np.load(os.path.join(GOLDEN, "g3_forward_11_6x64.npz"))
    state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
    rng = np.random.RandomState(3)
    boards, lm = _random_positions(orc, 11, 70, rng)
    outs = {}
    for heads in ("mfma", "valu"):
        os.environ["AZX_HEADS"] = heads
        try:
            E = eng.Engine(board_size=11, n_games=8, simulations=10, search_batch_size=10,
                           evaluator=eng.EVAL_RESNET, num_blocks=6, base_chans=64)
        finally:
            os.environ.pop("AZX_HEADS", None)
        assert ("k_heads_mfma" in E.kernel_info()) == (heads == "mfma")
        E.set_weights(state)
        outs[heads] = E.forward(boards, lm)
        if heads == "mfma":
            solo = [E.forward(boards[i:i + 1], lm[i:i + 1]) for i in (0, 31, 32, 69)]
            rev = E.forward(boards[::-1].copy(), lm[::-1].copy())
        E.close()
    legal = lm > 0
    v, lp = outs["mfma"]
    assert np.abs(v - outs["valu"][0]).max() <= 2e-6 and np.abs(lp - outs["valu"][1])[legal].max() <= 2e-6
    for (sv, slp), i in zip(solo, (0, 31, 32, 69)):
        assert np.array_equal(sv[0], v[i]) and np.array_equal(slp[0][legal[i]], lp[i][legal[i]]), i
    assert np.array_equal(rev[0][::-1], v) and np.array_equal(rev[1][::-1][legal], lp[legal])
