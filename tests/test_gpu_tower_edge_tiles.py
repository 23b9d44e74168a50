"""The fused split-f16 tower under its two position-tile maps: `edge`, the default, gives every wave one
tile of pure edge cells and skips that tile's MFMAs on the three taps that read only padding; AZX_TOWER_TILES=rows is the
row-major map with nothing skipped.  A skipped product would have added +-0 to an accumulator that started as +0 and the
order of the others is the same, so the two must agree bit for bit: in Engine.forward and in a search that plays moves.
The map itself is tests/test_tower_tile_map.py's (no GPU)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    from azalea_amd import engine
    return engine


def make_engine(eng, tiles, **kw):
    """An engine whose network is created under AZX_TOWER_TILES=`tiles` (None: unset, the default map)."""
    old = os.environ.pop("AZX_TOWER_TILES", None)
    if tiles is not None:
        os.environ["AZX_TOWER_TILES"] = tiles
    try:
        return eng.Engine(evaluator=eng.EVAL_RESNET, base_chans=64, **kw)
    finally:
        os.environ.pop("AZX_TOWER_TILES", None)
        if old is not None:
            os.environ["AZX_TOWER_TILES"] = old


def random_net(n, blocks, seed):
    import torch
    from azalea_amd.network import HexNetwork
    torch.manual_seed(seed)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=64).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.3, 1.7)
    return {k: v.detach().numpy() for k, v in net.state_dict().items()}


def positions(n, count, seed):
    """An empty board, a nearly full one, then seeded random stones; legal moves = the empty cells, tile + 1, padded."""
    rng = np.random.RandomState(seed)
    boards = np.zeros((count, n, n), np.int32)
    for i in range(count):
        if i == 0:
            continue
        flat = boards[i].reshape(-1)
        if i == 1:
            flat[:] = 1 + (np.arange(n * n) + np.arange(n * n) // n) % 2
            flat[rng.choice(n * n, 2, replace=False)] = 0
        else:
            stones = rng.randint(1, n * n - 1)
            cells = rng.choice(n * n, stones, replace=False)
            flat[cells] = 1 + rng.randint(0, 2, stones)
    lm = np.zeros((count, n * n), np.int32)
    for i in range(count):
        free = np.flatnonzero(boards[i].reshape(-1) == 0) + 1
        lm[i, :len(free)] = free
    return boards, lm


CASES = [("g3", 11, 6)] + [("random", n, blocks) for n in (11, 10, 8, 3) for blocks in (1, 6)]


@pytest.mark.parametrize("net,n,blocks", CASES)
def test_forward_is_bit_exact_between_the_two_maps(eng, net, n, blocks):
    if net == "g3":
        z = np.load(os.path.join(GOLDEN, "g3_forward_11_6x64.npz"))
        assert [int(x) for x in z["cfg"]] == [11, 6, 64]
        state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
    else:
        state = random_net(n, blocks, seed=100 * n + blocks)
    kw = dict(board_size=n, n_games=8, simulations=10, search_batch_size=10, num_blocks=blocks)
    A, B = make_engine(eng, None, **kw), make_engine(eng, "rows", **kw)
    try:
        assert "AZX_TOWER_TILES=edge" in A.kernel_info() and "AZX_TOWER_TILES=rows" in B.kernel_info()
        assert "k_tower_f16x3_s16" in A.kernel_info() and "k_tower_f16x3_s16" in B.kernel_info()
        A.set_weights(state)
        B.set_weights(state)
        boards, lm = positions(n, 37, seed=7 * n + blocks)
        for count in (1, 2, 3, 37):          # a lone board with a dead partner, a full block, odd tails
            va, la = A.forward(boards[:count], lm[:count])
            vb, lb = B.forward(boards[:count], lm[:count])
            assert np.isfinite(va).all() and np.isfinite(la[lm[:count] > 0]).all()
            assert np.array_equal(bits(va), bits(vb)), (count, np.abs(va - vb).max())
            assert np.array_equal(bits(la), bits(lb)), (count, np.abs(la - lb).max())
        # the other boards of a batch do not matter either: the last board alone
        v1, l1 = A.forward(boards[36:37], lm[36:37])
        assert np.array_equal(bits(v1), bits(va[36:37])) and np.array_equal(bits(l1), bits(la[36:37]))
    finally:
        A.close()
        B.close()


def test_shipped_checkpoint_forward_under_the_default_map(eng):
    """Golden G8 (the reference's trained 6x64 network) as test_gpu_net_parity.py asserts it, on an engine that is
    shown to run the edge map."""
    z = np.load(os.path.join(GOLDEN, "g8_checkpoint.npz"))
    n, blocks, chans = [int(x) for x in z["cfg"]]
    assert chans == 64
    state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
    E = make_engine(eng, None, board_size=n, n_games=8, simulations=10, search_batch_size=10, num_blocks=blocks)
    try:
        assert "AZX_TOWER_TILES=edge" in E.kernel_info()
        E.set_weights(state)
        value, logprob = E.forward(z["board"], z["legal_moves"])
        legal = z["legal_moves"] > 0
        assert np.abs(value - z["value"]).max() <= TOL
        assert np.abs(logprob - z["moves_logprob"])[legal].max() <= TOL
    finally:
        E.close()


def test_play_is_bit_exact_between_the_two_maps(eng):
    """64 games on 11x11 with 6x64, 30 simulations in batches of 10, three moves from seeded random prefixes."""
    n, G = 11, 64
    state = random_net(n, 6, seed=5)
    rng = np.random.RandomState(11)
    prefixes = [[int(c) + 1 for c in rng.choice(n * n, rng.randint(0, 20), replace=False)] for _ in range(G)]
    seen = {}
    for tiles in (None, "rows"):
        E = make_engine(eng, tiles, board_size=n, n_games=G, simulations=30, search_batch_size=10, num_blocks=6,
                        exploration_coef=0.5)
        try:
            assert ("AZX_TOWER_TILES=%s" % (tiles or "edge")) in E.kernel_info()
            E.set_weights(state)
            E.reset(moves=prefixes)
            trace = []
            for _ in range(3):
                E.search()
                root = E.get_root()
                trace.append(root)
                assert (root["k"] > 0).all() and (root["root_visits"] > 0).all()
                E.advance(np.argmax(root["child_visits"], axis=1).astype(np.int32))
                trace.append(E.get_games())
            seen[tiles] = trace
        finally:
            E.close()
    for a, b in zip(seen[None], seen["rows"]):
        assert a.keys() == b.keys()
        for key in a:
            if a[key].dtype == np.float32:
                assert np.array_equal(bits(a[key]), bits(b[key])), key
            else:
                assert np.array_equal(a[key], b[key]), key


def test_kernel_info_names_the_map(eng):
    kw = dict(board_size=5, n_games=2, simulations=10, search_batch_size=10)
    for tiles, said in ((None, "edge"), ("edge", "edge"), ("rows", "rows")):
        E = make_engine(eng, tiles, num_blocks=1, **kw)
        assert "AZX_TOWER_TILES=%s" % said in E.kernel_info(), E.kernel_info()
        E.close()
    # the other towers have no tile map; like every switch the setting is reported all the same, so that two engines'
    # descriptions differ only in what differs between them
    E = eng.Engine(evaluator=eng.EVAL_RESNET, base_chans=64, num_blocks=1, flags=eng.FLAG_TOWER_F16, **kw)
    assert "k_tower_f16_s16" in E.kernel_info() and "AZX_TOWER_TILES=edge" in E.kernel_info(), E.kernel_info()
    E.close()
