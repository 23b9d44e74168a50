"""The fused split-f16 tower's single k-loop (one instance for both kinds of layer, the epilogue chosen by the layer's
parity), its branches over the light tile's padding taps and the 8-row offset of board 1 in the LDS image,
on the smallest shapes at which they can go wrong: with one residual block one layer of each kind runs through the loop,
with two the cross-layer weight prefetch passes a residual -> plain boundary; N = 11 and 10 have full edge classes and
dead rows topping a tile up, N = 3 and 2 tiles of mostly (or only) dead rows.  `edge` must equal `rows` bit for bit, and
both must be within 1e-4 of the CPU oracle's fp32 forward on the legal moves (as tests/test_gpu_net_parity.py compares).
Positions and BatchNorm statistics are seeded as in tests/test_gpu_tower_edge_tiles.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4
COUNTS = (1, 2, 3, 5)          # a dead partner, a full block, odd tails


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


@pytest.mark.parametrize("blocks", (1, 2))
@pytest.mark.parametrize("n", (11, 10, 3, 2))
def test_edge_equals_rows_and_both_match_the_oracle(eng, n, blocks):
    from oracle import oracle as orc
    state = random_net(n, blocks, seed=100 * n + blocks)
    boards, lm = positions(n, max(COUNTS), seed=7 * n + blocks)
    want_v, want_lp = orc.Net(n, blocks, 64, state).forward(boards, lm)
    legal = lm > 0
    kw = dict(board_size=n, n_games=8, simulations=10, search_batch_size=10, num_blocks=blocks)
    A, B = make_engine(eng, None, **kw), make_engine(eng, "rows", **kw)
    try:
        assert "k_tower_f16x3_s16" in A.kernel_info() and "AZX_TOWER_TILES=edge" in A.kernel_info(), A.kernel_info()
        assert "k_tower_f16x3_s16" in B.kernel_info() and "AZX_TOWER_TILES=rows" in B.kernel_info(), B.kernel_info()
        A.set_weights(state)
        B.set_weights(state)
        for count in COUNTS:
            va, la = A.forward(boards[:count], lm[:count])
            vb, lb = B.forward(boards[:count], lm[:count])
            assert np.array_equal(bits(va), bits(vb)), (count, np.abs(va - vb).max())
            assert np.array_equal(bits(la), bits(lb)), (count, np.abs(la - lb).max())
            for name, v, lp in (("edge", va, la), ("rows", vb, lb)):
                ev = np.abs(v - want_v[:count]).max()
                el = np.abs(lp - want_lp[:count])[legal[:count]].max()
                print("N = %d, %d block(s), %d board(s), %s: value %.3g, log-prob %.3g off the oracle" % (n, blocks, count, name, ev, el))
                assert ev <= TOL and el <= TOL, (count, name, ev, el)
    finally:
        A.close()
        B.close()
