"""Float64 torch emulation of the plain-f16 WIDE tower (AZX_FLAG_TOWER_F16 on 128 / 256 channels: k_stem_wide_f16 +
k_conv_wide_f16_s16 per layer): the yardstick of tests/test_gpu_wide_f16.py, pinned by tests/test_wide_f16_emulation.py.
A plain module, no test in it.

The definition (include/azx.h) is tests/f16_emulation.py's with one difference: the wide path computes the heads in
fp32 from the unrounded activations of the last layer (k_heads), so the six 1x1 head filters and their input are NOT
rounded.  BatchNorm is folded as the weight packer does it (f16_emulation._fold); the folded stem and conv weights
enter as f16(w); the activation written back after each ReLU enters the next conv as f16(a); sums, bias and the
residual (the unrounded block input) are not rounded -- float64 here, fp32 in the kernel; the one-hot stem input is
exact.  rounded=False leaves every f16 rounding out: the network itself.

Also here, shared by the CPU and the GPU test: the seeded fixtures (weights with randomised BatchNorm statistics,
positions) and the exact float64 module's outputs on them, computed once per process."""
import functools

import numpy as np
import torch
from torch.nn import functional as F

from f16_emulation import _fold


def forward(state, blocks, board, legal_moves, rounded=True):
    """(value [B], moves_logprob [B, K]) as float64 numpy arrays; `state`: the HexNetwork state dict (numpy or torch)."""
    r16 = (lambda t: t.float().half().double()) if rounded else (lambda t: t)
    g = lambda name: torch.as_tensor(state[name]).double()   # noqa: E731
    board, legal_moves = torch.as_tensor(board).long(), torch.as_tensor(legal_moves).long()

    def folded(conv, bn, rnd):
        scale, shift = _fold(state, bn)
        return rnd((g(conv) * scale[:, None, None, None]).float().double()), shift[None, :, None, None]

    # stem: T[co][v] per tap = scale[co] * sum_i emb[v][i] * w[co][i][tap]; zero padding = no contribution off the board
    scale, shift = _fold(state, "bn1")
    table = torch.einsum("vi,oiyx->ovyx", g("encoder.weight"), g("conv1.weight")) * scale[:, None, None, None]
    onehot = F.one_hot(board, 3).permute(0, 3, 1, 2).double()
    x = F.relu(F.conv2d(onehot, r16(table.float().double()), padding=1) + shift[None, :, None, None])
    for b in range(blocks):
        w1, b1 = folded("resblocks.%d.conv1.weight" % b, "resblocks.%d.bn1" % b, r16)
        w2, b2 = folded("resblocks.%d.conv2.weight" % b, "resblocks.%d.bn2" % b, r16)
        y = F.relu(F.conv2d(r16(x), w1, padding=1) + b1)
        x = F.relu(F.conv2d(r16(y), w2, padding=1) + b2 + x)        # the residual is the unrounded block input
    same = lambda t: t                                       # noqa: E731  (the heads: fp32 from the unrounded `act`)
    wv, bv = folded("value_conv1.weight", "value_bn1", same)
    wp, bp = folded("move_conv1.weight", "move_bn1", same)
    v = F.relu(F.conv2d(x, wv) + bv).flatten(1)
    v = F.linear(F.relu(F.linear(v, g("value_fc2.weight"), g("value_fc2.bias"))), g("value_fc3.weight"), g("value_fc3.bias"))
    p = F.relu(F.conv2d(x, wp) + bp).flatten(1)
    logit = F.linear(p, g("move_fc.weight"), g("move_fc.bias"))
    logit = torch.gather(logit, 1, (legal_moves - 1).clamp(min=0)).masked_fill(legal_moves == 0, -99)
    return torch.tanh(v).squeeze(1).numpy(), F.log_softmax(logit, dim=1).numpy()


# name: (board size, blocks, channels, boards, seed) -- the smallest shapes at which the wide kernel can still go wrong:
# 25 cells (position wave 1 owns no valid row, one column block, fewer boards than a group of 8); 81 cells (wave 1 owns
# exactly row 80, three blocks of residual in place); 13x13 with two column blocks and 11 boards (two groups, an 8 + 3
# split over two streams); configs[4]'s depth
FIXTURES = {"5x5": (5, 1, 128, 5, 31), "9x9": (9, 3, 128, 9, 41), "13x13": (13, 2, 256, 11, 51), "19x256": (13, 19, 256, 4, 61)}


def seeded_net(n, blocks, chans, seed):
    """Seeded net with randomised BatchNorm statistics, as test_gpu_tower_f16._seeded_net makes its own."""
    from azalea_amd.network import HexNetwork
    torch.manual_seed(seed)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.3, 1.7)
    return {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}


def positions(n, count, seed):
    rng = np.random.RandomState(seed)
    boards = rng.randint(0, 3, size=(count, n, n)).astype(np.int32)
    boards[:, 0, 0] = 0
    lm = np.zeros((count, n * n), np.int32)
    for i in range(count):
        e = np.flatnonzero(boards[i].ravel() == 0) + 1
        lm[i, :len(e)] = e
    return boards, lm


def exact(n, blocks, chans, state, boards, lm):
    """The float64 HexNetwork's (value, moves_logprob)."""
    from azalea_amd.network import HexNetwork
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).double().eval()
    net.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    with torch.no_grad():
        out = net(torch.as_tensor(boards), torch.as_tensor(lm))
    return out["value"].numpy(), out["moves_logprob"].numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    """One fixture: weights, inputs, the exact float64 module's outputs and the float64 emulation's.  Computed once;
    callers leave the arrays unchanged."""
    n, blocks, chans, count, seed = FIXTURES[name]
    state = seeded_net(n, blocks, chans, seed)
    boards, lm = positions(n, count, seed + 1)
    value, logprob = exact(n, blocks, chans, state, boards, lm)
    ev, elp = forward(state, blocks, boards, lm, rounded=True)
    return dict(n=n, blocks=blocks, chans=chans, state=state, boards=boards, lm=lm, legal=lm > 0,
                value=value, logprob=logprob, emu_value=ev, emu_logprob=elp)
