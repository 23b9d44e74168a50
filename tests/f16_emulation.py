"""Float64 torch emulation of the plain-f16 tower (AZX_FLAG_TOWER_F16, k_tower_f16_s16): the yardstick of
tests/test_gpu_tower_f16.py, pinned by tests/test_tower_f16_emulation.py.  A plain module, no test in it.

The definition (include/azx.h): BatchNorm folded into the convolutions and the 3 -> 4 embedding folded into the stem
as the weight packer does it (scale = w / sqrt(var + 1e-5), shift = b - mean * scale in f64, the products stored as
fp32); the folded stem, conv and head-filter weights enter as f16(w); the activation written back after each ReLU
enters the next conv and the head filters as f16(a); sums, bias and the residual (the unrounded block input) are not
rounded -- float64 here, fp32 in the kernel; the one-hot stem input is exact; the heads behind the six planes are
unchanged.  rounded=False leaves every f16 rounding out: the network itself."""
import numpy as np
import torch
from torch.nn import functional as F


def _fold(state, pre):
    w, b, m, v = (torch.as_tensor(state[pre + k]).double() for k in (".weight", ".bias", ".running_mean", ".running_var"))
    scale = w / torch.sqrt(v + 1e-5)
    return scale, (b - m * scale).float().double()


def _lo_half(rem, bits):
    """f16(rem) kept to `bits` explicit mantissa bits, rounded to nearest on the f16 pattern (half away from zero, a carry
    into the exponent included) as lo_round_bits / split2_f16 do it in a build with AZX_LO_BITS = bits; 10 keeps all."""
    assert 0 <= bits <= 10
    pat = rem.float().half().contiguous().view(torch.int16).numpy().view(np.uint16).astype(np.uint32)
    if bits < 10:
        pat = (pat + (1 << (9 - bits))) & ((0xFFFF << (10 - bits)) & 0xFFFF)
    return torch.from_numpy(pat.astype(np.uint16).view(np.int16)).view(torch.float16).double()


def forward(state, blocks, board, legal_moves, rounded=True, lo_bits=None):
    """(value [B], moves_logprob [B, K]) as float64 numpy arrays; `state`: the HexNetwork state dict (numpy or torch).

    lo_bits = b (default None: the plain-f16 tower above) makes every rounded operand hi + lo_b instead of hi, with
    hi = f16(x) and lo_b = f16(x - hi) kept to b mantissa bits: the definition of the default tower's hi + lo split
    (k_tower_f16x3_s16; b = 10 is the shipped one, fewer bits are the AZX_LO_BITS diagnostic builds) in float64.  The
    lo * lo product the kernel drops, 2^-22 of the result, stays in."""
    if not rounded:
        r16 = lambda t: t                                       # noqa: E731
    elif lo_bits is None:
        r16 = lambda t: t.float().half().double()               # noqa: E731
    else:
        def r16(t):
            hi = t.float().half().double()
            return hi + _lo_half(t - hi, lo_bits)
    g = lambda name: torch.as_tensor(state[name]).double()   # noqa: E731
    board, legal_moves = torch.as_tensor(board).long(), torch.as_tensor(legal_moves).long()

    def folded(conv, bn):
        scale, shift = _fold(state, bn)
        return r16((g(conv) * scale[:, None, None, None]).float().double()), shift[None, :, None, None]

    # stem: T[co][v] per tap = scale[co] * sum_i emb[v][i] * w[co][i][tap]; zero padding = no contribution off the board
    scale, shift = _fold(state, "bn1")
    table = torch.einsum("vi,oiyx->ovyx", g("encoder.weight"), g("conv1.weight")) * scale[:, None, None, None]
    onehot = F.one_hot(board, 3).permute(0, 3, 1, 2).double()
    x = F.relu(F.conv2d(onehot, r16(table.float().double()), padding=1) + shift[None, :, None, None])
    for b in range(blocks):
        w1, b1 = folded("resblocks.%d.conv1.weight" % b, "resblocks.%d.bn1" % b)
        w2, b2 = folded("resblocks.%d.conv2.weight" % b, "resblocks.%d.bn2" % b)
        y = F.relu(F.conv2d(r16(x), w1, padding=1) + b1)
        x = F.relu(F.conv2d(r16(y), w2, padding=1) + b2 + x)        # the residual is the unrounded block input
    wv, bv = folded("value_conv1.weight", "value_bn1")
    wp, bp = folded("move_conv1.weight", "move_bn1")
    xr = r16(x)
    v = F.relu(F.conv2d(xr, wv) + bv).flatten(1)
    v = F.linear(F.relu(F.linear(v, g("value_fc2.weight"), g("value_fc2.bias"))), g("value_fc3.weight"), g("value_fc3.bias"))
    p = F.relu(F.conv2d(xr, wp) + bp).flatten(1)
    logit = F.linear(p, g("move_fc.weight"), g("move_fc.bias"))
    logit = torch.gather(logit, 1, (legal_moves - 1).clamp(min=0)).masked_fill(legal_moves == 0, -99)
    return torch.tanh(v).squeeze(1).numpy(), F.log_softmax(logit, dim=1).numpy()
