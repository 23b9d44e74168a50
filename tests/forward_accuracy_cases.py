"""Fixtures, the float64 truth and the bounds of tests/test_gpu_forward_accuracy.py (the default, fp32-class towers held
to the exact float64 module in units of fp32's own error), pinned on the CPU by tests/test_forward_accuracy_cases.py.
A plain module, no test in it.

A fixture is a network shape with an odd number of positions on random boards and two weight sets:
  "plain"   a seeded net with randomised BatchNorm statistics, as the other forward tests make theirs;
  "peaked"  the same net with move_fc (weight and bias) scaled by one factor and value_fc3 by another, so that it looks
            like a trained one where it matters for accuracy: the median over rows of (max - min legal logit) is at
            least the median of the same quantity over golden G8's recorded moves_logprob, and at least a quarter of
            the values have |v| > 0.9.  The factors are computed in float64 from those two conditions; only layers
            behind the tower are scaled, so the activations stay where the plain net has them (max_act, far inside the
            f16 range -- tests/test_gpu_weights.py owns the range edge).
Each weight set carries the outputs of HexNetwork(...).double() -- the truth -- and of the same module in fp32 on the
CPU, whose largest distances from the truth on the value and on the legal log-probabilities are the units e32_v and
e32_lp.  Golden G8 (the reference's trained 6x64 checkpoint with its recorded positions) is a fixture too.

A case is a fixture under a set of environment switches: CASES lists them with the tower family whose bound holds
them; expected_kernels() says what azx_net_create dispatches a shape to."""
import functools
import os
from contextlib import contextmanager

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("plain", "peaked")

# name: (board size, blocks, channels, positions, seed) -- the smallest shapes that reach every tower kernel and every
# tiling edge; 33 positions: an odd count, so the last block / tile of every kernel is ragged
FIXTURES = {
    "11x11_2x64": (11, 2, 64, 33, 101),      # fused: edge tiles on the largest board they cover
    "5x5_1x64": (5, 1, 64, 7, 102),          # fused: 7 boards (a dead partner board), rows >= ncells
    "8x8_2x64": (8, 2, 64, 33, 103),
    "2x2_1x64": (2, 1, 64, 33, 104),
    "g8": None,                              # fused: the trained checkpoint, 6x64 on 11x11, 48 recorded positions
    "11x11_1x64": (11, 1, 64, 33, 105),      # <64,4,2,1,2> (under AZX_TOWER=fp32)
    "13x13_2x64": (13, 2, 64, 33, 106),      # <64,6,1,2,2>
    "12x12_1x64": (12, 1, 64, 33, 107),
    "13x13_2x32": (13, 2, 32, 33, 108),      # <32,6,2,2,1>
    "9x9_1x32": (9, 1, 32, 33, 109),
    "13x13_2x128": (13, 2, 128, 33, 110),    # wide split-f16
    "12x12_1x256": (12, 1, 256, 33, 111),
    "5x5_0x128": (5, 0, 128, 33, 112),       # the stem alone
    "11x11_2x128": (11, 2, 128, 35, 113),    # 35 boards: split over streams with a ragged part
    "7x7_1x16": (7, 1, 16, 33, 114),         # VALU pair
    "13x13_1x48": (13, 1, 48, 33, 115),
}

FUSED, WIDE, FP32 = "split-f16 fused", "split-f16 wide", "exact fp32"

# case id: (fixture, environment around the creation of the engine, tower family)
CASES = {
    "11x11_2x64": ("11x11_2x64", {}, FUSED),
    "5x5_1x64": ("5x5_1x64", {}, FUSED),
    "8x8_2x64": ("8x8_2x64", {}, FUSED),
    "2x2_1x64": ("2x2_1x64", {}, FUSED),
    "g8": ("g8", {}, FUSED),
    "11x11_2x64_rows": ("11x11_2x64", {"AZX_TOWER_TILES": "rows"}, FUSED),
    "11x11_2x64_heads_valu": ("11x11_2x64", {"AZX_HEADS": "valu"}, FUSED),
    "11x11_1x64_fp32": ("11x11_1x64", {"AZX_TOWER": "fp32"}, FP32),
    "13x13_2x64": ("13x13_2x64", {}, FP32),
    "12x12_1x64": ("12x12_1x64", {}, FP32),
    "13x13_2x32": ("13x13_2x32", {}, FP32),
    "9x9_1x32": ("9x9_1x32", {}, FP32),
    "13x13_2x128": ("13x13_2x128", {}, WIDE),
    "12x12_1x256": ("12x12_1x256", {}, WIDE),
    "5x5_0x128": ("5x5_0x128", {}, WIDE),
    "11x11_2x128_35": ("11x11_2x128", {}, WIDE),
    "7x7_1x16": ("7x7_1x16", {}, FP32),
    "13x13_1x48": ("13x13_1x48", {}, FP32),
}
# (case, kind) pairs of the GPU test: every case with both weight sets, the scalar heads once (behind the peaked net)
PAIRS = [(c, k) for c in CASES for k in KINDS if c != "11x11_2x64_heads_valu" or k == "peaked"]

# The bounds: max |kernel - truth| <= R * e32 + floor.  R per tower family is twice the worst ratio (error - floor) / e32
# measured on an MI355X (profiles/forward_accuracy.json: 2.16, 4.56, 2.10), rounded up to an integer; the factor of two
# covers summation order (the plain-f16 tests measured 1.3x) and the variation of torch's CPU kernels from box to box.
# The floors guard against a lucky e32: half an ulp of fp32 at the output's size.  The wide family's larger ratio is
# the split's own: with 1152 and more terms per sum, its float64 definition (22-bit operands, exact sums) is already
# 4.9 e32 from the truth on the value of the peaked 11x11 2x128 fixture, and the wide kernels also carry the residual
# stream between their launches as hi + lo pairs.
R = {FUSED: 5, WIDE: 10, FP32: 5}
FLOOR_V = 2.0 ** -24


def floor_lp(fx):
    return 2.0 ** -24 * float(np.abs(fx["logprob"][fx["legal"]]).max())


@contextmanager
def environ(**env):
    """The switches are read once, by azx_create: set them around the creation of an engine."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def expected_kernels(n, blocks, chans, env=None):
    """What azx_net_create dispatches (n, blocks, chans) to under `env`, as kernel_info() begins: '<tower> + <heads> ('."""
    env = env or {}
    cells, fp32 = n * n, env.get("AZX_TOWER") == "fp32"
    fused = chans == 64 and cells <= 121 and blocks >= 1 and not fp32
    if fused:
        tower = "k_tower_f16x3_s16"
    elif chans == 64 and cells <= 128:
        tower = "k_tower_mfma<64,4,2,1,2> (fp32 MFMA)"
    elif chans == 64 and cells <= 192:
        tower = "k_tower_mfma<64,6,1,2,2> (fp32 MFMA)"
    elif chans == 32 and cells <= 192:
        tower = "k_tower_mfma<32,6,2,2,1> (fp32 MFMA)"
    elif chans % 128 == 0 and cells <= 192 and not fp32:
        tower = "k_stem_wide_f16x3 + k_conv_wide_f16x3_s16 per layer"
    else:
        tower = "k_stem_generic + k_conv_generic (VALU)"
    heads = "k_heads_mfma" if fused and env.get("AZX_HEADS") != "valu" else "k_heads"
    return "%s + %s (" % (tower, heads)


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


def logit_gaps(logprob, legal):
    """Per row, max - min over the legal entries: of log-probabilities or of logits, their differences are the same."""
    return np.array([row[ok].max() - row[ok].min() for row, ok in zip(logprob, legal) if ok.sum() > 1])


@functools.lru_cache(maxsize=None)
def g8_median_gap():
    z = np.load(os.path.join(GOLDEN, "g8_checkpoint.npz"))
    return float(np.median(logit_gaps(z["moves_logprob"].astype(np.float64), z["legal_moves"] > 0)))


SATURATED, SATURATED_SHARE = 0.9, 0.25       # "peaked": at least this share of the values has |v| above this


def _module(n, blocks, chans, state, dtype):
    from azalea_amd.network import HexNetwork
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).to(dtype).eval()
    net.load_state_dict({k: torch.as_tensor(v) for k, v in state.items()})
    return net


def _outputs(n, blocks, chans, state, boards, lm, dtype):
    with torch.no_grad():
        out = _module(n, blocks, chans, state, dtype)(torch.as_tensor(boards), torch.as_tensor(lm))
    return out["value"].double().numpy(), out["moves_logprob"].double().numpy()


def _peaked(n, blocks, chans, state, boards, lm):
    """`state` with move_fc and value_fc3 scaled -- by the smallest factors, never below 1, that meet the two conditions
    on these positions, found in float64: logits and the value's pre-activation are linear in their factor."""
    net = _module(n, blocks, chans, state, torch.float64)
    seen = {}
    hook = net.value_fc3.register_forward_hook(lambda m, i, o: seen.__setitem__("u", o.detach().squeeze(1).numpy()))
    with torch.no_grad():
        out = net(torch.as_tensor(boards), torch.as_tensor(lm))
    hook.remove()
    gap = float(np.median(logit_gaps(out["moves_logprob"].numpy(), lm > 0)))
    need = int(np.ceil(SATURATED_SHARE * len(boards)))
    u = np.sort(np.abs(seen["u"]))[::-1][need - 1]                  # the need-th largest |pre-activation|
    margin = 1.0 + 2.0 ** -6                                        # strictly above both thresholds
    s_p = max(1.0, margin * g8_median_gap() / gap)
    s_v = max(1.0, margin * float(np.arctanh(SATURATED)) / float(u))
    peaked = {k: v.copy() for k, v in state.items()}
    for k, s in (("move_fc.weight", s_p), ("move_fc.bias", s_p), ("value_fc3.weight", s_v), ("value_fc3.bias", s_v)):
        peaked[k] = (peaked[k].astype(np.float64) * s).astype(np.float32)
    return peaked, s_p, s_v


def _max_activation(n, blocks, chans, state, boards, lm):
    """The largest |activation| the tower writes (every BatchNorm output and block output), in float64."""
    from azalea_amd.network import Resblock
    net = _module(n, blocks, chans, state, torch.float64)
    top = [0.0]
    for m in net.modules():
        if isinstance(m, (torch.nn.BatchNorm2d, Resblock)):
            m.register_forward_hook(lambda m, i, o: top.__setitem__(0, max(top[0], float(o.abs().max()))))
    with torch.no_grad():
        net(torch.as_tensor(boards), torch.as_tensor(lm))
    return top[0]


@functools.lru_cache(maxsize=None)
def fixture(name, kind):
    """One fixture with one weight set: weights, inputs, the float64 module's outputs (the truth), the fp32 CPU module's
    distances from them (the units) and the scale factors.  Computed once; callers leave the arrays unchanged."""
    assert kind in KINDS
    if name == "g8":
        z = np.load(os.path.join(GOLDEN, "g8_checkpoint.npz"))
        n, blocks, chans = [int(x) for x in z["cfg"]]
        state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
        boards, lm = z["board"], z["legal_moves"]
    else:
        n, blocks, chans, count, seed = FIXTURES[name]
        state = seeded_net(n, blocks, chans, seed)
        boards, lm = positions(n, count, seed + 1000)
    s_p = s_v = 1.0
    if kind == "peaked":
        state, s_p, s_v = _peaked(n, blocks, chans, state, boards, lm)
    legal = lm > 0
    value, logprob = _outputs(n, blocks, chans, state, boards, lm, torch.float64)
    v32, lp32 = _outputs(n, blocks, chans, state, boards, lm, torch.float32)
    return dict(n=n, blocks=blocks, chans=chans, state=state, boards=boards, lm=lm, legal=legal, value=value,
                logprob=logprob, e32_v=float(np.abs(v32 - value).max()), e32_lp=float(np.abs(lp32 - logprob)[legal].max()),
                s_p=s_p, s_v=s_v, max_act=_max_activation(n, blocks, chans, state, boards, lm))


def errors(fx, value, logprob):
    """(max |value - truth|, max over legal entries |logprob - truth|) of one set of outputs on a fixture."""
    return (float(np.abs(np.asarray(value, np.float64) - fx["value"]).max()),
            float(np.abs(np.asarray(logprob, np.float64) - fx["logprob"])[fx["legal"]].max()))


def bounds(fx, family):
    return R[family] * fx["e32_v"] + FLOOR_V, R[family] * fx["e32_lp"] + floor_lp(fx)
