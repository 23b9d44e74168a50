"""Writes tests/golden/tower_forward_digests.json: what every tower azx_net_create can choose packs and computes, as
digests, one case per row of the choice's table at the smallest shape that reaches it.
tests/test_gpu_tower_choice_digests.py reads the file, runs the same cases through `run_case` below and compares; it
never writes it.

Made ONCE, on the commit BEFORE the choice of the tower was folded into one descriptor (TowerChoice, net_priv.h),
with that commit's library: the fixture is what says the descriptor hands the packers and the launches what the integer
`tower_variant` and its re-derivations did.  Needs a GPU.  Every case is run twice and nothing is written when the two
runs differ.

    python tests/golden/make_tower_forward_digests.py

A case is a seeded HexNetwork with perturbed BatchNorm statistics on 8 positions (empty, nearly full, random), under an
engine flag and a set of environment switches.  Per case the fixture holds the `net=` field of azx_kernel_info, the
digest of the packed operands under the device pack and under AZX_PACK=host (the same: the two packs are bit-identical)
and a SHA-256 over the bytes of forward()'s values and log-probabilities.
"""
import hashlib
import json
import os
import re
import sys
from contextlib import contextmanager

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "tower_forward_digests.json")

SEED, POSITIONS = 20261021, 8
F16 = 4                     # AZX_FLAG_TOWER_F16

# name: (board size, blocks, channels, engine flags, environment around the creation of the engine)
CASES = {
    "generic": (5, 1, 16, 0, {}),
    "mfma_64_4": (5, 0, 64, 0, {}),
    "mfma_64_6": (12, 1, 64, 0, {}),
    "mfma_32_6": (5, 1, 32, 0, {}),
    "fused": (5, 1, 64, 0, {}),
    "fused_f16": (5, 1, 64, F16, {}),
    "fused_rows": (5, 1, 64, 0, {"AZX_TOWER_TILES": "rows"}),
    "fused_heads_valu": (5, 1, 64, 0, {"AZX_HEADS": "valu"}),
    "fused_fp32": (5, 1, 64, 0, {"AZX_TOWER": "fp32"}),
    "wide": (5, 1, 128, 0, {}),
    "wide_f16": (5, 1, 128, F16, {}),
    "wide_streams1": (5, 1, 128, 0, {"AZX_WIDE_STREAMS": "1"}),
    "wide_stem": (5, 0, 128, 0, {}),
}
SWITCHES = ("AZX_TOWER", "AZX_TOWER_TILES", "AZX_WIDE_STREAMS", "AZX_HEADS", "AZX_PACK")


def seeded_state(n, blocks, chans):
    import torch
    from azalea_amd.network import HexNetwork
    torch.manual_seed(SEED + 1000 * n + 10 * chans + blocks)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.3, 1.7)
    return {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}


def positions(n):
    """POSITIONS boards: the empty one, one with a single empty cell, random ones; and their legal-move rows."""
    rng = np.random.RandomState(SEED + n)
    boards = rng.randint(0, 3, size=(POSITIONS, n, n)).astype(np.int32)
    boards[0] = 0
    boards[1] = rng.randint(1, 3, size=(n, n))
    boards[1, n // 2, n - 1] = 0
    boards[2:, 0, 0] = 0
    lm = np.zeros((POSITIONS, n * n), np.int32)
    for i in range(POSITIONS):
        e = np.flatnonzero(boards[i].ravel() == 0) + 1
        lm[i, :len(e)] = e
    return boards, lm


@contextmanager
def switches(env):
    """The switches are read once, by azx_create: every one of them is set as `env` has it or removed around it."""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def make_engine(n, blocks, chans, flags, env):
    from azalea_amd import engine as eng
    with switches(env):
        return eng.Engine(board_size=n, n_games=POSITIONS, simulations=8, search_batch_size=1,
                          evaluator=eng.EVAL_RESNET, num_blocks=blocks, base_chans=chans, flags=flags)


def net_field(info):
    return re.search(r"; net=(.*?); switches:", info).group(1)


def run_case(case):
    n, blocks, chans, flags, env = case
    state = seeded_state(n, blocks, chans)
    boards, lm = positions(n)
    out = {}
    for pack in ("device", "host"):
        E = make_engine(n, blocks, chans, flags, dict(env, AZX_PACK=pack))
        try:
            E.set_weights(state)
            out["weights_" + pack] = E.weights_digest()
            if pack == "device":
                out["net"] = net_field(E.kernel_info())
                value, logprob = E.forward(boards, lm)
                h = hashlib.sha256()
                h.update(np.ascontiguousarray(value).tobytes())
                h.update(np.ascontiguousarray(logprob).tobytes())
                out["forward"] = h.hexdigest()
        finally:
            E.close()
    return out


def collect():
    return dict(seed=SEED, positions=POSITIONS, cases={name: run_case(case) for name, case in CASES.items()})


def main():
    sys.path.insert(0, ROOT)
    first, second = collect(), collect()
    if first != second:
        for name in first["cases"]:
            if first["cases"][name] != second["cases"][name]:
                print("case %s differs between two runs:\n  %r\n  %r" % (name, first["cases"][name], second["cases"][name]))
        raise SystemExit("two runs differ: nothing written")
    with open(FIXTURE, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (FIXTURE, len(first["cases"])))


if __name__ == "__main__":
    main()
