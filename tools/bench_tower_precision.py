#!/usr/bin/env python3
"""The plain-f16 tower (AZX_FLAG_TOWER_F16, k_tower_f16_s16; opt-in, outside every parity claim) measured against the
split-f16 tower (k_tower_f16x3_s16), in ONE process on one GPU.  Recorded, not gated: no test asserts a speed.

  (a) tower + heads launch time at the headline's batch: 4096 games x 10 rows per evaluation, 11x11, golden G3's 6x64
      weights, the one-stream play loop (AZX_PIPELINE=0, so a network launch overlaps nothing) -- the engine's own
      net_seconds / net_launches over `--steps` moves, with the rows a launch evaluated on average beside it
  (b) play_steps of the headline configuration (400 simulations, the default pipelined loop), plies per second
      (a) and (b): both precisions, `--repeats` runs each, alternating, medians and spread (max - min) / median
  (c) evaluate_throughput of golden G8's weights (the reference's trained 6x64 network) against themselves, one agent
      with tower_precision="f16", `--games` games at `--sims` simulations, move sampling on: the f16 side's share of
      the wins with its binomial (Wilson) 95 % interval

    python tools/bench_tower_precision.py [--steps 10] [--repeats 3] [--games 400] [--sims 400]
One JSON line (profiles/tower_f16_bench.json).

--wide: the same (a) and (b) for the wide tower (k_conv_wide_f16_s16 against k_conv_wide_f16x3_s16) at the shape and
batch of bench.py's config5 leg: 13x13, 19x256, 512 games x 10 rows per evaluation, 800 simulations, a seeded
randomly initialised network (speed does not depend on the weights).  No (c): no trained wide checkpoint exists, so
strength at the two precisions is NOT measured.
    python tools/bench_tower_precision.py --wide [--steps 2] [--repeats 3]      (profiles/wide_f16_bench.json)"""
import argparse
import json
import math
import os
import statistics
import sys

os.environ.pop("AZX_TOWER", None)      # the lenient AZX_TOWER=f16 would put the plain tower on both sides
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from azalea_amd import engine as eng
from azalea_amd import evaluation
from azalea_amd.azalea_agent import AzaleaAgent
from azalea_amd.game.hex import HexGame
from azalea_amd.policy import Policy

BOARD, GAMES, BATCH = 11, 4096, 10
BLOCKS, CHANS, SIMS, DESYNC = 6, 64, 400, 92
GOLDEN = os.path.join(ROOT, "tests", "golden")
PRECISIONS = (("f16x3", 0), ("f16", eng.FLAG_TOWER_F16))


def golden_state(name):
    z = np.load(os.path.join(GOLDEN, name))
    assert [int(x) for x in z["cfg"]] == [11, 6, 64]
    return {k[2:]: z[k] for k in z.files if k.startswith("w:")}


def seeded_state(board, blocks, chans, seed=0):
    from azalea_amd.network import HexNetwork
    torch.manual_seed(seed)
    net = HexNetwork(board_size=board, num_blocks=blocks, base_chans=chans).eval()
    return {k: v.detach().numpy() for k, v in net.state_dict().items()}


def headline_engine(flags, sims, state, pipeline):
    """bench.py's headline engine (--wide: its config5 leg's) with the pool started out of phase (random prefixes of
    0..DESYNC plies)."""
    if pipeline:
        os.environ.pop("AZX_PIPELINE", None)
    else:
        os.environ["AZX_PIPELINE"] = "0"                 # read once, by azx_create
    try:
        E = eng.Engine(board_size=BOARD, n_games=GAMES, simulations=sims, search_batch_size=BATCH, exploration_coef=0.5,
                       exploration_depth=15, noise_alpha=0.03, noise_scale=0.25, temperature=1.0,
                       evaluator=eng.EVAL_RESNET, num_blocks=BLOCKS, base_chans=CHANS, flags=flags)
    finally:
        os.environ.pop("AZX_PIPELINE", None)
    E.set_weights(state)
    E.reset(moves=eng.random_prefixes(BOARD, np.arange(GAMES, dtype=np.int64), DESYNC, 1))
    E.play_steps(1 if CHANS > 64 else 2)
    return E


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs)


def alternate(engines, steps, repeats, figure):
    runs = {name: [] for name in engines}
    extra = {}
    for _ in range(repeats):
        for name, E in engines.items():
            st = E.play_steps(steps)
            runs[name].append(figure(st))
            extra[name] = st
            print("%s: %s" % (name, runs[name][-1]), file=sys.stderr, flush=True)
    return runs, extra


def wilson(k, n, z=1.96):
    p = k / n
    d = 1 + z * z / n
    c = p + z * z / (2 * n)
    h = z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n))
    return (c - h) / d, (c + h) / d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--games", type=int, default=400)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--skip", default="", help="comma list of a, b, c")
    ap.add_argument("--wide", action="store_true", help="the wide tower at bench.py's config5 shape (13x13, 19x256); no (c)")
    args = ap.parse_args()
    skip = set(args.skip.split(","))
    if args.wide:
        global BOARD, GAMES, BLOCKS, CHANS, SIMS, DESYNC
        BOARD, GAMES, BLOCKS, CHANS, SIMS, DESYNC = 13, 512, 19, 256, 800, 128
        skip.add("c")
    if args.steps is None:
        args.steps = 2 if args.wide else 10
    res = {"board": BOARD, "games": GAMES, "batch": BATCH, "device": torch.cuda.get_device_name(0),
           "steps": args.steps, "repeats": args.repeats}
    g3 = seeded_state(BOARD, BLOCKS, CHANS) if args.wide else golden_state("g3_forward_11_6x64.npz")
    # stem + convs + the six head filters: 11.7 MFLOP per 6x64 row on 11x11, 7.58 GFLOP per 19x256 row on 13x13
    flop_per_row = 2.0 * BOARD * BOARD * (27 * CHANS + 2 * BLOCKS * 9 * CHANS * CHANS + 6 * CHANS)
    if args.wide:
        res.update(blocks=BLOCKS, chans=CHANS, sims=SIMS, weights="seeded random initialisation",
                   strength="NOT measured: no trained wide checkpoint exists")

    for leg, pipeline in (("a", False), ("b", True)):
        if leg in skip:
            continue
        engines = {name: headline_engine(flags, SIMS, g3, pipeline) for name, flags in PRECISIONS}
        try:
            if leg == "a":
                runs, last = alternate(engines, args.steps, args.repeats,
                                       lambda st: 1e3 * st["net_seconds"] / max(1, st["net_launches"]))
                out = {"what": "tower + heads, ms per launch (one-stream loop)"}
                for name in engines:
                    ms = statistics.median(runs[name])
                    rows = last[name]["evals"] / max(1, last[name]["net_launches"])
                    out[name] = {"ms_per_launch": runs[name], "median_ms": ms, "spread": spread(runs[name]),
                                 "rows_per_launch": rows, "tflops": flop_per_row * rows / (ms * 1e-3) / 1e12,
                                 "frac_of_f16_mfma_peak": flop_per_row * rows / (ms * 1e-3) / 1e12 / 2500.0,
                                 "kernel_info": engines[name].kernel_info()}
                out["f16x3_over_f16_ms"] = out["f16x3"]["median_ms"] / out["f16"]["median_ms"]
                res["launch"] = out
            else:
                runs, _ = alternate(engines, args.steps, args.repeats, lambda st: st["plies"] / st["seconds"])
                out = {"what": "play_steps, headline configuration, plies per second"}
                for name in engines:
                    out[name] = {"plies_per_sec": runs[name], "median": statistics.median(runs[name]),
                                 "spread": spread(runs[name]), "kernel_info": engines[name].kernel_info()}
                out["f16_over_f16x3"] = out["f16"]["median"] / out["f16x3"]["median"]
                res["play_steps"] = out
        finally:
            for E in engines.values():
                E.close()

    if "c" not in skip:
        g8 = golden_state("g8_checkpoint.npz")
        agents = []
        for prec in ("f16", "f16x3"):
            p = Policy()
            p.initialize(dict(device="cuda:0", network="HexNetwork", board_size=BOARD, num_blocks=6, base_chans=64,
                              simulations=args.sims, search_batch_size=BATCH, exploration_coef=0.5, exploration_depth=15,
                              exploration_noise_alpha=0.03, exploration_noise_scale=0.25, exploration_temperature=1.0))
            p.net.load_state_dict({k: torch.as_tensor(v) for k, v in g8.items()})
            p.net.eval()
            p.settings["move_sampling"] = True
            p.settings["move_exploration"] = False
            p.tower_precision = prec
            agents.append(AzaleaAgent(lambda: HexGame(BOARD), policy=p, device="cuda:0"))
        info, games = {}, {}
        out = evaluation.evaluate_throughput(agents, args.games, n_slots=args.games, seed=1, info=info, games=games)
        wins, _, losses = out[(0, 1)]
        lo, hi = wilson(wins, wins + losses)
        res["match"] = {"weights": "golden G8", "sims": args.sims, "games": wins + losses, "move_sampling": True,
                        "f16_wins": int(wins), "f16x3_wins": int(losses), "f16_win_share": wins / (wins + losses),
                        "wilson_95": [lo, hi], "interval_excludes_half": not (lo <= 0.5 <= hi),
                        "mean_game_length": float(games[(0, 1)]["length"].mean()),
                        "towers": [info[i].split("net=")[-1].split(" + ")[0] for i in (0, 1)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
