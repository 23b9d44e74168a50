#!/usr/bin/env python3
"""Resignation of device self-play (azx_set_resign; opt-in, NOT the reference's behaviour) measured at the headline
configuration, in ONE process on one GPU.  Recorded, not gated: no test asserts a speed, and nothing here says anything
about playing strength or training efficiency -- neither is measured.

  4096 games, 11x11, golden G8's weights (the reference's trained 6x64 network: a random network's values sit near 0
  and never resign), 400 simulations in batches of 10, the default pipelined loop, every game from the empty board.

  (a) calibration: keep_prob = 1 (every game exempt: nobody resigns, every crossing is counted) at each of
      --thresholds with min_ply 10, `--calib-steps` play_steps each on a fresh engine; from azx_resign_stats the
      false-positive rate (exempt games whose would-be resigner went on to win / exempt games with a crossing) and the
      plies a resignation would have saved.
  (b) throughput: the loosest of those thresholds whose measured false-positive rate is at most 5 % (AlphaGo Zero's
      criterion; -0.95 if none qualifies, and the result says so), keep_prob = 0.1, against resignation off: after a
      warm-up `--repeats` runs of `--steps` play_steps each, alternating, medians and spread (max - min) / median of
      games/s, plies/s, recorded rows/s and the mean length of the games finished.

    python tools/bench_resign.py [--calib-steps 130] [--steps 40] [--repeats 3] [--warmup 100]
One JSON line.  profiles/resign_bench.json holds it under "resign"; under "bench_py_resignation_never_set" the same
file holds bench.py's runs with resignation never set, this build and the parent commit's library alternating
(tools/lib_bench.py), with the medians, the min-max spreads and the criterion."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from azalea_amd import engine as eng

BOARD, GAMES, BATCH = 11, 4096, 10
BLOCKS, CHANS, SIMS = 6, 64, 400
MIN_PLY, KEEP_PROB, MAX_FALSE_POSITIVE = 10, 0.1, 0.05
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIGURES = ("games_per_sec", "plies_per_sec", "recorded_rows_per_sec", "mean_game_length")


def golden_state(name):
    z = np.load(os.path.join(GOLDEN, name))
    assert [int(x) for x in z["cfg"]] == [11, 6, 64]
    return {k[2:]: z[k] for k in z.files if k.startswith("w:")}


def headline_engine(state):
    E = eng.Engine(board_size=BOARD, n_games=GAMES, simulations=SIMS, search_batch_size=BATCH, exploration_coef=0.5,
                   exploration_depth=15, noise_alpha=0.03, noise_scale=0.25, temperature=1.0,
                   evaluator=eng.EVAL_RESNET, num_blocks=BLOCKS, base_chans=CHANS)
    E.set_weights(state)
    return E


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs) if statistics.median(xs) else 0.0


def calibrate(state, threshold, steps):
    E = headline_engine(state)
    try:
        E.set_resign(threshold, MIN_PLY, 1.0)
        st = E.play_steps(steps)
        rs = E.resign_stats()
    finally:
        E.close()
    crossed = rs["exempt_crossed"]
    return {"threshold": threshold, "min_ply": MIN_PLY, "steps": steps, "games": rs["exempt"], "crossed": crossed,
            "false_positives": rs["false_positives"],
            "false_positive_rate": rs["false_positives"] / max(crossed, 1),
            "share_crossing": crossed / max(rs["exempt"], 1),
            "plies_saved": rs["sum_plies_saved"],
            "plies_saved_per_game": rs["sum_plies_saved"] / max(rs["exempt"], 1),
            "mean_game_length": st["sum_game_length"] / max(st["games"], 1),
            "plies_per_sec": st["plies"] / st["seconds"]}


def one_run(E, steps):
    st = E.play_steps(steps)
    return {"games_per_sec": st["games"] / st["seconds"], "plies_per_sec": st["plies"] / st["seconds"],
            "recorded_rows_per_sec": st["positions"] / st["seconds"],
            "mean_game_length": st["sum_game_length"] / max(st["games"], 1),
            "games": st["games"], "plies": st["plies"], "seconds": st["seconds"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--thresholds", type=float, nargs="+", default=[-0.8, -0.9, -0.95])
    ap.add_argument("--calib-steps", type=int, default=130)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--skip-calibration", type=float, default=None, metavar="THRESHOLD",
                    help="run (b) alone at this threshold")
    args = ap.parse_args()
    state = golden_state("g8_checkpoint.npz")
    res = {"board": BOARD, "games": GAMES, "batch": BATCH, "sims": SIMS, "blocks": BLOCKS, "chans": CHANS,
           "weights": "golden G8", "min_ply": MIN_PLY, "device": torch.cuda.get_device_name(0),
           "strength_and_training_efficiency": "NOT measured"}
    if args.skip_calibration is None:
        res["calibration"] = []
        for t in args.thresholds:
            c = calibrate(state, t, args.calib_steps)
            res["calibration"].append(c)
            print("calibration %r" % (c,), file=sys.stderr, flush=True)
        ok = [c["threshold"] for c in res["calibration"]
              if c["crossed"] > 0 and c["false_positive_rate"] <= MAX_FALSE_POSITIVE]
        res["criterion"] = "loosest threshold with a false-positive rate <= %g" % MAX_FALSE_POSITIVE
        res["criterion_met"] = bool(ok)
        threshold = max(ok) if ok else -0.95
    else:
        threshold = args.skip_calibration
    res["throughput"] = {"threshold": threshold, "keep_prob": KEEP_PROB, "steps": args.steps, "repeats": args.repeats,
                         "warmup": args.warmup}
    engines = {"off": headline_engine(state), "resign": headline_engine(state)}
    runs = {name: [] for name in engines}
    try:
        engines["resign"].set_resign(threshold, MIN_PLY, KEEP_PROB)
        for E in engines.values():
            E.play_steps(args.warmup)         # past the first games' common start: games end and restart out of phase
        for _ in range(args.repeats):
            for name, E in engines.items():
                r = one_run(E, args.steps)
                runs[name].append(r)
                print("%s: %r" % (name, r), file=sys.stderr, flush=True)
        for name, E in engines.items():
            out = {"kernel_info": E.kernel_info(), "runs": runs[name]}
            for f in FIGURES:
                xs = [r[f] for r in runs[name]]
                out[f] = {"median": statistics.median(xs), "spread": spread(xs)}
            res["throughput"][name] = out
        res["throughput"]["resign_stats"] = engines["resign"].resign_stats()
        res["throughput"]["resign_over_off"] = {
            f: res["throughput"]["resign"][f]["median"] / res["throughput"]["off"][f]["median"]
            for f in FIGURES if res["throughput"]["off"][f]["median"]}
    finally:
        for E in engines.values():
            E.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
