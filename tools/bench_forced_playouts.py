#!/usr/bin/env python3
"""Forced playouts and policy target pruning of device self-play (azx_set_forced_playouts; opt-in, NOT the reference's
behaviour) measured at the headline configuration, in ONE process on one GPU.  Recorded, not gated: no test asserts a
speed, no threshold is set in advance, and nothing here says anything about playing strength or training efficiency --
neither is measured.

  4096 games, 11x11, golden G8's weights (the reference's trained 6x64 network), 400 simulations in batches of 10,
  exploration_depth 15, the default pipelined loop, every game from the empty board.

  Option (2.0, prune) against off: after `--warmup` play_steps (past the first games' common start), `--repeats` runs
  of `--steps` play_steps each, alternating; medians and spread (max - min) / median of plies/s, finished games/s,
  recorded rows/s and evaluated rows per ply; from azx_forced_playouts_stats the share of selects whose forced set was
  non-empty and the visits removed per recorded row.  Then one play() of `--rows` rows under each of three settings -- off,
  (2.0, prune), (2.0, noprune) -- gives the mean entropy (nats) of the recorded rows, over all rows and over the rows of
  the plies drawn at T = 1 (ply < exploration_depth; later rows are one-hot whatever the option).

    python tools/bench_forced_playouts.py [--steps 40] [--repeats 3] [--warmup 100] [--rows 20000]
One JSON line.  profiles/forced_playouts_bench.json holds it under "forced_playouts"; under "bench_py_option_never_set"
the same file holds bench.py's runs with the option never set, this build and the parent commit's library alternating
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
BLOCKS, CHANS, SIMS, DEPTH = 6, 64, 400, 15
NB = SIMS // BATCH + 1
K, PRUNE = 2.0, True
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIGURES = ("plies_per_sec", "games_per_sec", "recorded_rows_per_sec", "evals_per_ply")
ON_FIGURES = ("share_of_selects_forced", "visits_removed_per_recorded_row", "share_of_recorded_rows_pruned")


def golden_state(name):
    z = np.load(os.path.join(GOLDEN, name))
    assert [int(x) for x in z["cfg"]] == [11, 6, 64]
    return {k[2:]: z[k] for k in z.files if k.startswith("w:")}


def headline_engine(state):
    E = eng.Engine(board_size=BOARD, n_games=GAMES, simulations=SIMS, search_batch_size=BATCH, exploration_coef=0.5,
                   exploration_depth=DEPTH, noise_alpha=0.03, noise_scale=0.25, temperature=1.0,
                   evaluator=eng.EVAL_RESNET, num_blocks=BLOCKS, base_chans=CHANS)
    E.set_weights(state)
    return E


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs) if statistics.median(xs) else 0.0


def one_run(E, steps, on):
    before = E.forced_playouts_stats()
    st = E.play_steps(steps)
    fs = {k: v - before[k] for k, v in E.forced_playouts_stats().items()}
    plies = st["plies"]
    assert st["selects"] == BATCH * NB * plies, (st["selects"], plies)      # forcing changes where a select goes, not how many
    assert on or fs == dict.fromkeys(fs, 0)
    r = {"plies_per_sec": plies / st["seconds"], "games_per_sec": st["games"] / st["seconds"],
         "recorded_rows_per_sec": st["positions"] / st["seconds"], "evals_per_ply": st["evals"] / plies,
         "plies": plies, "games": st["games"], "seconds": st["seconds"]}
    if on:
        assert fs["full_plies"] == plies
        r.update(share_of_selects_forced=fs["forced_selects"] / st["selects"],
                 visits_removed_per_recorded_row=fs["visits_removed"] / max(plies, 1),
                 share_of_recorded_rows_pruned=fs["rows_pruned"] / max(plies, 1))
    return r


def row_entropy(E, rows):
    """Mean entropy (nats) of the rows of one play(): over all rows, and over the rows of plies drawn at T = 1."""
    got, _ = E.play(rows)
    p = got["moves_prob"].astype(np.float64)
    h = -(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)).sum(1)
    ply = (got["board"].reshape(len(p), -1) != 0).sum(1)
    t1 = ply < DEPTH
    return {"rows": int(len(p)), "mean_entropy": float(h.mean()), "t1_rows": int(t1.sum()),
            "mean_entropy_t1_rows": float(h[t1].mean()), "mean_support_t1_rows": float((p[t1] > 0).sum(1).mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rows", type=int, default=20000)
    args = ap.parse_args()
    state = golden_state("g8_checkpoint.npz")
    res = {"board": BOARD, "games": GAMES, "batch": BATCH, "sims": SIMS, "blocks": BLOCKS, "chans": CHANS,
           "exploration_depth": DEPTH, "weights": "golden G8", "device": torch.cuda.get_device_name(0),
           "k": K, "prune": PRUNE, "steps": args.steps, "repeats": args.repeats, "warmup": args.warmup,
           "strength_and_training_efficiency": "NOT measured"}
    engines = {"off": headline_engine(state), "on": headline_engine(state)}
    runs = {name: [] for name in engines}
    try:
        engines["on"].set_forced_playouts(K, PRUNE)
        for E in engines.values():
            E.play_steps(args.warmup)         # past the first games' common start: games end and restart out of phase
        for _ in range(args.repeats):
            for name, E in engines.items():
                r = one_run(E, args.steps, name == "on")
                runs[name].append(r)
                print("%s: %r" % (name, r), file=sys.stderr, flush=True)
        for name, E in engines.items():
            out = {"kernel_info": E.kernel_info(), "runs": runs[name]}
            for f in FIGURES + (ON_FIGURES if name == "on" else ()):
                xs = [r[f] for r in runs[name]]
                out[f] = {"median": statistics.median(xs), "spread": spread(xs)}
            res[name] = out
        res["on_over_off"] = {f: res["on"][f]["median"] / res["off"][f]["median"]
                              for f in FIGURES if res["off"][f]["median"]}
        # row entropy with and without pruning: the timed engines go on, then the off engine forces without pruning
        entropy = {"off": row_entropy(engines["off"], args.rows), "forced_pruned": row_entropy(engines["on"], args.rows)}
        engines["off"].set_forced_playouts(K, False)
        engines["off"].play_steps(args.warmup)                  # games begun under the new setting replace the old ones
        entropy["forced_not_pruned"] = row_entropy(engines["off"], args.rows)
        res["row_entropy_nats"] = entropy
    finally:
        for E in engines.values():
            E.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
