#!/usr/bin/env python3
"""Training targets of the recorded self-play rows (azx_set_train_targets: visit-share policy rows, z/q-blended
rewards; opt-in, NOT the reference's behaviour) measured at the headline configuration, in ONE process on one GPU.
Recorded, not gated: no test asserts a speed and there is no target.  The option adds a select per stored row element
and three products per harvested row, so plies/s, rows/s and games/s should be EQUAL with the option on and off.

  4096 games, 11x11, golden G8's weights (the reference's trained 6x64 network), 400 simulations in batches of 10,
  exploration_depth 15, the default pipelined loop, every game from the empty board.

  Option off against on (("visits", 0.5)): after `--warmup` play_steps (past the first games' common start),
  `--repeats` runs of `--steps` play_steps each, alternating; medians and spread (max - min) / median of plies/s,
  finished games/s and recorded rows/s.  The games of the two engines are the same games (the option never touches the
  move draw), which the equal ply, game and row counts of every pair of runs show (asserted).

  Then what the rows look like, on the engine with the option on, set to ("visits", 0.0) so that the stored reward is z
  and row metric 7 is v: one play() of at least `--rows` rows.  From azx_train_targets_stats the share of greedy rows
  (ply >= exploration_depth) with more than one visited child -- the rows that differ from the reference's one-hot
  rows; from the rows the mean entropy (nats) of the greedy rows and of all rows, and the mean |z - v| over the rows.

    python tools/bench_train_targets.py [--steps 40] [--repeats 3] [--warmup 100] [--rows 20000]
One JSON line.  profiles/train_targets_bench.json holds it under "train_targets"; under "bench_py_option_never_set" the
same file holds bench.py's runs with the option never set, this build and the parent commit's library alternating
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
ON = ("visits", 0.5)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIGURES = ("plies_per_sec", "games_per_sec", "recorded_rows_per_sec")


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


def one_run(E, steps):
    st = E.play_steps(steps)
    return {"plies_per_sec": st["plies"] / st["seconds"], "games_per_sec": st["games"] / st["seconds"],
            "recorded_rows_per_sec": st["positions"] / st["seconds"], "plies": st["plies"], "games": st["games"],
            "rows": st["positions"], "seconds": st["seconds"]}


def row_figures(E, min_rows):
    """One play() with the stored reward z and metric 7 v: the statistics' shares, entropies, mean |z - v|."""
    E.set_train_targets("visits", 0.0)
    rows, st = E.play(min_rows)
    m = E.play_row_metrics()
    ts = E.train_targets_stats()
    p = rows["moves_prob"].astype(np.float64)
    ent = -(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)).sum(1)
    ply = (rows["board"].reshape(len(p), -1) != 0).sum(1)
    greedy = ply >= DEPTH
    z, v = rows["reward"].astype(np.float64), m[:, 7].astype(np.float64)
    assert (np.abs(z) == 1).all() and np.isfinite(v).all()
    return {"rows": int(len(p)), "games": int(st["games"]), "stats": ts,
            "greedy_share_of_rows_written": ts["greedy_rows"] / max(ts["rows"], 1),
            "share_of_greedy_rows_with_more_than_one_visited_child": ts["greedy_rows_wide"] / max(ts["greedy_rows"], 1),
            "mean_entropy_greedy_rows_nats": float(ent[greedy].mean()),
            "mean_entropy_all_rows_nats": float(ent.mean()),
            "mean_visited_children_greedy_rows": float(m[greedy, 1].mean()),
            "mean_abs_z_minus_v": float(np.abs(z - v).mean()),
            "mean_abs_z_minus_v_greedy_rows": float(np.abs(z - v)[greedy].mean()),
            "mean_v_times_z": float((v * z).mean())}


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
           "steps": args.steps, "repeats": args.repeats, "warmup": args.warmup, "on": list(ON)}
    engines = {"off": headline_engine(state), "on": headline_engine(state)}
    runs = {name: [] for name in engines}
    try:
        engines["on"].set_train_targets(*ON)
        for E in engines.values():
            E.play_steps(args.warmup)         # past the first games' common start: games end and restart out of phase
        for _ in range(args.repeats):
            for name, E in engines.items():
                r = one_run(E, args.steps)
                runs[name].append(r)
                print("%s: %r" % (name, r), file=sys.stderr, flush=True)
            a, b = runs["off"][-1], runs["on"][-1]
            assert (a["plies"], a["games"], a["rows"]) == (b["plies"], b["games"], b["rows"]), (a, b)
        for name, E in engines.items():
            out = {"kernel_info": E.kernel_info(), "runs": runs[name]}
            for f in FIGURES:
                xs = [r[f] for r in runs[name]]
                out[f] = {"median": statistics.median(xs), "spread": spread(xs)}
            res[name] = out
        res["on_over_off"] = {f: res["on"][f]["median"] / res["off"][f]["median"] for f in FIGURES}
        res["same_games"] = "equal ply, game and row counts in every pair of runs"
        res["rows"] = row_figures(engines["on"], args.rows)
    finally:
        for E in engines.values():
            E.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
