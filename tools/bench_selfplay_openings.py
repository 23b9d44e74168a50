#!/usr/bin/env python3
"""The weighted opening book of device self-play (azx_set_selfplay_openings; opt-in, NOT the reference's behaviour)
measured at the headline configuration, in ONE process on one GPU.  Recorded, not gated: no test asserts a speed, no
speed-up is claimed.  These are RATES and tallies, not strength: nothing here says anything about playing strength or
training efficiency -- neither is measured.

  4096 games, 11x11, golden G8's weights (the reference's trained 6x64 network), 400 simulations in batches of 10,
  exploration_depth 15, the default pipelined loop.  Book off (every game from the empty board) against the book of all
  121 one-ply openings, uniform.  After `--warmup` play_steps (past the first games' common start), `--repeats` runs of
  `--steps` play_steps each, alternating; medians and spread (max - min) / median of plies/s, finished games/s, recorded
  rows/s, mean length of the finished games (from the empty board) and evaluated rows per ply.  Then the per-opening
  tallies of the book engine since the book was set: games finished and colour 1's share of the wins, by first move --
  which first moves THIS network considers balanced.

    python tools/bench_selfplay_openings.py [--steps 40] [--repeats 3] [--warmup 100]
One JSON line.  profiles/selfplay_openings_bench.json holds it under "selfplay_openings"; under
"bench_py_option_never_set" the same file holds bench.py's runs with the option never set, this build and the parent
commit's library alternating (tools/lib_bench.py), with the medians, the min-max spreads and the criterion."""
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

BOARD, GAMES, BATCH, SIMS = 11, 4096, 10, 400
BLOCKS, CHANS, DEPTH = 6, 64, 15
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIGURES = ("plies_per_sec", "games_per_sec", "recorded_rows_per_sec", "mean_game_length", "evals_per_ply")


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
    plies = st["plies"]
    assert st["selects"] == BATCH * (SIMS // BATCH + 1) * plies, (st["selects"], plies)
    return {"plies_per_sec": plies / st["seconds"], "games_per_sec": st["games"] / st["seconds"],
            "recorded_rows_per_sec": st["positions"] / st["seconds"],
            "mean_game_length": st["sum_game_length"] / max(st["games"], 1), "evals_per_ply": st["evals"] / plies,
            "plies": plies, "games": st["games"], "seconds": st["seconds"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=100)
    args = ap.parse_args()
    state = golden_state("g8_checkpoint.npz")
    book = eng.all_openings(BOARD, 1)
    res = {"board": BOARD, "games": GAMES, "batch": BATCH, "sims": SIMS, "blocks": BLOCKS, "chans": CHANS,
           "exploration_depth": DEPTH, "weights": "golden G8", "device": torch.cuda.get_device_name(0),
           "book": "all %d one-ply openings, uniform" % len(book), "steps": args.steps, "repeats": args.repeats,
           "warmup": args.warmup, "strength_and_training_efficiency": "NOT measured"}
    engines = {"off": headline_engine(state), "book": headline_engine(state)}
    runs = {name: [] for name in engines}
    try:
        engines["book"].set_selfplay_openings(book)
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
            res[name] = out
        st = engines["book"].selfplay_openings_stats()
        fin, won = st["finished"], st["wins_color1"]
        res["book"]["per_opening"] = {
            "first_move_tile_plus_1": [o[0] for o in book], "started": st["started"].tolist(), "finished": fin.tolist(),
            "wins_color1": won.tolist(),
            "win_share_color1": [round(float(w) / f, 4) if f else None for w, f in zip(won.tolist(), fin.tolist())],
            "mean_length": [round(float(p) / f, 2) if f else None for p, f in zip(st["plies"].tolist(), fin.tolist())]}
        res["book"]["win_share_color1_all"] = float(won.sum()) / max(int(fin.sum()), 1)
        res["book_over_off"] = {f: res["book"][f]["median"] / res["off"][f]["median"] for f in FIGURES}
    finally:
        for E in engines.values():
            E.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
