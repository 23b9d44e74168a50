#!/usr/bin/env python3
"""Early stop of device self-play (azx_set_early_stop; opt-in, NOT the reference's behaviour) measured at the headline
configuration, in ONE process on one GPU.  Recorded, not gated: no test asserts a speed, there is no speed-up target,
and nothing here says anything about playing strength or training efficiency -- neither is measured.

  4096 games, 11x11, golden G8's weights (the reference's trained 6x64 network: a random network's searches stop far
  less often), 400 simulations in batches of 10 (41 select batches), exploration_depth 15, the default pipelined loop,
  every game from the empty board.

  Option off against on: after `--warmup` play_steps (the warm-up of tools/bench_resign.py: past the first games'
  common start), `--repeats` runs of `--steps` play_steps each, alternating; medians and spread (max - min) / median of
  plies/s, finished games/s, recorded rows/s, evaluated rows per ply and net_seconds per ply; from azx_early_stop_stats
  the share of T = 0 plies stopped and the mean batches a T = 0 ply used.  In every run the selects per ply must equal
  bs * (41 * plies - batches skipped) / plies exactly (asserted).  A CPU estimate on the oracle (four games read off
  full searches, so counterfactual) gave about 0.67 of the 41 batches on T = 0 plies: the result carries both.

    python tools/bench_early_stop.py [--steps 40] [--repeats 3] [--warmup 100]
One JSON line.  profiles/early_stop_bench.json holds it under "early_stop"; under "bench_py_option_never_set" the same
file holds bench.py's runs with the option never set, this build and the parent commit's library alternating
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
CPU_ESTIMATE_T0_BATCH_SHARE = 0.67
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIGURES = ("plies_per_sec", "games_per_sec", "recorded_rows_per_sec", "evals_per_ply", "net_seconds_per_ply",
           "selects_per_ply")


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
    before = E.early_stop_stats()
    st = E.play_steps(steps)
    es = {k: v - before[k] for k, v in E.early_stop_stats().items()}
    plies = st["plies"]
    # the derivable figure, exactly: every ply runs 41 batches of 10 selects less the batches its stop skipped
    assert st["selects"] == BATCH * (NB * plies - es["batches_skipped"]), (st["selects"], plies, es)
    assert on or es == dict.fromkeys(es, 0)
    r = {"plies_per_sec": plies / st["seconds"], "games_per_sec": st["games"] / st["seconds"],
         "recorded_rows_per_sec": st["positions"] / st["seconds"], "evals_per_ply": st["evals"] / plies,
         "net_seconds_per_ply": st["net_seconds"] / plies, "selects_per_ply": st["selects"] / plies,
         "plies": plies, "games": st["games"], "seconds": st["seconds"]}
    if on:
        t0 = max(es["t0_plies"], 1)
        r.update(t0_plies=es["t0_plies"], t0_share_of_plies=es["t0_plies"] / plies,
                 share_of_t0_plies_stopped=es["stopped_plies"] / t0,
                 mean_batches_per_t0_ply=NB - es["batches_skipped"] / t0,
                 t0_batch_share=(NB - es["batches_skipped"] / t0) / NB)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=100)
    args = ap.parse_args()
    state = golden_state("g8_checkpoint.npz")
    res = {"board": BOARD, "games": GAMES, "batch": BATCH, "sims": SIMS, "blocks": BLOCKS, "chans": CHANS,
           "exploration_depth": DEPTH, "weights": "golden G8", "device": torch.cuda.get_device_name(0),
           "steps": args.steps, "repeats": args.repeats, "warmup": args.warmup,
           "cpu_estimate_t0_batch_share": CPU_ESTIMATE_T0_BATCH_SHARE,
           "strength_and_training_efficiency": "NOT measured"}
    engines = {"off": headline_engine(state), "on": headline_engine(state)}
    runs = {name: [] for name in engines}
    try:
        engines["on"].set_early_stop(True)
        for E in engines.values():
            E.play_steps(args.warmup)         # past the first games' common start: games end and restart out of phase
        for _ in range(args.repeats):
            for name, E in engines.items():
                r = one_run(E, args.steps, name == "on")
                runs[name].append(r)
                print("%s: %r" % (name, r), file=sys.stderr, flush=True)
        for name, E in engines.items():
            out = {"kernel_info": E.kernel_info(), "runs": runs[name]}
            figures = FIGURES + (("share_of_t0_plies_stopped", "mean_batches_per_t0_ply", "t0_batch_share",
                                  "t0_share_of_plies") if name == "on" else ())
            for f in figures:
                xs = [r[f] for r in runs[name]]
                out[f] = {"median": statistics.median(xs), "spread": spread(xs)}
            res[name] = out
        res["on_over_off"] = {f: res["on"][f]["median"] / res["off"][f]["median"]
                              for f in FIGURES if res["off"][f]["median"]}
        res["selects_per_ply_identity"] = "held exactly in every run"
    finally:
        for E in engines.values():
            E.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
