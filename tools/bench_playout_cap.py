#!/usr/bin/env python3
"""Playout cap randomisation (azx_set_playout_cap; opt-in, NOT the reference's behaviour) measured against plain
self-play at the headline configuration, in ONE process on one GPU.  Recorded, not gated: no test asserts a speed, and
nothing here says anything about playing strength or training efficiency -- neither is measured.

  4096 games, 11x11, golden G3's 6x64 weights, bench.py's 400 simulations in batches of 10, the default pipelined
  loop, the pool started out of phase; cap off against cap (0.25, simulations / 4); after a warm-up `--repeats` runs of
  `--steps` play_steps each, alternating, medians and spread (max - min) / median of
      plies per second, recorded rows (full plies) per second, rows harvested with finished games per second,
      evaluated rows per ply and net_seconds per ply.
  One figure is derivable and both sides are printed: the selections a run made must equal, exactly,
      batch * (nb_full * full plies + nb_fast * fast plies)
  with the plies counted by azx_playout_cap_stats (per ply: batch * (p_obs * nb_full + (1 - p_obs) * nb_fast)).

    python tools/bench_playout_cap.py [--steps 10] [--repeats 3] [--warmup 4]
One JSON line (profiles/playout_cap_bench.json)."""
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
BLOCKS, CHANS, SIMS, DESYNC = 6, 64, 400, 92
FULL_PROB, FAST_SIMS = 0.25, SIMS // 4
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIGURES = ("plies_per_sec", "recorded_rows_per_sec", "harvested_rows_per_sec", "evals_per_ply", "net_seconds_per_ply")


def golden_state(name):
    z = np.load(os.path.join(GOLDEN, name))
    assert [int(x) for x in z["cfg"]] == [11, 6, 64]
    return {k[2:]: z[k] for k in z.files if k.startswith("w:")}


def headline_engine(state, cap, warmup):
    """bench.py's headline engine with the pool started out of phase (random prefixes of 0..DESYNC plies)."""
    E = eng.Engine(board_size=BOARD, n_games=GAMES, simulations=SIMS, search_batch_size=BATCH, exploration_coef=0.5,
                   exploration_depth=15, noise_alpha=0.03, noise_scale=0.25, temperature=1.0,
                   evaluator=eng.EVAL_RESNET, num_blocks=BLOCKS, base_chans=CHANS)
    E.set_weights(state)
    E.reset(moves=eng.random_prefixes(BOARD, np.arange(GAMES, dtype=np.int64), DESYNC, 1))
    if cap:
        E.set_playout_cap(FULL_PROB, FAST_SIMS)
    E.play_steps(warmup)
    return E


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs) if statistics.median(xs) else 0.0


def one_run(E, steps, capped):
    nb_full, nb_fast = SIMS // BATCH + 1, FAST_SIMS // BATCH + 1
    before = E.playout_cap_stats()
    st = E.play_steps(steps)
    after = E.playout_cap_stats()
    full = after["full_plies"] - before["full_plies"] if capped else st["plies"]
    fast = after["fast_plies"] - before["fast_plies"] if capped else 0
    derived = BATCH * (nb_full * full + nb_fast * fast)
    out = {"plies_per_sec": st["plies"] / st["seconds"], "recorded_rows_per_sec": full / st["seconds"],
           "harvested_rows_per_sec": st["positions"] / st["seconds"], "evals_per_ply": st["evals"] / st["plies"],
           "net_seconds_per_ply": st["net_seconds"] / st["plies"],
           "plies": st["plies"], "full_plies": full, "fast_plies": fast, "p_obs": full / max(1, full + fast),
           "selects": st["selects"], "selects_derived": derived,
           "selects_per_ply": st["selects"] / st["plies"], "selects_per_ply_derived": derived / max(1, full + fast),
           "selects_equal": st["selects"] == derived and st["plies"] == full + fast}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=4)
    args = ap.parse_args()
    state = golden_state("g3_forward_11_6x64.npz")
    engines = {"off": headline_engine(state, False, args.warmup), "cap": headline_engine(state, True, args.warmup)}
    res = {"board": BOARD, "games": GAMES, "batch": BATCH, "sims": SIMS, "blocks": BLOCKS, "chans": CHANS,
           "cap": {"full_prob": FULL_PROB, "fast_simulations": FAST_SIMS},
           "nb_full": SIMS // BATCH + 1, "nb_fast": FAST_SIMS // BATCH + 1,
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "repeats": args.repeats, "warmup": args.warmup,
           "strength_and_training_efficiency": "NOT measured"}
    runs = {name: [] for name in engines}
    try:
        for _ in range(args.repeats):
            for name, E in engines.items():
                r = one_run(E, args.steps, name == "cap")
                runs[name].append(r)
                print("%s: selects %d, batch * (nb_full * full + nb_fast * fast) = %d (%s); per ply %.4f vs %.4f at "
                      "p_obs %.4f; %.1f plies/s" % (name, r["selects"], r["selects_derived"],
                                                    "equal" if r["selects_equal"] else "NOT EQUAL", r["selects_per_ply"],
                                                    r["selects_per_ply_derived"], r["p_obs"], r["plies_per_sec"]),
                      file=sys.stderr, flush=True)
        for name, E in engines.items():
            out = {"kernel_info": E.kernel_info(), "runs": runs[name],
                   "selects_equal": all(r["selects_equal"] for r in runs[name])}
            for f in FIGURES:
                xs = [r[f] for r in runs[name]]
                out[f] = {"median": statistics.median(xs), "spread": spread(xs)}
            res[name] = out
        res["cap_over_off"] = {f: res["cap"][f]["median"] / res["off"][f]["median"] for f in FIGURES
                               if res["off"][f]["median"]}
    finally:
        for E in engines.values():
            E.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
