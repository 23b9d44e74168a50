#!/usr/bin/env python3
"""The policy temperature of the search's priors (azx_set_policy_temp; opt-in, NOT the reference's behaviour) measured at
the headline configuration on one GPU.  Recorded, not gated: no test asserts a speed, no threshold is set in advance.
These are RATES and search shapes, not strength (tools/strength_policy_temp.py plays the games).

  4096 games, 11x11, golden G8's weights (the reference's trained 6x64 network), 400 simulations in batches of 10,
  exploration_depth 15, the default pipelined loop, every game from the empty board.

  "policy_temp": (6, 8) and (4, 8) against the option off, side by side in ONE process: after `--warmup` play_steps (past
  the first games' common start), `--repeats` runs of `--steps` play_steps each, alternating; medians and spread
  (max - min) / median of plies/s, evaluated rows per ply, mean select depth (sum_depth / selects) and the mean entropy,
  in nats, of the STORED priors of the pool's roots after each run -- depth is expected to fall and root width to rise --
  and the option's statistics.

  "bench_py_option_never_set" (with --parent-lib NAME, a build of the parent commit's library put beside this build's as
  azalea_amd/NAME): bench.py with the option never set, this build and the parent's alternating (tools/lib_bench.py),
  `--repeats` runs of `--steps` moves each; the medians, the min-max spreads and the criterion -- each median inside the
  other's min-max range, and `evals` the same in every run.

    python tools/bench_policy_temp.py [--steps 40] [--repeats 3] [--warmup 100] [--parent-lib libazx_parent.so] [--only-bench-py] [--order m4,m6,off]
One JSON line; profiles/policy_temp_bench.json holds it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import bench_fpu as bf

SETTINGS = {"off": (8, 8), "m6": (6, 8), "m4": (4, 8)}
FIGURES = ("plies_per_sec", "evals_per_ply", "mean_depth", "root_prior_entropy")


def root_entropy(E):
    r = E.get_root()
    ent = []
    for g in range(E.G):
        k = int(r["k"][g])
        p = r["child_prior"][g, :k].astype(np.float64)
        if k and p.sum() > 0:
            p = p[p > 0]
            ent.append(float(-(p * np.log(p)).sum()))
    return float(np.mean(ent)) if ent else 0.0


def one_run(E, steps, on):
    before = E.policy_temp_stats()
    st = E.play_steps(steps)
    ps = {k: v - before[k] for k, v in E.policy_temp_stats().items()}
    plies = st["plies"]
    assert st["selects"] == bf.BATCH * (bf.SIMS // bf.BATCH + 1) * plies, (st["selects"], plies)
    assert (ps["tempered"] > 0) == on, ps
    return {"plies_per_sec": plies / st["seconds"], "evals_per_ply": st["evals"] / plies,
            "mean_depth": st["sum_depth"] / st["selects"], "root_prior_entropy": root_entropy(E), "plies": plies,
            "games": st["games"], "seconds": st["seconds"], "evals": st["evals"], "policy_temp_stats": ps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only-bench-py", action="store_true")
    ap.add_argument("--order", default="off,m6,m4", help="the order the engines are created, warmed up and run in")
    args = ap.parse_args()
    out = {}
    if not args.only_bench_py:
        state = bf.golden_state("g8_checkpoint.npz")
        res = {"board": bf.BOARD, "games": bf.GAMES, "batch": bf.BATCH, "simulations": bf.SIMS, "blocks": bf.BLOCKS,
               "chans": bf.CHANS, "exploration_depth": bf.DEPTH, "weights": "golden G8",
               "device": torch.cuda.get_device_name(0), "settings": {k: list(v) for k, v in SETTINGS.items()},
               "steps": args.steps, "repeats": args.repeats, "warmup": args.warmup, "order": args.order}
        order = args.order.split(",")
        assert sorted(order) == sorted(SETTINGS), order
        engines = {name: bf.headline_engine(state) for name in order}
        runs = {name: [] for name in engines}
        try:
            for name, E in engines.items():
                if SETTINGS[name] != (8, 8):
                    E.set_policy_temp(*SETTINGS[name])
                E.play_steps(args.warmup)     # past the first games' common start: games end and restart out of phase
            for _ in range(args.repeats):
                for name, E in engines.items():
                    r = one_run(E, args.steps, name != "off")
                    runs[name].append(r)
                    print("%s: %r" % (name, r), file=sys.stderr, flush=True)
            for name, E in engines.items():
                o = {"kernel_info": E.kernel_info(), "runs": runs[name]}
                for f in FIGURES:
                    xs = [r[f] for r in runs[name]]
                    o[f] = {"median": statistics.median(xs), "spread": bf.spread(xs)}
                res[name] = o
        finally:
            for E in engines.values():
                E.close()
        for name in ("m6", "m4"):
            res[name + "_over_off"] = {f: res[name][f]["median"] / res["off"][f]["median"] for f in FIGURES}
        out["policy_temp"] = res
    if args.parent_lib:
        out["bench_py_option_never_set"] = bf.never_set(args.parent_lib, args.steps, args.repeats, option="the policy temperature")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
