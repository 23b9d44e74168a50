#!/usr/bin/env python3
"""First-play urgency of the PUCT search (azx_set_fpu; opt-in, NOT the reference's behaviour) measured at the headline
configuration on one GPU.  Recorded, not gated: no test asserts a speed, no threshold is set in advance.  These are
RATES and search shapes, not strength (tools/strength_fpu.py plays the games).

  4096 games, 11x11, golden G8's weights (the reference's trained 6x64 network), 400 simulations in batches of 10,
  exploration_depth 15, the default pipelined loop, every game from the empty board.

  "fpu": REDUCTION (0.25 below the root, 0 at it) against the option off, side by side in ONE process: after `--warmup`
  play_steps (past the first games' common start), `--repeats` runs of `--steps` play_steps each, alternating; medians
  and spread (max - min) / median of plies/s, evaluated rows per ply and mean select depth (sum_depth / selects) -- the
  two quantities the option is expected to move -- and the option's statistics.

  "bench_py_option_never_set" (with --parent-lib NAME, a build of the parent commit's library put beside this build's as
  azalea_amd/NAME): bench.py with the option never set, this build and the parent's alternating (tools/lib_bench.py),
  `--repeats` runs of `--steps` moves each; the medians, the min-max spreads and the criterion, both ways it has been
  stated -- each median inside the other's min-max range; the medians no further apart than the larger spread -- and
  whether `evals` is the same in every run.

    python tools/bench_fpu.py [--steps 40] [--repeats 3] [--warmup 100] [--parent-lib libazx_parent.so]
One JSON line; profiles/fpu_bench.json holds it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from azalea_amd import engine as eng

BOARD, GAMES, BATCH, SIMS = 11, 4096, 10, 400
BLOCKS, CHANS, DEPTH = 6, 64, 15
REDUCTION = ("reduction", 0.0, 0.25, 0.0)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIGURES = ("plies_per_sec", "evals_per_ply", "mean_depth")


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
    before = E.fpu_stats()
    st = E.play_steps(steps)
    fs = {k: v - before[k] for k, v in E.fpu_stats().items()}
    plies = st["plies"]
    assert st["selects"] == BATCH * (SIMS // BATCH + 1) * plies, (st["selects"], plies)
    assert fs["selects"] == (st["selects"] if on else 0), (fs, st["selects"])
    return {"plies_per_sec": plies / st["seconds"], "evals_per_ply": st["evals"] / plies,
            "mean_depth": st["sum_depth"] / st["selects"], "plies": plies, "games": st["games"], "seconds": st["seconds"],
            "evals": st["evals"], "fpu_stats": fs}


def bench_py(lib, steps):
    cmd = [sys.executable]
    cmd += [os.path.join(ROOT, "tools", "lib_bench.py"), lib] if lib else [os.path.join(ROOT, "bench.py")]
    cmd += ["--gpus", "1", "--steps", str(steps), "--warmup", "5", "--no-config5"]
    out = subprocess.run(["timeout", "-k", "10", "600"] + cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                         check=True).stdout.decode()
    line = json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
    keep = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "evals", "plies_per_sec", "games_per_sec")
    return {k: line[k] for k in keep if k in line}


def never_set(parent_lib, steps, repeats, option="first-play urgency"):
    runs = {"this": [], "parent": []}
    for _ in range(repeats):
        for name, lib in (("this", None), ("parent", parent_lib)):
            runs[name].append(bench_py(lib, steps))
            print("bench.py %s: %r" % (name, runs[name][-1]), file=sys.stderr, flush=True)
    out = {"command": "python bench.py --gpus 1 --steps %d --warmup 5 --no-config5, %s never set; this build "
                      "and the parent commit's library (tools/lib_bench.py) alternating in one session, this build first"
                      % (steps, option), "order": ", ".join(["this, parent"] * repeats)}
    for name, rs in runs.items():
        vs = [r["value"] for r in rs]
        out[name] = {"runs": rs, "median": statistics.median(vs), "min": min(vs), "max": max(vs),
                     "spread_min_max": max(vs) - min(vs)}
    widest = max(out["this"]["spread_min_max"], out["parent"]["spread_min_max"])
    apart = abs(out["this"]["median"] - out["parent"]["median"])
    inside = (out["parent"]["min"] <= out["this"]["median"] <= out["parent"]["max"] and
              out["this"]["min"] <= out["parent"]["median"] <= out["this"]["max"])
    evals = {r["evals"] for rs in runs.values() for r in rs}
    out["criterion"] = {"medians_apart": apart, "larger_spread": widest,
                        "each_median_inside_the_others_min_max": bool(inside),
                        "medians_no_further_apart_than_the_larger_spread": bool(apart <= widest),
                        "evals_identical": len(evals) == 1, "evals": sorted(evals)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    state = golden_state("g8_checkpoint.npz")
    res = {"board": BOARD, "games": GAMES, "batch": BATCH, "simulations": SIMS, "blocks": BLOCKS, "chans": CHANS,
           "exploration_depth": DEPTH, "weights": "golden G8", "device": torch.cuda.get_device_name(0),
           "fpu": {"mode": REDUCTION[0], "reduction": REDUCTION[2], "root_reduction": REDUCTION[3]},
           "steps": args.steps, "repeats": args.repeats, "warmup": args.warmup}
    engines = {"off": headline_engine(state), "reduction": headline_engine(state)}
    runs = {name: [] for name in engines}
    try:
        engines["reduction"].set_fpu(*REDUCTION)
        for E in engines.values():
            E.play_steps(args.warmup)         # past the first games' common start: games end and restart out of phase
        for _ in range(args.repeats):
            for name, E in engines.items():
                r = one_run(E, args.steps, name == "reduction")
                runs[name].append(r)
                print("%s: %r" % (name, r), file=sys.stderr, flush=True)
        for name, E in engines.items():
            out = {"kernel_info": E.kernel_info(), "runs": runs[name]}
            for f in FIGURES:
                xs = [r[f] for r in runs[name]]
                out[f] = {"median": statistics.median(xs), "spread": spread(xs)}
            res[name] = out
    finally:
        for E in engines.values():
            E.close()
    res["reduction_over_off"] = {f: res["reduction"][f]["median"] / res["off"][f]["median"] for f in FIGURES}
    out = {"fpu": res}
    if args.parent_lib:
        out["bench_py_option_never_set"] = never_set(args.parent_lib, args.steps, args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
