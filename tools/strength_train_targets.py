#!/usr/bin/env python3
"""Playing strength under config["train_targets"] (azx_set_train_targets; NOT the reference's behaviour), taken once on
a small board: for each seed, tools/train_to_strength.py's training run (the reference's loop with everything on the
device) three times from the same seed and step count -- targets off, "visits", and ("visits", 0.5) -- and then each
network trained with the option against the OFF network of its seed in a device match
(evaluation.evaluate_throughput): `--games` games from the one-move opening book, every opening with the colours
both ways, temperature-1 sampling for the first exploration_depth plies, no root noise.

    python tools/strength_train_targets.py [--board 7] [--seeds 3 4] [--games 400] [--epochs 6]

One JSON line: per seed and setting the tally [wins of off, 0, wins of the option's network], the option's win rate and
its 95 % Wilson interval; the same pooled over the seeds.  There is no pass threshold: an interval that contains 0.5 is
reported as "no difference shown".  profiles/train_targets_strength.json holds the line."""
import argparse
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import train_to_strength as tts

SETTINGS = (("off", None), ("visits", "visits"), ("visits_mix_0.5", "visits:0.5"))


def wilson(wins, n, z=1.959964):
    if n == 0:
        return [0.0, 1.0]
    p = wins / n
    d = 1 + z * z / n
    c = p + z * z / (2 * n)
    h = z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n))
    return [(c - h) / d, (c + h) / d]


def verdict(wins, n):
    lo, hi = wilson(wins, n)
    return {"games": n, "wins": wins, "win_rate": wins / max(n, 1), "wilson95": [lo, hi],
            "verdict": "no difference shown" if lo <= 0.5 <= hi else ("stronger" if lo > 0.5 else "weaker")}


def train_one(args, seed, targets):
    from azalea_amd.policy_trainer import train
    a = argparse.Namespace(**vars(args))
    a.seed, a.train_targets = seed, targets
    policy = tts.make_policy(a, seed)
    t0 = time.perf_counter()
    train(policy, tts.train_config(a), tempfile.mkdtemp(prefix="azx_tt_strength_"), device_replay=True)
    torch.cuda.synchronize()
    return policy, time.perf_counter() - t0


def match(off, other, board, games, seed):
    from azalea_amd import engine, evaluation
    from azalea_amd.azalea_agent import AzaleaAgent
    from azalea_amd.game.hex import HexGame
    agents = []
    for p in (off, other):
        p.settings["move_sampling"] = True
        p.settings["move_exploration"] = False
        p.net.eval()
        agents.append(AzaleaAgent(lambda n=board: HexGame(n), policy=p, device="cuda:0"))
    out = evaluation.evaluate_throughput(agents, games, seed=seed, openings=engine.all_openings(board, 1))
    return [int(x) for x in out[(0, 1)]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=7)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--chans", type=int, default=32)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--c", type=float, default=1.0)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--alpha", type=float, default=0.3)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--replay", type=int, default=60000)
    ap.add_argument("--oversampling", type=float, default=4.0)
    ap.add_argument("--games-per-pool", dest="games", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--lr-decay", type=float, default=0.1)
    ap.add_argument("--lr-decay-epochs", type=int, default=0)
    ap.add_argument("--log-interval", type=int, default=5000)
    ap.add_argument("--mover-view", action="store_true")
    ap.add_argument("--seeds", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--match-games", type=int, default=400)
    args = ap.parse_args()
    steps = args.epochs * (args.replay // 128 + (1 if args.replay % 128 else 0))
    res = {"net": "%dx%d on %dx%d" % (args.blocks, args.chans, args.board, args.board), "sims": args.sims,
           "exploration_depth": args.depth, "epochs": args.epochs, "steps": steps, "seeds": args.seeds,
           "match": "%d games against the off network of the same seed, one-move opening book, colours both ways, "
                    "temperature-1 sampling for the first %d plies, no root noise" % (args.match_games, args.depth),
           "tally": "[wins of the off network, 0, wins of the option's network]", "by_seed": {}, "pooled": {}}
    pooled = {name: [0, 0] for name, _ in SETTINGS[1:]}
    for seed in args.seeds:
        nets, secs = {}, {}
        for name, targets in SETTINGS:
            nets[name], secs[name] = train_one(args, seed, targets)
            print("seed %d %s: trained in %.1f s" % (seed, name, secs[name]), file=sys.stderr, flush=True)
        entry = {"train_seconds": secs}
        for name, _ in SETTINGS[1:]:
            tally = match(nets["off"], nets[name], args.board, args.match_games, seed)
            entry[name] = dict(tally=tally, **verdict(tally[2], tally[0] + tally[2]))
            pooled[name][0] += tally[2]
            pooled[name][1] += tally[0] + tally[2]
            print("seed %d %s vs off: %r" % (seed, name, entry[name]), file=sys.stderr, flush=True)
        res["by_seed"][str(seed)] = entry
    for name, (w, n) in pooled.items():
        res["pooled"][name] = verdict(w, n)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
