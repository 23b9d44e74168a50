#!/usr/bin/env python3
"""What the policy temperature of the search's priors (Engine.set_policy_temp; opt-in, NOT the reference's behaviour)
does to PLAY, by tools/strength_fpu.py's protocol: the same weights with (eighths, root_eighths) against the same weights
with the option off, on the device (evaluation.evaluate_throughput), every game from one of engine.all_openings(n) --
both colours of each opening -- so that the games differ.  Recorded, not gated: no test asserts a strength.

  Weights: the checkpoint AZX_REF_CHECKPOINT names (a Policy checkpoint), else the reference's trained 11x11 6x64 model as
  the golden fixture tests/golden/g8_checkpoint.npz holds it, at 400 simulations.

    python tools/strength_policy_temp.py [--games 400] [--sims 400] [--eighths 6] [--root-eighths 8]
One JSON line: the tally, the score of the option-on side with its 95 % interval (normal approximation of a binomial
share; a Hex game has no draw) and the verdict in the words profiles/policy_temp_strength.json keeps."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import strength_fpu as sf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=400)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--eighths", type=int, default=6)
    ap.add_argument("--root-eighths", type=int, default=8)
    ap.add_argument("--checkpoint", default=os.environ.get("AZX_REF_CHECKPOINT"))
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    from azalea_amd import engine as eng
    from azalea_amd import evaluation
    from azalea_amd.azalea_agent import AzaleaAgent
    from azalea_amd.game.hex import HexGame

    policies = []
    for side in range(2):
        p, weights = (sf.checkpoint_policy(args.checkpoint, args.sims) if args.checkpoint
                      else sf.golden_policy(args.sims, args.seed))
        p.settings["move_sampling"] = True                  # temperature-1 draws for the policy's first exploration_depth
        p.settings["move_exploration"] = False              # plies, no root noise: as the other strength tools play
        p.net.eval()
        policies.append(p)
    policies[0].set_policy_temp((args.eighths, args.root_eighths))
    assert policies[0].policy_temp is not None and policies[1].policy_temp is None
    n = policies[0].board_size
    agents = [AzaleaAgent(lambda n=n: HexGame(n), policy=p, device="cuda:0") for p in policies]
    openings = eng.all_openings(n)
    games, info = {}, {}
    out = evaluation.evaluate_throughput(agents, args.games + (args.games & 1), seed=args.seed, openings=openings,
                                         games=games, info=info)
    w_on, _, w_off = (int(x) for x in out[(0, 1)])
    total = w_on + w_off
    score = w_on / total
    half = 1.96 * math.sqrt(score * (1.0 - score) / total)
    lo, hi = score - half, score + half
    verdict = ("no difference shown at this sample" if lo <= 0.5 <= hi else
               "the option-on side scores BELOW 0.5 at this sample" if hi < 0.5 else
               "the option-on side scores above 0.5 at this sample")
    length = games[(0, 1)]["length"]
    print(json.dumps({
        "what": "policy temperature (%d, %d) eighths -- temperature %.3g for the expanded rows, %.3g at the root -- against "
                "the option off, the same weights on both sides"
                % (args.eighths, args.root_eighths, 8.0 / args.eighths, 8.0 / args.root_eighths),
        "weights": weights, "board": n, "simulations": args.sims, "games": total, "openings": len(openings),
        "schedule": "every opening both ways round (evaluate_throughput(openings=all_openings(n))), moves drawn at "
                    "temperature 1 for the first %d plies and greedily after, no root noise" % policies[0].exploration_depth,
        "wins_option_on": w_on, "wins_option_off": w_off, "score_option_on": score, "interval_95": [lo, hi],
        "verdict": verdict, "default": "off (whatever this says)",
        "mean_game_length": float(np.mean(length)), "engines": {str(k): v for k, v in info.items()},
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
