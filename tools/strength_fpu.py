#!/usr/bin/env python3
"""What first-play urgency (Engine.set_fpu; opt-in, NOT the reference's behaviour) does to PLAY: the same weights with
REDUCTION (0.25 below the root, 0 at it) against the same weights with the option off, on the device
(evaluation.evaluate_throughput), every game from one of engine.all_openings(n) -- both colours of each opening -- so
that the games differ.  Recorded, not gated: no test asserts a strength.

  Weights: the checkpoint AZX_REF_CHECKPOINT names (a Policy checkpoint), else the reference's trained 11x11 6x64 model as
  the golden fixture tests/golden/g8_checkpoint.npz holds it, at 400 simulations.  (--board 7 plays a 7x7 network given
  with --checkpoint, e.g. one tools/train_to_strength.py trained.)

    python tools/strength_fpu.py [--games 400] [--sims 400] [--reduction 0.25] [--root-reduction 0.0]
One JSON line: the tally, the score of the option-on side with its 95 % interval (normal approximation of a binomial
share; a Hex game has no draw) and the verdict in the words profiles/fpu_strength.json keeps."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

DEPTH = 15                                  # the golden checkpoint's exploration_depth stand-in: the reference's default


def golden_policy(sims, seed):
    from azalea_amd.policy import Policy
    z = np.load(os.path.join(ROOT, "tests", "golden", "g8_checkpoint.npz"))
    n, blocks, chans = (int(x) for x in z["cfg"])
    p = Policy()
    p.initialize(dict(device="cuda:0", network="HexNetwork", board_size=n, num_blocks=blocks, base_chans=chans,
                      simulations=sims, search_batch_size=10, exploration_coef=0.5, exploration_depth=DEPTH,
                      exploration_noise_alpha=0.03, exploration_noise_scale=0.25, exploration_temperature=1.0, seed=seed))
    p.net.load_state_dict({k[2:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("w:")})
    p.net.to("cuda:0")
    return p, "golden G8 (the reference's trained 11x11 6x64 model)"


def checkpoint_policy(path, sims):
    from azalea_amd.policy import Policy
    p = Policy.load(path, device="cuda:0")
    p.simulations = sims
    return p, os.path.basename(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=400)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--reduction", type=float, default=0.25)
    ap.add_argument("--root-reduction", type=float, default=0.0)
    ap.add_argument("--checkpoint", default=os.environ.get("AZX_REF_CHECKPOINT"))
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    from azalea_amd import engine as eng
    from azalea_amd import evaluation
    from azalea_amd.azalea_agent import AzaleaAgent
    from azalea_amd.game.hex import HexGame

    policies = []
    for side in range(2):
        p, weights = (checkpoint_policy(args.checkpoint, args.sims) if args.checkpoint else golden_policy(args.sims, args.seed))
        p.settings["move_sampling"] = True                  # temperature-1 draws for the policy's first exploration_depth
        p.settings["move_exploration"] = False              # plies, no root noise: as the other strength tools play
        p.net.eval()
        policies.append(p)
    policies[0].set_fpu(("reduction", 0.0, args.reduction, args.root_reduction))
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
    verdict = ("no gain shown at this sample" if lo <= 0.5 <= hi else
               "the option-on side scores BELOW 0.5 at this sample" if hi < 0.5 else
               "the option-on side scores above 0.5 at this sample")
    length = games[(0, 1)]["length"]
    print(json.dumps({
        "what": "REDUCTION (%g below the root, %g at it) against the option off, the same weights on both sides"
                % (args.reduction, args.root_reduction),
        "weights": weights, "board": n, "simulations": args.sims, "games": total, "openings": len(openings),
        "schedule": "every opening both ways round (evaluate_throughput(openings=all_openings(n))), moves drawn at "
                    "temperature 1 for the first %d plies and greedily after, no root noise" % policies[0].exploration_depth,
        "wins_option_on": w_on, "wins_option_off": w_off, "score_option_on": score, "interval_95": [lo, hi],
        "verdict": verdict, "default": "off (whatever this says)",
        "mean_game_length": float(np.mean(length)), "engines": {str(k): v for k, v in info.items()},
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
