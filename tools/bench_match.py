#!/usr/bin/env python3
"""Evaluation matches measured: the tournament with the host in the per-ply loop (`evaluate_batched`) against the
same tournament played on the device (`evaluate_throughput`: engine.Match, azx_match_*), in ONE process on one GPU.
Random-weight 6x64 networks on 11x11, 400 simulations, move sampling on, exploration noise off (the agents of
tools/bench_evaluation.py).

  (a) evaluate_batched, two agents, 300 rounds (300 games resident)      } three times each, alternating,
  (b) evaluate_throughput, the same two agents, 300 rounds in 300 slots  } medians reported (wall time, set-up included)
  (c) evaluate_throughput, two agents, 16 384 rounds in 4 096 slots
  (d) for scale: self-play of one of the networks at 4 096 slots (Engine.play_steps from a pool started out of phase)
  (e) the three-agent round robin at 100 rounds both ways (evaluate_batched holds all 300 games at once, the device
      path plays its three pairs of 100 one after the other)

    python tools/bench_match.py [--sims 400] [--rounds 300] [--big-rounds 16384] [--big-slots 4096] [--rr-rounds 100]
One JSON line (profiles/match_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from azalea_amd import engine as eng
from azalea_amd import evaluation
from azalea_amd.azalea_agent import AzaleaAgent
from azalea_amd.game.hex import HexGame
from azalea_amd.policy import Policy

BOARD = 11


def agents(sims):
    out = []
    for seed in (1, 2, 3):
        torch.manual_seed(seed)
        p = Policy()
        p.initialize(dict(device="cuda:0", network="HexNetwork", board_size=BOARD, num_blocks=6, base_chans=64,
                          simulations=sims, search_batch_size=10, exploration_coef=0.5, exploration_depth=15,
                          exploration_noise_alpha=0.03, exploration_noise_scale=0.25, exploration_temperature=1.0))
        p.settings["move_sampling"] = True
        p.settings["move_exploration"] = False
        out.append(AzaleaAgent(lambda: HexGame(BOARD), policy=p, device="cuda:0"))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def tallies(out):
    return {"%d-%d" % p: list(map(int, v)) for p, v in out.items()}


def selfplay(pol, slots, sims, steps):
    """Throughput-mode self-play of one agent's network: the pool starts from seeded random positions of 0..92 plies
    (bench.py's desync, so finished games are spread over the moves), two untimed moves, then `steps` timed ones."""
    E = eng.Engine(board_size=BOARD, n_games=slots, simulations=sims, search_batch_size=10, exploration_coef=0.5,
                   exploration_depth=15, noise_alpha=0.03, noise_scale=0.0, temperature=1.0,
                   evaluator=eng.EVAL_RESNET, num_blocks=6, base_chans=64)
    sd = {k: v for k, v in pol.net.state_dict().items() if v.dtype == torch.float32}
    E.set_weights({k: (v.contiguous().data_ptr(), v.numel()) for k, v in sd.items()}, on_device=True)
    E.reset(moves=eng.random_prefixes(BOARD, np.arange(slots, dtype=np.int64), 92, 1))
    E.play_steps(2)
    st = E.play_steps(steps)
    info = E.kernel_info()
    E.close()
    return dict(slots=slots, steps=steps, seconds=st["seconds"], games=st["games"], plies=st["plies"],
                games_per_sec=st["games"] / st["seconds"], plies_per_sec=st["plies"] / st["seconds"],
                mean_game_length=st["sum_game_length"] / max(1, st["games"]), kernel_info=info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--big-rounds", type=int, default=16384)
    ap.add_argument("--big-slots", type=int, default=4096)
    ap.add_argument("--selfplay-steps", type=int, default=30)
    ap.add_argument("--rr-rounds", type=int, default=100)
    args = ap.parse_args()
    ag = agents(args.sims)
    two = ag[:2]
    res = {"board": BOARD, "net": "6x64 random-init", "sims": args.sims, "move_sampling": True, "exploration_noise": False,
           "device": torch.cuda.get_device_name(0)}

    # warm both paths once (allocator, kernel load) on a handful of games
    evaluation.evaluate_batched(two, 4)
    evaluation.evaluate_throughput(two, 4)

    # (a) / (b): one pair, the same number of games resident either way
    ta, tb = [], []
    for _ in range(args.repeats):
        t, out_a = timed(lambda: evaluation.evaluate_batched(two, args.rounds))
        ta.append(t)
        t, out_b = timed(lambda: evaluation.evaluate_throughput(two, args.rounds, n_slots=args.rounds))
        tb.append(t)
    res["pair"] = {
        "games": args.rounds, "slots": args.rounds, "repeats": args.repeats,
        "batched_seconds": ta, "throughput_seconds": tb,
        "batched_games_per_sec": args.rounds / statistics.median(ta),
        "throughput_games_per_sec": args.rounds / statistics.median(tb),
        "batched_tallies": tallies(out_a), "throughput_tallies": tallies(out_b)}

    # (c) a long match
    games = {}
    t, out_c = timed(lambda: evaluation.evaluate_throughput(two, args.big_rounds, n_slots=args.big_slots, games=games))
    length = games[(0, 1)]["length"]
    res["long_match"] = {"games": args.big_rounds, "slots": args.big_slots, "seconds": t,
                         "games_per_sec": args.big_rounds / t, "plies_per_sec": float(length.sum()) / t,
                         "mean_game_length": float(length.mean()), "tallies": tallies(out_c)}
    # (d) self-play of agent 0's network, for scale
    res["selfplay"] = selfplay(two[0].policy, args.big_slots, args.sims, args.selfplay_steps)
    res["long_match_over_selfplay_plies_per_sec"] = res["long_match"]["plies_per_sec"] / res["selfplay"]["plies_per_sec"]

    # (e) the three-agent round robin
    t_rb, out_rb = timed(lambda: evaluation.evaluate_batched(ag, args.rr_rounds))
    t_rt, out_rt = timed(lambda: evaluation.evaluate_throughput(ag, args.rr_rounds, n_slots=args.rr_rounds))
    n_rr = 3 * args.rr_rounds
    res["round_robin"] = {"agents": 3, "rounds": args.rr_rounds, "games": n_rr,
                          "batched_seconds": t_rb, "batched_games_per_sec": n_rr / t_rb,
                          "throughput_seconds": t_rt, "throughput_games_per_sec": n_rr / t_rt,
                          "batched_tallies": tallies(out_rb), "throughput_tallies": tallies(out_rt)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
