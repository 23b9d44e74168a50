#!/usr/bin/env python3
"""Measurements of the rollout evaluator (azx_set_rollout_evaluator; NOT the reference's behaviour), for the record in
profiles/rollout_bench.json.  Nothing here is asserted.

    python3 tools/bench_rollout.py --selfplay [--out FILE]
        rollout against rollout at the headline shape (11x11, 4096 slots, 400 simulations, batch 10, 64 rollouts):
        plies/s and the share of the time in hand-overs (play_steps' net_seconds), medians of three runs
    python3 tools/bench_rollout.py --anchor [--games 400] [--out FILE]
        the reference's shipped 11x11 6x64 model (the golden fixture tests/golden/g8_checkpoint.npz) against
        RolloutNet(64), both at 400 simulations, through evaluate_throughput; the tally with its 95 % Wilson interval
    python3 tools/bench_rollout.py --strength [--out FILE]
        the strength sanity match of tests/test_gpu_rollout.py (7x7, RolloutNet(32) against AZX_EVAL_UNIFORM)
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/bench_rollout.py --kernel-run
    python3 tools/bench_rollout.py --kernel-summary DIR [--out FILE]
        the kernel alone on 40 960 mid-game 11x11 rows at R = 16 / 64 / 256: --kernel-run is the program to trace (one
        warm-up and three launches per R, in that order), --kernel-summary reads the trace: ms per launch (median of the
        three) and rollouts/s, beside the tower's 7.55 ms per headline launch (README)

Every mode merges its entry into --out (default profiles/rollout_bench.json)."""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

KERNEL_ROWS, KERNEL_R, KERNEL_REPS = 40960, (16, 64, 256), 3
TOWER_MS = 7.55          # README: the 6x64 tower's launch at the headline pool


def merge(path, key, value):
    doc = {}
    if os.path.exists(path):
        doc = json.load(open(path))
    doc[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({key: value}))


def midgame_rows(n_rows, N=11, seed=1):
    """Random 11x11 positions with 40 to 80 stones, dealt alternately (the mover is colour 1)."""
    rng = np.random.RandomState(seed)
    cells = N * N
    boards = np.zeros((n_rows, cells), np.int32)
    for i in range(n_rows):
        stones = int(rng.randint(40, 81)) & ~1
        order = rng.permutation(cells)[:stones]
        boards[i, order[0::2]] = 1
        boards[i, order[1::2]] = 2
    return boards


def kernel_run():
    from azalea_amd import engine
    boards = midgame_rows(KERNEL_ROWS)
    for R in KERNEL_R:
        for _ in range(1 + KERNEL_REPS):
            wins, _, _ = engine.selftest_rollout(boards, R, seed=R)
        print("R=%d mean mover win share %.4f" % (R, wins.mean() / R))


def kernel_summary(trace_dir, out):
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if "k_rollout" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    if len(rows) != len(KERNEL_R) * (1 + KERNEL_REPS):
        raise SystemExit("expected %d k_rollout launches in the trace, found %d" % (len(KERNEL_R) * (1 + KERNEL_REPS), len(rows)))
    ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows]
    res = {"what": "k_rollout alone on %d mid-game 11x11 rows (40 to 80 stones), rocprofv3 kernel trace, median of %d "
                   "launches after one warm-up" % (KERNEL_ROWS, KERNEL_REPS),
           "tower_ms_per_headline_launch_README": TOWER_MS, "by_rollouts": {}}
    for i, R in enumerate(KERNEL_R):
        timed = ms[i * (1 + KERNEL_REPS) + 1:(i + 1) * (1 + KERNEL_REPS)]
        med = statistics.median(timed)
        res["by_rollouts"][str(R)] = {"ms_per_launch": round(med, 4), "ms_runs": [round(x, 4) for x in timed],
                                      "rollouts_per_second": round(KERNEL_ROWS * R / (med / 1e3)),
                                      "share_of_tower_launch": round(med / TOWER_MS, 4)}
    merge(out, "kernel_alone", res)


def selfplay(args):
    from azalea_amd import engine as eng
    E = eng.Engine(board_size=11, n_games=args.slots, simulations=args.sims, search_batch_size=10, exploration_coef=0.5,
                   exploration_depth=15, noise_alpha=0.03, noise_scale=0.25, temperature=1.0,
                   evaluator=eng.EVAL_EXTERNAL, seed=12345)
    E.set_rollout_evaluator(args.rollouts, 0)
    E.reset(moves=eng.random_prefixes(11, np.arange(args.slots), 60, 12345))
    E.play_steps(1)                             # warm-up
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        st = E.play_steps(args.plies)
        wall = time.perf_counter() - t0
        runs.append({"plies": st["plies"], "wall_seconds": round(wall, 4), "plies_per_second": round(st["plies"] / wall, 1),
                     "net_seconds": round(st["net_seconds"], 4), "mcts_seconds": round(st["mcts_seconds"], 4),
                     "handover_share_of_wall": round(st["net_seconds"] / wall, 4), "evals": st["evals"]})
    stats = E.rollout_stats()
    res = {"what": "rollout(%d) self-play, 11x11, %d slots, %d simulations, batch 10, %d moves per run; hand-overs are "
                   "play_steps' net_seconds (order + host sync + export + k_rollout + import)" %
                   (args.rollouts, args.slots, args.sims, args.plies),
           "engine": E.kernel_info(), "runs": runs,
           "median_plies_per_second": statistics.median(r["plies_per_second"] for r in runs),
           "median_handover_share_of_wall": statistics.median(r["handover_share_of_wall"] for r in runs),
           "rollout_stats": stats, "mover_win_share_of_rollouts": round(stats["rollouts_won"] / max(1, stats["rollouts"]), 4)}
    E.close()
    merge(args.out, "selfplay_headline_shape", res)


def wilson(k, n, z=1.96):
    if n == 0:
        return [0.0, 1.0]
    p = k / n
    d = 1 + z * z / n
    c = p + z * z / (2 * n)
    h = z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n))
    return [round((c - h) / d, 4), round((c + h) / d, 4)]


def anchor(args):
    import torch
    from azalea_amd import evaluation
    from azalea_amd.azalea_agent import AzaleaAgent
    from azalea_amd.game.hex import HexGame
    from azalea_amd.policy import Policy
    from azalea_amd.rollout import RolloutNet
    z = np.load(os.path.join(ROOT, "tests", "golden", "g8_checkpoint.npz"))
    board, blocks, chans = (int(x) for x in z["cfg"])
    cfg = dict(board_size=board, simulations=args.sims, search_batch_size=10, exploration_coef=0.5, exploration_depth=6,
               exploration_noise_alpha=0.03, exploration_noise_scale=0.25, exploration_temperature=1.0, seed=1)
    net = Policy()
    net.initialize(dict(cfg, device="cuda:0", network="HexNetwork", num_blocks=blocks, base_chans=chans))
    net.net.load_state_dict({k[2:]: torch.as_tensor(z[k]) for k in z.files if k.startswith("w:")})
    net.net.to("cuda:0")
    roll = Policy()
    roll.initialize(dict(cfg, device="cpu", network="azalea_amd.rollout.RolloutNet", num_blocks=0, base_chans=0))
    roll.net = RolloutNet(args.rollouts, seed=0)
    agents = []
    for p in (net, roll):
        p.settings["move_sampling"] = True          # temperature 1 for the first 6 plies, no root noise
        p.settings["move_exploration"] = False
        agents.append(AzaleaAgent(lambda n=board: HexGame(n), policy=p, device="cuda:0"))
    info, games = {}, {}
    t0 = time.perf_counter()
    out = evaluation.evaluate_throughput(agents, args.games, seed=7, info=info, games=games)
    wall = time.perf_counter() - t0
    w_net, _, w_roll = (int(x) for x in out[(0, 1)])
    g = games[(0, 1)]
    distinct = len({tuple(r[:n]) for r, n in zip(g["moves"].tolist(), g["length"].tolist())})
    res = {"what": "golden G8 weights (%dx%d on %dx%d) against RolloutNet(%d), both at %d simulations, temperature 1 for "
                   "the first 6 plies, no noise, %d games through evaluate_throughput, colours shared evenly" %
                   (blocks, chans, board, board, args.rollouts, args.sims, args.games),
           "tally_network_rollout": [w_net, w_roll], "network_win_share": round(w_net / max(1, w_net + w_roll), 4),
           "network_win_share_wilson95": wilson(w_net, w_net + w_roll), "distinct_games": distinct,
           "mean_length": round(float(g["length"].mean()), 2), "wall_seconds": round(wall, 2), "rollout_engine": info[1]}
    merge(args.out, "anchor_g8_vs_rollout", res)


def strength(args):
    from azalea_amd import engine as eng
    kw = dict(board_size=7, n_games=64, simulations=200, search_batch_size=10, exploration_coef=0.5, exploration_depth=4,
              noise_alpha=0.03, noise_scale=0.0, temperature=1.0)
    A = eng.Engine(evaluator=eng.EVAL_EXTERNAL, seed=1 << 32, **kw)
    B = eng.Engine(evaluator=eng.EVAL_UNIFORM, seed=2 << 32, **kw)
    A.set_rollout_evaluator(32, 0)
    m = eng.Match(A, B)
    res = m.play(64, moves=True)
    st = res["stats"]
    distinct = len({tuple(r[:n]) for r, n in zip(res["moves"].tolist(), res["length"].tolist())})
    merge(args.out, "strength_sanity_7x7", {
        "what": "tests/test_gpu_rollout.py's match: rollout(32) against AZX_EVAL_UNIFORM, 7x7, 200 simulations a side, "
                "temperature 1 for the first 4 plies, no noise, 64 games, colours shared evenly; the bar is 44 wins",
        "wins_rollout_uniform": list(st["wins"]), "first_player_wins": st["first_player_wins"],
        "distinct_games": distinct, "seconds": round(st["seconds"], 3)})
    m.close()
    A.close()
    B.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kernel-summary", default=None, metavar="DIR")
    ap.add_argument("--selfplay", action="store_true")
    ap.add_argument("--anchor", action="store_true")
    ap.add_argument("--strength", action="store_true")
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--rollouts", type=int, default=64)
    ap.add_argument("--plies", type=int, default=3, help="--selfplay: moves per slot and run")
    ap.add_argument("--games", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_bench.json"))
    args = ap.parse_args()
    if args.kernel_run:
        kernel_run()
    if args.kernel_summary:
        kernel_summary(args.kernel_summary, args.out)
    if args.strength:
        strength(args)
    if args.selfplay:
        selfplay(args)
    if args.anchor:
        anchor(args)


if __name__ == "__main__":
    main()
