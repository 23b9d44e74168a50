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
One JSON line (profiles/match_bench.json).

`--external`: the match with a custom network instead -- a torch.nn.Module that is not a HexNetwork and whose `run` is
the PyTorch forward of a 6x64 HexNetwork -- and nothing of the above:
  (i)   evaluate_throughput(external_batch=True): the custom network against a 6x64 HexNetwork on the device tower,
        `--ext-games` games in `--ext-slots` slots
  (ii)  the same two agents through evaluation.evaluate, the host loop, `--host-games` games (once: it is slow)
  (iii) two custom agents under AZX_MATCH_INTERLEAVE=1 and =0 (read at azx_match_create)
  (iv)  self-play of the custom network at the same slot count, in plies/s: the EVAL_EXTERNAL engine with
        policy.external_evaluator registered that Player(external_batch=True) plays with, driven by play_steps from a
        pool started out of phase as (d) above
(i), (iii) and (iv) `--repeats` times, alternating, medians of the wall time with the set-up included.

    python tools/bench_match.py --external [--ext-games 256] [--ext-slots 256] [--host-games 2] [--repeats 3]
One JSON line (profiles/match_external_bench.json).  `--external --trace-run`: two matches of the two custom agents and
nothing else, for `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_match.py ...`.

`--tournament`: the round robin as ONE device-resident tournament (evaluate_throughput(pooled=True): engine.Tournament,
azx_tournament_*) against the pairs played one after the other (pooled=False), and nothing of the above:
  (f) three agents, `--rr-rounds` rounds: 100 slots per engine for the pairs loop, 200 (100 tables per pair) pooled
  (g) `--tour-agents` agents, `--tour-rounds` rounds (8 and 20: 28 pairs, 560 games; 20 slots per engine for the pairs
      loop, 140 -- 20 tables per pair -- pooled)
each `--repeats` times, alternating, medians of the wall time with the set-up included, and the spread (max - min) /
median of either.  The tallies of the two schedules are the same games, and are checked to be.

    python tools/bench_match.py --tournament [--rr-rounds 100] [--tour-agents 8] [--tour-rounds 20] [--repeats 3]
One JSON line (profiles/tournament_bench.json).  `--tournament --trace-run`: two pooled runs of (g) and nothing else,
for the profiler as above.

`--collect`: what harvesting the games' replay rows on the device costs, and what it buys (nothing of the above):
  (h) one engine.Match of two 6x64 agents, `--big-rounds` games in `--big-slots` slots, `--repeats` times alternately
      without and with collect="device" (the rows stay in engine a's harvest queue), medians of the device time of the
      call (azx_match_stats.seconds) and of the wall time, and the spread (max - min) / median of either
  (j) Player(None, [a, b], device_match=True, n_games=S).read for S in `--player-slots`, with `--chunks` games per
      Match.play call in units of S: rows/s and games/s over `--player-reads` reads of one chunk's worth of rows
  (k) the same two agents through the host loop (Player without device_match: play_game, one game at a time),
      `--host-games` games
`--collect --trace-run`: one harvesting (or, with `--no-harvest`, plain) match of (h)'s shape and nothing else, for the
profiler as above.

    python tools/bench_match.py --collect [--big-rounds 16384] [--big-slots 4096] [--repeats 3]
                                          [--player-slots 256,4096] [--chunks 1,2,4] [--host-games 2]
One JSON line (profiles/match_rows_bench.json).

`--openings N`: the match from an opening book against the same match from the empty board (nothing of the above):
  (l) one engine.Match of two 6x64 agents, `--big-rounds` games in `--big-slots` slots, `--repeats` times alternately
      without a book and from the first N of engine.all_openings(11, 1) (game u from opening (u >> 1) % N), medians of
      the device time of the call and of the wall time, the spread of either, and plies per second (a game from an
      opening is a move shorter, so games per second alone would flatter the book)

    python tools/bench_match.py --openings 121 [--big-rounds 16384] [--big-slots 4096] [--repeats 3]
One JSON line (profiles/match_openings_bench.json, when measured)."""
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


def agents(sims, count=3):
    out = []
    for seed in range(1, count + 1):
        torch.manual_seed(seed)
        p = Policy()
        p.initialize(dict(device="cuda:0", network="HexNetwork", board_size=BOARD, num_blocks=6, base_chans=64,
                          simulations=sims, search_batch_size=10, exploration_coef=0.5, exploration_depth=15,
                          exploration_noise_alpha=0.03, exploration_noise_scale=0.25, exploration_temperature=1.0))
        p.settings["move_sampling"] = True
        p.settings["move_exploration"] = False
        out.append(AzaleaAgent(lambda: HexGame(BOARD), policy=p, device="cuda:0"))
    return out


class CustomNet(torch.nn.Module):
    """Not a HexNetwork: evaluates with the PyTorch forward of one, behind the reference's duck-typed contract."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    @property
    def device(self):               # (the reference's Network has it; Policy's host loop sends its batches there)
        return self.inner.device

    def run(self, batch):
        return self.inner.run(batch)


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


def selfplay_external(pol, slots, sims, steps):
    """selfplay() for a custom network: the engine Player(external_batch=True) plays with."""
    from azalea_amd.policy import external_evaluator
    E = eng.Engine(board_size=BOARD, n_games=slots, simulations=sims, search_batch_size=10, exploration_coef=0.5,
                   exploration_depth=15, noise_alpha=0.03, noise_scale=0.0, temperature=1.0, evaluator=eng.EVAL_EXTERNAL)
    pol.net.eval()
    E.set_external_evaluator(external_evaluator(pol.net))
    E.reset(moves=eng.random_prefixes(BOARD, np.arange(slots, dtype=np.int64), 92, 1))
    E.play_steps(1)
    st = E.play_steps(steps)
    E.close()
    return dict(seconds=st["seconds"], plies=st["plies"], plies_per_sec=st["plies"] / st["seconds"])


def external_main(args):
    ag = agents(args.sims)
    for a in (ag[0], ag[2]):
        a.policy.net = CustomNet(a.policy.net)
    custom, tower, custom2 = ag
    res = {"board": BOARD, "net": "6x64 random-init", "sims": args.sims, "move_sampling": True, "exploration_noise": False,
           "device": torch.cuda.get_device_name(0), "games": args.ext_games, "slots": args.ext_slots,
           "repeats": args.repeats}
    G, S = args.ext_games, args.ext_slots

    def match(field, interleave):
        os.environ["AZX_MATCH_INTERLEAVE"] = str(interleave)
        games = {}
        t, out = timed(lambda: evaluation.evaluate_throughput(field, G, n_slots=S, games=games, external_batch=True))
        print("match of %d games, interleave %s: %.2f s, %d plies" % (G, interleave, t, games[(0, 1)]["length"].sum()),
              file=sys.stderr, flush=True)
        return t, float(games[(0, 1)]["length"].sum()), out

    if args.trace_run:      # the program to put behind `rocprofv3 --kernel-trace --stats --`: two matches of two custom agents
        match([custom, custom2], 1)
        t, plies, _ = match([custom, custom2], 1)
        print(json.dumps({"games": G, "slots": S, "seconds": t, "plies": plies}))
        return
    # warm every path once: the convolution library prepares its kernels per batch size
    t_warm, _, _ = match([custom, tower], 1)
    res["warm_up_match_seconds"] = t_warm
    match([custom, custom2], 1)
    selfplay_external(custom.policy, S, args.sims, 1)

    t_i, t_on, t_off, sp = [], [], [], []
    plies_i = plies_on = plies_off = 0.0
    for _ in range(args.repeats):
        t, plies_i, out_i = match([custom, tower], 1)
        t_i.append(t)
        t, plies_on, _ = match([custom, custom2], 1)
        t_on.append(t)
        t, plies_off, _ = match([custom, custom2], 0)
        t_off.append(t)
        sp.append(selfplay_external(custom.policy, S, args.sims, args.selfplay_steps))
        print("self-play: %s" % sp[-1], file=sys.stderr, flush=True)
    os.environ.pop("AZX_MATCH_INTERLEAVE", None)
    med = statistics.median
    res["custom_vs_tower"] = {"seconds": t_i, "games_per_sec": G / med(t_i), "plies_per_sec": plies_i / med(t_i),
                              "tallies": tallies(out_i)}
    # (ii) the parent's path for the same two agents
    t_h, out_h = timed(lambda: evaluation.evaluate([custom, tower], args.host_games))
    print("host loop, %d games: %.2f s" % (args.host_games, t_h), file=sys.stderr, flush=True)
    res["host_loop"] = {"games": args.host_games, "seconds": t_h, "games_per_sec": args.host_games / t_h,
                        "tallies": tallies(out_h)}
    res["throughput_over_host_loop_games_per_sec"] = res["custom_vs_tower"]["games_per_sec"] / res["host_loop"]["games_per_sec"]
    res["custom_vs_custom"] = {"interleaved_seconds": t_on, "plain_seconds": t_off,
                               "interleaved_plies_per_sec": plies_on / med(t_on),
                               "plain_plies_per_sec": plies_off / med(t_off),
                               "plain_over_interleaved_seconds": med(t_off) / med(t_on),
                               "spread_interleaved": (max(t_on) - min(t_on)) / med(t_on),
                               "spread_plain": (max(t_off) - min(t_off)) / med(t_off)}
    res["selfplay_external"] = {"steps": args.selfplay_steps, "plies_per_sec": [x["plies_per_sec"] for x in sp],
                                "median_plies_per_sec": med([x["plies_per_sec"] for x in sp])}
    res["match_over_selfplay_plies_per_sec"] = (res["custom_vs_tower"]["plies_per_sec"] /
                                                res["selfplay_external"]["median_plies_per_sec"])
    print(json.dumps(res))


def tournament_main(args):
    K, R = args.tour_agents, args.tour_rounds
    ag = agents(args.sims, max(3, K))
    res = {"board": BOARD, "net": "6x64 random-init", "sims": args.sims, "move_sampling": True, "exploration_noise": False,
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats}

    def run(field, rounds, pooled):
        k = len(field)
        n_slots = (k - 1) * rounds if pooled else rounds
        t, out = timed(lambda: evaluation.evaluate_throughput(field, rounds, n_slots=n_slots, pooled=pooled))
        print("%d agents, %d rounds, %s: %.2f s" % (k, rounds, "pooled" if pooled else "pairs", t), file=sys.stderr, flush=True)
        return t, tallies(out)

    if args.trace_run:      # the program to put behind `rocprofv3 --kernel-trace --stats --`
        run(ag[:K], R, True)
        t, _ = run(ag[:K], R, True)
        print(json.dumps({"agents": K, "rounds": R, "games": K * (K - 1) // 2 * R, "seconds": t}))
        return
    # warm both paths once (allocator, kernel load) on a handful of games
    run(ag[:3], 4, False)
    run(ag[:3], 4, True)

    def leg(field, rounds):
        k = len(field)
        n = k * (k - 1) // 2 * rounds
        t_pairs, t_pooled = [], []
        for _ in range(args.repeats):
            t, out_pairs = run(field, rounds, False)
            t_pairs.append(t)
            t, out_pooled = run(field, rounds, True)
            t_pooled.append(t)
            assert out_pooled == out_pairs, "the pooled schedule played other games"
        med = statistics.median
        return {"agents": k, "rounds": rounds, "games": n, "slots_per_engine_pairs": rounds,
                "slots_per_engine_pooled": (k - 1) * rounds, "tables_per_pair": rounds,
                "pairs_seconds": t_pairs, "pooled_seconds": t_pooled,
                "pairs_games_per_sec": n / med(t_pairs), "pooled_games_per_sec": n / med(t_pooled),
                "spread_pairs": (max(t_pairs) - min(t_pairs)) / med(t_pairs),
                "spread_pooled": (max(t_pooled) - min(t_pooled)) / med(t_pooled),
                "pairs_over_pooled_seconds": med(t_pairs) / med(t_pooled), "tallies": out_pooled}

    res["round_robin_3"] = leg(ag[:3], args.rr_rounds)        # (f)
    res["ladder"] = leg(ag[:K], R)                            # (g)
    print(json.dumps(res))


def match_engines(ag, slots):
    """One engine per agent, as evaluation.evaluate_throughput builds them (move sampling on, noise off)."""
    out = []
    for k, a in enumerate(ag):
        pol = a.policy
        E = eng.Engine(board_size=BOARD, n_games=slots, simulations=pol.simulations, search_batch_size=pol.search_batch_size,
                       exploration_coef=pol.exploration_coef, exploration_depth=pol.exploration_depth,
                       noise_alpha=pol.exploration_noise_alpha, noise_scale=0.0, temperature=pol.exploration_temperature,
                       evaluator=eng.EVAL_RESNET, num_blocks=pol.num_blocks, base_chans=pol.base_chans, seed=k << 32)
        pol.net.eval()
        sd = {n: v for n, v in pol.net.state_dict().items() if v.dtype == torch.float32}
        E.set_weights({n: (v.contiguous().data_ptr(), v.numel()) for n, v in sd.items()}, on_device=True)
        out.append(E)
    return out


def collect_main(args):
    from azalea_amd.parallel_player import Player
    two = agents(args.sims, 2)
    med = statistics.median
    spread = lambda xs: (max(xs) - min(xs)) / med(xs)
    res = {"board": BOARD, "net": "6x64 random-init", "sims": args.sims, "move_sampling": True, "exploration_noise": False,
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats}
    G, S = args.big_rounds, args.big_slots
    if G > 0:
        a, b = match_engines(two, S)
        m = eng.Match(a, b)

        def run(collect):
            t, out = timed(lambda: m.play(G, collect=collect))
            print("match of %d games in %d slots, collect=%s: wall %.2f s, device %.2f s, %d rows" % (
                G, S, collect, t, out["stats"]["seconds"], out.get("n_rows", 0)), file=sys.stderr, flush=True)
            return t, out

        if args.trace_run:
            t, out = run(False if args.no_harvest else "device")
            print(json.dumps({"games": G, "slots": S, "harvest": not args.no_harvest, "seconds": t,
                              "device_seconds": out["stats"]["seconds"], "rows": out.get("n_rows", 0)}))
            return
        m.play(min(G, 2 * S) if args.warm_games < 0 else args.warm_games, collect="device")   # warm: allocator, queue, kernel load
        wall = {False: [], "device": []}
        dev = {False: [], "device": []}
        rows = plies = 0
        for _ in range(args.repeats):
            for collect in (False, "device"):
                t, out = run(collect)
                wall[collect].append(t)
                dev[collect].append(out["stats"]["seconds"])
                plies = out["stats"]["plies"]
                rows = out.get("n_rows", rows)
        res["harvest_cost"] = {
            "games": G, "slots": S, "rows": rows, "plies": plies,
            "off_device_seconds": dev[False], "on_device_seconds": dev["device"],
            "off_wall_seconds": wall[False], "on_wall_seconds": wall["device"],
            "off_games_per_sec": G / med(dev[False]), "on_games_per_sec": G / med(dev["device"]),
            "on_rows_per_sec": rows / med(dev["device"]),
            "on_over_off_device_seconds": med(dev["device"]) / med(dev[False]),
            "on_over_off_wall_seconds": med(wall["device"]) / med(wall[False]),
            "spread_off": spread(dev[False]), "spread_on": spread(dev["device"])}
        m.close()
        a.close()
        b.close()
    # (j) the two-agent Player on the device
    res["player"] = []
    for slots in [int(x) for x in args.player_slots.split(",") if x]:
        for chunk in [int(x) for x in args.chunks.split(",") if x]:
            Player.MATCH_CHUNK = chunk
            pl = Player(None, two, device_match=True, n_games=slots, gather=False)
            pl.read(1)                                       # the first chunk: engines, queue, kernel load
            while pl._games:
                pl._games.popleft()
            secs, nrows, ngames = [], 0, 0
            for _ in range(args.player_reads):
                t, (frame, metrics) = timed(lambda: pl.read(1))
                n_q = sum(len(r["reward"]) for r, _ in pl._games)
                g_q = len(pl._games)
                pl._games.clear()                            # the whole chunk counts: what one production yields
                secs.append(t)
                nrows += len(frame) + n_q
                ngames += int(metrics["games"]) + g_q
            pl.stop()
            res["player"].append({"slots": slots, "chunk_games": chunk * slots, "reads": args.player_reads,
                                  "seconds": secs, "rows": nrows, "games": ngames,
                                  "rows_per_sec": nrows / sum(secs), "games_per_sec": ngames / sum(secs)})
            print("player: %s" % res["player"][-1], file=sys.stderr, flush=True)
    # (k) the host loop for the same two agents
    if args.host_games > 0:
        pl = Player(None, two, n_games=1, gather=False)

        def host_games():
            for _ in range(args.host_games):
                pl._produce(1)
        t, _ = timed(host_games)
        rows = sum(len(r["reward"]) for r, _ in pl._games)
        res["host_loop"] = {"games": len(pl._games), "rows": rows, "seconds": t, "games_per_sec": len(pl._games) / t,
                            "rows_per_sec": rows / t}
        pl.stop()
        print("host loop: %s" % res["host_loop"], file=sys.stderr, flush=True)
        for r in res["player"]:
            r["over_host_loop_rows_per_sec"] = r["rows_per_sec"] / res["host_loop"]["rows_per_sec"]
    print(json.dumps(res))


def openings_main(args):
    two = agents(args.sims, 2)
    med = statistics.median
    spread = lambda xs: (max(xs) - min(xs)) / med(xs)
    G, S = args.big_rounds, args.big_slots
    book = eng.all_openings(BOARD, 1)[:args.openings]
    res = {"board": BOARD, "net": "6x64 random-init", "sims": args.sims, "move_sampling": True, "exploration_noise": False,
           "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "games": G, "slots": S,
           "openings": len(book), "opening_plies": 1}
    a, b = match_engines(two, S)
    m = eng.Match(a, b)
    m.play(min(G, 2 * S), openings=book)                     # warm: allocator, kernel load
    keys = ("empty_board", "book")
    wall = {k: [] for k in keys}
    dev = {k: [] for k in keys}
    plies = {k: 0 for k in keys}
    for _ in range(args.repeats):
        for k in keys:
            t, out = timed(lambda: m.play(G, openings=book if k == "book" else None))
            print("match of %d games in %d slots, %s: wall %.2f s, device %.2f s, %d plies" % (
                G, S, k, t, out["stats"]["seconds"], out["stats"]["plies"]), file=sys.stderr, flush=True)
            wall[k].append(t)
            dev[k].append(out["stats"]["seconds"])
            plies[k] = out["stats"]["plies"]
    for k in keys:
        res[k] = {"device_seconds": dev[k], "wall_seconds": wall[k], "plies": plies[k],
                  "games_per_sec": G / med(dev[k]), "plies_per_sec": plies[k] / med(dev[k]), "spread": spread(dev[k])}
    res["book_over_empty_board_plies_per_sec"] = res["book"]["plies_per_sec"] / res["empty_board"]["plies_per_sec"]
    m.close()
    a.close()
    b.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--openings", type=int, default=0, metavar="N",
                    help="the match from the first N one-move openings against the match from the empty board")
    ap.add_argument("--collect", action="store_true")
    ap.add_argument("--no-harvest", action="store_true", help="--collect --trace-run: the same match without harvesting")
    ap.add_argument("--warm-games", type=int, default=-1)
    ap.add_argument("--player-slots", default="256,4096")
    ap.add_argument("--chunks", default="1,2,4")
    ap.add_argument("--player-reads", type=int, default=1)
    ap.add_argument("--external", action="store_true")
    ap.add_argument("--ext-games", type=int, default=256)
    ap.add_argument("--ext-slots", type=int, default=256)
    ap.add_argument("--host-games", type=int, default=2)
    ap.add_argument("--trace-run", action="store_true", help="--external: only two custom-vs-custom matches (for a profiler)")
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--big-rounds", type=int, default=16384)
    ap.add_argument("--big-slots", type=int, default=4096)
    ap.add_argument("--selfplay-steps", type=int, default=30)
    ap.add_argument("--rr-rounds", type=int, default=100)
    ap.add_argument("--tournament", action="store_true")
    ap.add_argument("--tour-agents", type=int, default=8)
    ap.add_argument("--tour-rounds", type=int, default=20)
    args = ap.parse_args()
    if args.openings > 0:
        return openings_main(args)
    if args.collect:
        return collect_main(args)
    if args.external:
        return external_main(args)
    if args.tournament:
        return tournament_main(args)
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
