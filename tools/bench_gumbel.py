#!/usr/bin/env python3
"""The Gumbel root search with sequential halving of device self-play (azx_set_gumbel; opt-in, NOT the reference's
behaviour) measured at the headline configuration, in ONE process on one GPU.  Recorded, not gated: no test asserts a
speed, no threshold is set in advance.  These are RATES, not strength: nothing here says anything about playing strength
or training efficiency -- neither is measured.

  4096 games, 11x11, golden G8's weights (the reference's trained 6x64 network), batches of 10, exploration_depth 15,
  the default pipelined loop, every game from the empty board.

  Four configurations: off at 400 simulations, m = 16 at 400, m = 16 at 64, off at 64.  The two of one simulation count
  run side by side: after `--warmup` play_steps (past the first games' common start), `--repeats` runs of `--steps`
  play_steps each, alternating; medians and spread (max - min) / median of plies/s, recorded rows/s and evaluated rows
  per ply.  Then one play() of `--rows` rows gives the mean entropy (nats) of the recorded rows, and one more -- with the
  rows switched to visit shares (set_train_targets("visits"); under the option improved_rows=False), which leaves the
  games as they are -- the share of plies whose played move is not the (first) most-visited child.

    python tools/bench_gumbel.py [--steps 40] [--repeats 3] [--warmup 100] [--rows 20000]
One JSON line.  profiles/gumbel_bench.json holds it under "gumbel"; under "bench_py_option_never_set" the same file holds
bench.py's runs with the option never set, this build and the parent commit's library alternating (tools/lib_bench.py),
with the medians, the min-max spreads and the criterion."""
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
BLOCKS, CHANS, DEPTH = 6, 64, 15
M, C_VISIT, C_SCALE = 16, 50.0, 1.0
SIMS = (400, 64)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIGURES = ("plies_per_sec", "recorded_rows_per_sec", "evals_per_ply")


def golden_state(name):
    z = np.load(os.path.join(GOLDEN, name))
    assert [int(x) for x in z["cfg"]] == [11, 6, 64]
    return {k[2:]: z[k] for k in z.files if k.startswith("w:")}


def headline_engine(state, sims):
    E = eng.Engine(board_size=BOARD, n_games=GAMES, simulations=sims, search_batch_size=BATCH, exploration_coef=0.5,
                   exploration_depth=DEPTH, noise_alpha=0.03, noise_scale=0.25, temperature=1.0,
                   evaluator=eng.EVAL_RESNET, num_blocks=BLOCKS, base_chans=CHANS)
    E.set_weights(state)
    return E


def spread(xs):
    return (max(xs) - min(xs)) / statistics.median(xs) if statistics.median(xs) else 0.0


def one_run(E, steps, sims, on):
    before = E.gumbel_stats()
    st = E.play_steps(steps)
    gs = {k: v - before[k] for k, v in E.gumbel_stats().items()}
    plies = st["plies"]
    assert st["selects"] == BATCH * (sims // BATCH + 1) * plies, (st["selects"], plies)
    assert gs == (dict(plies=plies, halvings=gs["halvings"], root_selects=st["selects"], improved_rows=plies) if on
                  else dict.fromkeys(gs, 0)), (gs, plies)
    return {"plies_per_sec": plies / st["seconds"], "recorded_rows_per_sec": st["positions"] / st["seconds"],
            "evals_per_ply": st["evals"] / plies, "halvings_per_ply": gs["halvings"] / max(plies, 1), "plies": plies,
            "games": st["games"], "seconds": st["seconds"]}


def entropy_of(p):
    p = p.astype(np.float64)
    return -(np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)).sum(1)


def row_entropy(E, rows):
    """Mean entropy (nats) of the rows of one play(): over all rows, and over the rows of plies before exploration_depth."""
    got, _ = E.play(rows)
    h = entropy_of(got["moves_prob"])
    early = (got["board"].reshape(len(h), -1) != 0).sum(1) < DEPTH
    return {"rows": int(len(h)), "mean_entropy": float(h.mean()), "early_rows": int(early.sum()),
            "mean_entropy_early_rows": float(h[early].mean()), "mean_entropy_later_rows": float(h[~early].mean())}


def off_leader_share(E, rows):
    """Share of plies (of games harvested whole, rows = visit shares) whose played move is not the first most-visited
    child: the move is the one stone the game's next row adds."""
    got, _ = E.play(rows)
    uid, board, prob = got["game_uid"], got["board"].reshape(len(got["game_uid"]), -1), got["moves_prob"]
    same = np.flatnonzero(uid[1:] == uid[:-1])
    off = n = 0
    for r in same:
        new = np.flatnonzero(board[r + 1] != board[r])
        if len(new) != 1:
            continue
        child = int((board[r][:new[0]] == 0).sum())             # the rank of the new stone's cell among the empty cells
        n += 1
        off += int(np.argmax(prob[r]) != child)
    return {"plies": n, "share_not_most_visited": off / max(n, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rows", type=int, default=20000)
    args = ap.parse_args()
    state = golden_state("g8_checkpoint.npz")
    res = {"board": BOARD, "games": GAMES, "batch": BATCH, "blocks": BLOCKS, "chans": CHANS, "exploration_depth": DEPTH,
           "weights": "golden G8", "device": torch.cuda.get_device_name(0), "m": M, "c_visit": C_VISIT,
           "c_scale": C_SCALE, "steps": args.steps, "repeats": args.repeats, "warmup": args.warmup,
           "strength_and_training_efficiency": "NOT measured"}
    for sims in SIMS:
        engines = {"off": headline_engine(state, sims), "gumbel": headline_engine(state, sims)}
        runs = {name: [] for name in engines}
        try:
            engines["gumbel"].set_gumbel(M, C_VISIT, C_SCALE, improved_rows=True)
            for E in engines.values():
                E.play_steps(args.warmup)     # past the first games' common start: games end and restart out of phase
            for _ in range(args.repeats):
                for name, E in engines.items():
                    r = one_run(E, args.steps, sims, name == "gumbel")
                    runs[name].append(r)
                    print("%d %s: %r" % (sims, name, r), file=sys.stderr, flush=True)
            for name, E in engines.items():
                out = {"kernel_info": E.kernel_info(), "runs": runs[name]}
                for f in FIGURES:
                    xs = [r[f] for r in runs[name]]
                    out[f] = {"median": statistics.median(xs), "spread": spread(xs)}
                out["row_entropy_nats"] = row_entropy(E, args.rows)
                E.set_train_targets("visits")
                if name == "gumbel":
                    E.set_gumbel(M, C_VISIT, C_SCALE, improved_rows=False)
                E.play_steps(BOARD * BOARD)                     # every game in flight now began after the switch ...
                E.play(args.rows)                               # ... and the rows recorded before it are handed over
                out["played_move"] = off_leader_share(E, args.rows)
                res["%s_%d" % (name, sims)] = out
        finally:
            for E in engines.values():
                E.close()
    for a, b in (("gumbel_400", "off_400"), ("gumbel_64", "off_64"), ("gumbel_64", "off_400"), ("gumbel_64", "gumbel_400")):
        res["%s_over_%s" % (a, b)] = {f: res[a][f]["median"] / res[b][f]["median"] for f in FIGURES}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
