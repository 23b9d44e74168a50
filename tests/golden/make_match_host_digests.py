"""Writes tests/golden/match_host_digests.json: a SHA-256 per case over what small device matches and tournaments
return.  tests/test_gpu_match_host_digests.py reads the file, replays the same cases through `run_case` below and
compares; it never writes it.

Made ONCE, on the commit BEFORE the host code of azx_match_* and azx_tournament_* was folded into one ply loop
(DESIGN 7.19), with that commit's library and Python: the fixture is what says the shared loop enqueues what the two
hand-written loops did.  Needs a GPU.  Every case is run twice and nothing is written when the two runs differ.

    python tests/golden/make_match_host_digests.py [--out FILE]
    python tests/golden/make_match_host_digests.py --case NAME      (prints that case's digest and writes nothing)

A digest covers `outcome`, `length`, `moves` and `opening` where the play returns them, the integer fields of the stats
and, where the play collects, the harvested rows and their row metrics.  A game's rows are contiguous in the harvest
queue with plies ascending, and the digest checks that and keeps that order; whole games are taken by game_uid, since
the order in which games that end in the same ply reach the queue is not fixed: every finished game's wave reserves its
rows with one atomicAdd on the queue's row count (match_harvest in azalea_amd/csrc/match_kernels.hip, called from both
step kernels), and the waves of one launch get there in no set order.  A tournament's
digest is taken over its pairs' digests in pair order and then the rows; the one-pair tournament's is its pair's alone,
so that it can be held against the Match over the same games.

All cases run 20 simulations in batches of 5 on 8 slots (the 13x13 case 12: one game per slot) and play 12 to 16 games
with the uniform-hash evaluator, except `match_resnet`, whose agent 0 is a seeded 1x16 network on 5x5: that digest pins
the device numerics of the tower on the machine type the fixture was written on (an MI355X), not only the host code.
"""
import argparse
import functools
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
FIXTURE = os.path.join(HERE, "match_host_digests.json")

SLOTS = 8
SEEDS = (11, (1 << 40) + 5, (2 << 40) + 9)
# three different agents: exploration coefficient, depth and noise scale (agent 0 plays without noise)
AGENTS = (dict(exploration_coef=0.5, exploration_depth=6, noise_scale=0.0),
          dict(exploration_coef=1.5, exploration_depth=10, noise_scale=0.25),
          dict(exploration_coef=1.0, exploration_depth=4, noise_scale=0.25))
BOOK = ([13], [7, 19])       # tiles of every board from 5x5 up; no opening that short decides a game
ROW_KEYS = ("board", "color", "nlegal", "moves_prob", "reward", "game_uid")
STAT_KEYS = ("games", "first_player_wins", "voided", "plies")

# the case made in a child process under AZX_MATCH_INTERLEAVE=0 (read at azx_match_create) and the case it must equal
PLAIN_ORDER, PLAIN_ORDER_OF = "match_external_plain_order", "match_external"


def engine(eng, n, agent, kind="hash", slots=SLOTS):
    """Agent `agent` on an n x n board.  kind 'hash': the inline uniform-hash evaluator; 'ext': an EVAL_EXTERNAL engine
    with the same evaluator registered as a PyTorch stub; 'net': a seeded 1x16 network on the device tower."""
    cfg = dict(board_size=n, n_games=slots, simulations=20, search_batch_size=5, noise_alpha=0.3, temperature=1.0,
               seed=SEEDS[agent], **AGENTS[agent])
    if kind == "hash":
        return eng.Engine(evaluator=eng.EVAL_UNIFORM_HASH, **cfg)
    if kind == "ext":
        if TESTS not in sys.path:
            sys.path.insert(0, TESTS)
        from test_gpu_external_eval import uniform_hash_evaluator
        E = eng.Engine(evaluator=eng.EVAL_EXTERNAL, **cfg)
        E.set_external_evaluator(uniform_hash_evaluator(n * n))
        return E
    import torch
    from azalea_amd.network import HexNetwork
    torch.manual_seed(20261021 + agent)
    net = HexNetwork(board_size=n, num_blocks=1, base_chans=16).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.6, 1.4)
    E = eng.Engine(evaluator=eng.EVAL_RESNET, num_blocks=1, base_chans=16, **cfg)
    E.set_weights({k: v.detach().numpy() for k, v in net.state_dict().items() if v.dtype.is_floating_point})
    return E


def game_digest(res):
    """SHA-256 over one Match.play result, or one pair's dict of a Tournament.play result, without its rows."""
    h = hashlib.sha256()
    for k in ("outcome", "length", "moves", "opening"):
        if k in res:
            h.update(k.encode())
            h.update(np.ascontiguousarray(res[k]).tobytes())
    st = res["stats"]
    h.update(np.asarray([st[k] for k in STAT_KEYS] + list(st["wins"]), np.int64).tobytes())
    return h


def add_rows(h, out):
    """The harvested rows of a collecting play into `h`: whole games by game_uid, a game's rows in queue order."""
    rows, metrics = out["rows"], out["row_metrics"]
    uid = rows["game_uid"]
    assert len(uid) == out["n_rows"] == len(metrics)
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
    assert len(np.unique(uid[starts])) == len(starts), "a game's rows are not contiguous in the harvest queue"
    order = np.argsort(uid, kind="stable")
    for k in ROW_KEYS:
        h.update(np.ascontiguousarray(rows[k][order]).tobytes())
    h.update(np.ascontiguousarray(metrics[order]).tobytes())


def play_match(eng, n, kinds, n_games, slots=SLOTS, **kw):
    engines = [engine(eng, n, i, kind, slots) for i, kind in enumerate(kinds)]
    m = eng.Match(*engines)
    try:
        out = m.play(n_games, **kw)
    finally:
        m.close()
        for E in engines:
            E.close()
    h = game_digest(out)
    if kw.get("collect"):
        add_rows(h, out)
    return h.hexdigest()


def play_tournament(eng, n, kinds, pairs, rounds, **kw):
    engines = [engine(eng, n, i, kind) for i, kind in enumerate(kinds)]
    t = eng.Tournament(engines)
    try:
        out = t.play(pairs, rounds, **kw)
    finally:
        t.close()
        for E in engines:
            E.close()
    if len(pairs) == 1:
        return game_digest(out[tuple(pairs[0])]).hexdigest()
    h = hashlib.sha256()
    for p in pairs:
        h.update(game_digest(out[tuple(p)]).digest())
    if kw.get("collect"):
        add_rows(h, out)
    return h.hexdigest()


HASH2 = ("hash", "hash")
REFILL = dict(n_games=14, first_game=6, moves=True)          # also the games of the one-pair tournament
CASES = {
    # a plain play: none of the setters is called
    "match_5_plain": lambda eng: play_match(eng, 5, HASH2, 12),
    "match_9_collect_first_mover": lambda eng: play_match(eng, 9, HASH2, 12, moves=True, collect=True, first_mover=1),
    # one game per slot: no slot is refilled
    "match_13_book_no_refill": lambda eng: play_match(eng, 13, HASH2, 12, slots=12, moves=True, openings=BOOK),
    # more games than slots: finished slots are refilled
    "match_5_refill": lambda eng: play_match(eng, 5, HASH2, **REFILL),
    "match_external": lambda eng: play_match(eng, 5, ("ext", "hash"), 12, first_game=3, moves=True),
    "tournament_3_collect_book": lambda eng: play_tournament(
        eng, 7, ("hash",) * 3, [(0, 1), (0, 2), (1, 2)], 4, first_game=2, tables_per_pair=2, moves=True, collect=True,
        sink=1, openings=BOOK),
    "tournament_one_pair": lambda eng: play_tournament(
        eng, 5, HASH2, [(0, 1)], REFILL["n_games"], first_game=REFILL["first_game"], tables_per_pair=SLOTS, moves=True),
    "match_resnet": lambda eng: play_match(eng, 5, ("net", "hash"), 12, moves=True, collect=True),
}
SAME_GAMES = ("tournament_one_pair", "match_5_refill")       # equal digests: a pair plays its Match's games


def fresh_case(name):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from azalea_amd import engine as eng
    return CASES[name](eng)


run_case = functools.lru_cache(maxsize=None)(fresh_case)     # the tests share a case's digest


def child_digest(name, env):
    """`name` in a fresh process under the environment `env`."""
    import subprocess
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], env=env, check=True,
                         stdout=subprocess.PIPE, timeout=300).stdout.decode()
    return out.split()[-1]


def plain_order_digest():
    return child_digest(PLAIN_ORDER_OF, dict(os.environ, AZX_MATCH_INTERLEAVE="0"))


def collect():
    out = {name: fresh_case(name) for name in CASES}
    out[PLAIN_ORDER] = plain_order_digest()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--case", default=None)
    args = ap.parse_args()
    if args.case is not None:
        print(fresh_case(args.case))
        return
    first, second = collect(), collect()
    if first != second:
        for name in first:
            if first[name] != second[name]:
                print("case %s differs between two runs:\n  %s\n  %s" % (name, first[name], second[name]))
        raise SystemExit("two runs differ: nothing written")
    if first[PLAIN_ORDER] != first[PLAIN_ORDER_OF] or first[SAME_GAMES[0]] != first[SAME_GAMES[1]]:
        raise SystemExit("cases that must agree differ: nothing written\n%s" % json.dumps(first, indent=1))
    with open(args.out, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (args.out, len(first)))


if __name__ == "__main__":
    main()
