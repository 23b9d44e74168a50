"""Writes tests/golden/g14_option_prefixes.json: the stop-hash and tied-max prefixes of tests/option_positions.py.

A CPU scan with this repository's own oracle: random mid-game prefixes of each wide board, searched with the "hash"
evaluator at c_puct 0.5 under the early-stop rule (tests/early_stop_reference.py).  Kept per board: up to HIGH prefixes
whose search stops early on a leader in word 1 or above with a move that does not end the game, up to LOW that stop on a
leader in word 0, and up to NEVER that never stop; none whose full search ends in a tie.

A second scan keeps, per board, TIED short prefixes whose forced search ("hash", c_puct 4) ends with the most-visited
count shared by children in two words of the root AND whose pruned counts depend on which of them the prune measures
against: the inputs that tell "the FIRST most-visited child" from any other.

Only the move lists are stored: every expected value is recomputed when the tests run.

    python tests/golden/make_option_prefixes.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import early_stop_reference as es  # noqa: E402
import forced_playouts_reference as fp  # noqa: E402
import option_positions as op  # noqa: E402

TRIES, HIGH, LOW, NEVER = 500, 5, 2, 3
TIED, TIED_TRIES = 3, 400


def scan(n):
    cfg = op.narrow(n)
    rng = np.random.RandomState(3000 + n)
    high, low, never = [], [], []
    for _ in range(TRIES):
        plies = int(rng.randint(2, cfg.cells - 66))             # k >= 67: a leader can lie in word 1
        prefix = op.random_prefix(rng, cfg, plies)
        r = es.reference(prefix, "hash", cfg)
        if r is None:
            continue
        if r["b_star"] == cfg.nb:
            if len(never) < NEVER:
                never.append(prefix)
        elif r["leader"] >= 64 and not r["ends"]:
            if len(high) < HIGH:
                high.append(prefix)
        elif len(low) < LOW:
            low.append(prefix)
    print("%dx%d: stopping on a leader in word 1 or above %d, in word 0 %d, never stopping %d"
          % (n, n, len(high), len(low), len(never)))
    return [list(map(int, p)) for p in high + low + never]


def scan_tied(n):
    cfg = op.wide(n)
    rng = np.random.RandomState(5000 + n)
    found = []
    for _ in range(TIED_TRIES):
        if len(found) == TIED:
            break
        prefix = op.random_prefix(rng, cfg, int(rng.randint(2, 8)))
        s = fp.Search(prefix, "hash", op.K_FORCED, cfg=cfg)
        if op.later_maximum(s.n) is None:
            continue
        r = fp.prune(s.n, s.w, s.p, op.K_FORCED, cfg.c_puct)
        if not np.array_equal(r, fp.prune(s.n, s.w, s.p, op.K_FORCED, cfg.c_puct, b=op.later_maximum(s.n))):
            found.append(prefix)
    print("%dx%d: maximum shared across words with a prune that depends on the child measured against %d" % (n, n, len(found)))
    return [list(map(int, p)) for p in found]


def main():
    out = {"stop_hash": {str(n): scan(n) for n in op.BOARDS}, "tied_max": {str(n): scan_tied(n) for n in op.BOARDS}}
    with open(op.GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
