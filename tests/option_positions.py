"""Position families for the self-play options (forced playouts and pruning, early stop) on boards whose roots span
more than one 64-lane word of children: 9x9 (k <= 81, the smallest two-word case), 11x11, 12x12 (the third word holds
16 lanes or fewer) and 13x13 (three words; longer prefixes give two and one inside the three-word kernels).  A plain 5x5
root has at most 25 children, so nothing tests/forced_playouts_reference.py and tests/early_stop_reference.py hold there
runs an "across words" loop more than once.

Families (every prefix is built step by step on oracle.Hex and is a legal, unfinished game):
  sweep        "uniform" evaluator, c_puct 0.5, a few random plies: value 0 everywhere, so the forced child sweeps
               upward through the words.  13x13 adds longer random prefixes (k <= 128 and k <= 64).
  win-at-rank  "uniform", c_puct 0.5: the first player's stones fill a whole column except one gap cell (the first
               player connects top to bottom), the second player's lie elsewhere, the first player is to move.  The
               search finds the win once the sweep reaches it and then concentrates on it: a leader, an early stop and
               pruned children at a chosen rank.  A winning chain takes n - 1 stones of each colour, so k = n*n - 2n + 2:
               122 on 12x12, where no such position has a third word (13x13: 145).
  wide-hash    "hash" evaluator at c_puct 4: wide enough for visited, forced and pruned children in word 1.
  wider-hash   "hash" at c_puct 12, on 12x12 and 13x13 only: the sweep passes word 2 before the values take over, which
               puts pruned children of a "hash" search (and of any 12x12 search) in the third word.
  tied-max     "hash" at c_puct 4: prefixes (the same scan, the same file) whose forced search ends with the most-visited
               count shared by children in two words, with pruned counts that depend on which one is measured against.
  stop-hash    "hash" at c_puct 0.5: prefixes found by a CPU scan (tests/golden/make_option_prefixes.py) and kept as
               data in tests/golden/g14_option_prefixes.json; their expected values are recomputed here, never stored.

Shared by tests/test_options_wide_boards_api.py (CPU: the conditions on these inputs) and
tests/test_gpu_options_wide_boards.py; the references are computed once per process and never changed."""
import functools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import early_stop_reference as es  # noqa: E402
import forced_playouts_reference as fp  # noqa: E402
from early_stop_reference import Settings  # noqa: E402

BOARDS = (9, 11, 12, 13)
SIMS, BS = 400, 10
K_FORCED = fp.K_FORCED
TREE_CAP = 1 << 17                      # 13x13: 1 + 169 + 410 * 169 nodes at the most
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_option_prefixes.json")


def narrow(n):
    """c_puct 0.5, the tests' value: sweep and win-at-rank ("uniform"), stop-hash ("hash")."""
    return Settings(n=n, sims=SIMS, bs=BS, c_puct=0.5, tree_cap=TREE_CAP)


def wide(n):
    """c_puct 4: wide-hash."""
    return Settings(n=n, sims=SIMS, bs=BS, c_puct=4.0, tree_cap=TREE_CAP)


def wider(n):
    """c_puct 12: wider-hash."""
    return Settings(n=n, sims=SIMS, bs=BS, c_puct=12.0, tree_cap=TREE_CAP)


WIDER_BOARDS = (12, 13)


def words_of(n):
    """The 64-lane words an empty n x n board's root has."""
    return (n * n + 63) // 64


def random_prefix(rng, cfg, plies):
    """`plies` random legal moves from the empty board, unfinished (drawn again until it is)."""
    while True:
        h, moves = es.game_at([], cfg), []
        while len(moves) < plies and not h.result:
            legal = h.legal_moves()
            moves.append(int(legal[rng.randint(len(legal))]))
            h.step(moves[-1])
        if not h.result:
            return tuple(moves)


# 13x13: k = 169 - plies > 128, in (64, 128] and <= 64: root_pick's RS 3, 2 and 1 inside the SLOTS = 3 kernels
SWEEP_PLIES = {9: (2, 3, 4, 6), 11: (2, 3, 4, 6), 12: (2, 3, 4, 6), 13: (2, 3, 4, 6, 60, 110)}


@functools.lru_cache(maxsize=None)
def sweep_prefixes(n):
    rng = np.random.RandomState(1000 + n)
    return tuple(random_prefix(rng, narrow(n), plies) for plies in SWEEP_PLIES[n])


def column_with_gap(n, col, gap_row):
    """The prefix of 2 * (n - 1) plies: the first player on every cell of column `col` but row `gap_row`, the second on
    the highest-index cells outside the column (they leave the ranks before the gap alone); first player to move.
    Cells are row-major from 1.  Returns (prefix, rank of the winning child)."""
    mine = [r * n + col + 1 for r in range(n) if r != gap_row]
    free = [c for c in range(1, n * n + 1) if (c - 1) % n != col]
    theirs = free[-(n - 1):]
    prefix = []
    for a, b in zip(mine, theirs):
        prefix += [a, b]
    win = gap_row * n + col + 1
    taken = set(prefix)
    rank = sum(1 for c in range(1, win) if c not in taken)
    return tuple(prefix), rank


# (column, gap row): chosen for ranks in every word the position has
WIN_SPOTS = {
    9: ((1, 0), (4, 2), (7, 3), (3, 7), (6, 8), (8, 8), (2, 8)),
    11: ((1, 0), (5, 2), (9, 4), (3, 7), (6, 8), (8, 9), (10, 9)),
    12: ((1, 0), (5, 2), (9, 4), (3, 7), (6, 8), (8, 9), (10, 10)),
    13: ((1, 0), (5, 2), (9, 3), (3, 6), (6, 7), (8, 8), (10, 9),
         (11, 11), (12, 11), (9, 12), (12, 12)),
}


@functools.lru_cache(maxsize=None)
def win_prefixes(n):
    """((prefix, rank of the winning child), ...)"""
    return tuple(column_with_gap(n, *spot) for spot in WIN_SPOTS[n])


WIDE_HASH_PLIES = (2, 4, 5)


@functools.lru_cache(maxsize=None)
def wide_hash_prefixes(n):
    rng = np.random.RandomState(2000 + n)
    return tuple(random_prefix(rng, wide(n), plies) for plies in WIDE_HASH_PLIES)


@functools.lru_cache(maxsize=None)
def wider_hash_prefixes(n):
    rng = np.random.RandomState(4000 + n)
    return tuple(random_prefix(rng, wider(n), plies) for plies in WIDE_HASH_PLIES)


@functools.lru_cache(maxsize=None)
def tied_max_prefixes(n):
    with open(GOLDEN) as f:
        return tuple(tuple(p) for p in json.load(f)["tied_max"][str(n)])


def later_maximum(n):
    """The first most-visited child of the LAST word that holds one, where that is not the first most-visited child's
    word; else None."""
    idx = np.flatnonzero(np.asarray(n) == np.max(n))
    if len(idx) == 0 or (idx[0] >> 6) == (idx[-1] >> 6):
        return None
    return int(idx[(idx >> 6) == (idx[-1] >> 6)][0])


@functools.lru_cache(maxsize=None)
def stop_hash_prefixes(n):
    with open(GOLDEN) as f:
        return tuple(tuple(p) for p in json.load(f)["stop_hash"][str(n)])


# ---- references ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forced_refs(n, family):
    """forced_playouts_reference.position() of every prefix of the family ("sweep", "win", "wide_hash", "tied_max",
    "wider_hash"); the dicts also carry `family` and, for "win", `win_rank`."""
    if family == "sweep":
        kind, cfg, items = "uniform", narrow(n), [(p, None) for p in sweep_prefixes(n)]
    elif family == "win":
        kind, cfg, items = "uniform", narrow(n), list(win_prefixes(n))
    elif family == "wide_hash":
        kind, cfg, items = "hash", wide(n), [(p, None) for p in wide_hash_prefixes(n)]
    elif family == "tied_max":
        kind, cfg, items = "hash", wide(n), [(p, None) for p in tied_max_prefixes(n)]
    else:
        assert family == "wider_hash" and n in WIDER_BOARDS
        kind, cfg, items = "hash", wider(n), [(p, None) for p in wider_hash_prefixes(n)]
    out = []
    for prefix, rank in items:
        r = fp.position(prefix, kind, K_FORCED, cfg)
        r.update(family=family, win_rank=rank)
        out.append(r)
    return tuple(out)


def forced_set(n, kind):
    """(cfg, refs) of the one engine that plays a board's positions of `kind`: "uniform" = sweep + win-at-rank,
    "hash" = wide-hash + tied-max, "hash_wider" = wider-hash."""
    if kind == "uniform":
        return narrow(n), forced_refs(n, "sweep") + forced_refs(n, "win")
    if kind == "hash_wider":
        return wider(n), forced_refs(n, "wider_hash")
    return wide(n), forced_refs(n, "wide_hash") + forced_refs(n, "tied_max")


@functools.lru_cache(maxsize=None)
def stop_refs(n, family):
    """(early_stop_reference.reference() of every prefix of the family ("win", "stop_hash", "sweep"), ties dropped;
    the number dropped)."""
    cfg = narrow(n)
    if family == "win":
        kind, prefixes = "uniform", [p for p, _ in win_prefixes(n)]
    elif family == "sweep":
        kind, prefixes = "uniform", list(sweep_prefixes(n))
    else:
        assert family == "stop_hash"
        kind, prefixes = "hash", list(stop_hash_prefixes(n))
    refs, dropped = [], 0
    for prefix in prefixes:
        r = es.reference(prefix, kind, cfg)
        if r is None:
            dropped += 1
        else:
            r["family"] = family
            refs.append(r)
    return tuple(refs), dropped


def stop_set(n, kind):
    """(cfg, refs) of the one engine that plays a board's early-stop positions of `kind`: "uniform" = win-at-rank and
    the sweep positions that do not end in a tie, "hash" = stop-hash."""
    if kind == "uniform":
        return narrow(n), stop_refs(n, "win")[0] + stop_refs(n, "sweep")[0]
    return narrow(n), stop_refs(n, "stop_hash")[0]


# ---- beyond the sqrt table: a 5x5 root whose visit sum passes AZX_SQRT_TAB = 4096 ------------------------------------------
LONG = Settings(n=5, sims=4600, bs=10, c_puct=0.5, tree_cap=1 << 17)      # 1 + 25 + 461 * 10 * 25 nodes at the most
LONG_PREFIXES = ((), (13, 7), (1, 25, 13, 12))


@functools.lru_cache(maxsize=None)
def long_refs():
    return tuple(fp.position(p, "uniform", K_FORCED, LONG) for p in LONG_PREFIXES)


def by_word(indices, n_words):
    """How many of the child indices fall in each 64-lane word."""
    c = np.bincount(np.asarray(list(indices), np.int64) >> 6, minlength=n_words)
    return [int(x) for x in c[:n_words]] + [int(c[n_words:].sum())] * (len(c) > n_words)


def pruned_children(refs):
    """The indices of the children the prune reduced, over the set."""
    return [int(i) for r in refs for i in np.flatnonzero(r["r"] < r["n"])]
