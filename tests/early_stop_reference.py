"""The early-stop rule of include/azx.h ("Early stop of a search whose move can no longer change") over the UNMODIFIED
CPU oracle: a position's search is run on a fresh oracle Tree one select batch at a time (oracle.search with
simulations = bs - 1 runs exactly one batch; a chain of such calls leaves the tree one call of the whole search leaves,
tests/test_early_stop_api.py holds that), and after every batch the rule is tested on the root children's visit counts.

Board size, simulations, batch, c_puct and the oracle tree's capacity are a frozen Settings (the float32 1/k table
follows from the board); the default is the 5x5 setup every function had before it took one.

Positions: every non-terminal prefix of a few oracle-greedy 5x5 games that open with two random plies.  A position whose
FULL search ends with a tie for most visits is dropped: the device breaks such a tie by a draw.

Shared by tests/test_early_stop_api.py (CPU) and tests/test_gpu_early_stop.py; the references are computed once per
process and never changed."""
import dataclasses
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@functools.lru_cache(maxsize=None)
def table_for(cells):
    """float32 1/k for k = 0 .. cells (1/1 at 0): the engine's prior table."""
    return (np.float32(1.0) / np.arange(0, cells + 1).clip(1).astype(np.float32)).astype(np.float32)


@dataclasses.dataclass(frozen=True)
class Settings:
    """One search setup: hashable, so that the lru_caches of the reference modules key on it."""
    n: int = 5
    sims: int = 200
    bs: int = 10
    c_puct: float = 0.5
    tree_cap: int = 1 << 16            # nodes of the oracle's Tree

    @property
    def cells(self):
        return self.n * self.n

    @property
    def nb(self):
        return self.sims // self.bs + 1     # select batches of a full search (mcts.py:268)

    @property
    def table(self):
        return table_for(self.cells)


DEFAULT = Settings()
N, CELLS = DEFAULT.n, DEFAULT.cells
SIMS, BS, C_PUCT = DEFAULT.sims, DEFAULT.bs, DEFAULT.c_puct
NB = DEFAULT.nb
TABLE = DEFAULT.table
MAX_DROPPED_SHARE, MIN_STOPPING = 0.10, 40     # the caps on the inputs (conditions, asserted by positions())


def evaluator(kind, cfg=DEFAULT):
    from oracle import oracle as orc
    if kind == "hash":
        return orc.UniformEval(hash_value=True, prior_by_k=cfg.table)
    assert kind == "uniform"
    return orc.UniformEval()


def game_at(prefix, cfg=DEFAULT):
    from oracle import oracle as orc
    h = orc.Hex(cfg.n)
    for m in prefix:
        h.step(m)
    return h


def top_two(counts):
    """(n1, n2, leader): the largest and second-largest count and the first index of the largest; n2 = 0 with one."""
    c = np.asarray(counts, np.float32)
    leader = int(np.argmax(c))
    rest = np.delete(c, leader)
    return float(c[leader]), (float(rest.max()) if len(rest) else 0.0), leader


def rule_holds(counts, batches_left, bs=BS):
    n1, n2, _ = top_two(counts)
    return n1 - n2 > batches_left * bs


def search_batches(prefix, kind, nb=None, bs=None, stop=True, cfg=DEFAULT):
    """Search `prefix` batch by batch on a fresh tree.  Returns (b, tree, leader): b = the number of batches run --
    the first count at which the rule holds (`stop`), else nb -- the oracle tree there and the first most-visited
    child's index."""
    from oracle import oracle as orc
    nb = cfg.nb if nb is None else nb
    bs = cfg.bs if bs is None else bs
    h, ev, t = game_at(prefix, cfg), evaluator(kind, cfg), orc.Tree(cfg.tree_cap)
    b = 0
    while b < nb:
        if stop and b > 0 and rule_holds(t.root_stats()[0], nb - b, bs):
            break
        st = orc.search(t, h, ev, bs - 1, bs, cfg.c_puct)
        assert st.status == 0
        b += 1
    return b, t, top_two(t.root_stats()[0])[2]


def root_after(tree):
    """(child visits, child values, root visits, root value) of the tree's root, as azx_get_root reports a slot's."""
    nv, tv, _, rv, rw = tree.root_stats()
    return (np.asarray(nv, np.float32), np.asarray(tv, np.float32), np.float32(rv), np.float32(rw))


def reference(prefix, kind, cfg=DEFAULT):
    """One position's reference: dict(prefix, b_star, leader, tile, ends, stop_root, full_root, full_leader) -- b_star
    the batch count at which the rule first holds (cfg.nb if never), leader the most-visited child there and `tile` its
    move, `ends` whether that move ends the game, stop_root / full_root the oracle root (root_after) after
    tree.move(leader) of the stopped and of the full search; None for a position whose full search ends in a tie."""
    full_b, full_t, full_leader = search_batches(prefix, kind, stop=False, cfg=cfg)
    counts = full_t.root_stats()[0]
    if (counts == counts.max()).sum() > 1:
        return None
    b_star, t, leader = search_batches(prefix, kind, cfg=cfg)
    h = game_at(prefix, cfg)
    tile = int(h.legal_moves()[leader])
    h.step(tile)
    t.move(leader)
    full_t.move(full_leader)
    return dict(prefix=list(prefix), b_star=b_star, leader=leader, tile=tile, ends=bool(h.result),
                stop_root=root_after(t), full_root=root_after(full_t), full_leader=full_leader)


def greedy_games(kind, n_games, seed, cfg=DEFAULT):
    """Oracle-greedy games (each ply the full search's first most-visited child) after two random opening plies."""
    rng = np.random.RandomState(seed)
    games = []
    for _ in range(n_games):
        moves = [int(c) + 1 for c in rng.permutation(cfg.cells)[:2]]
        while not game_at(moves, cfg).result:
            _, t, leader = search_batches(moves, kind, stop=False, cfg=cfg)
            moves.append(int(game_at(moves, cfg).legal_moves()[leader]))
        games.append(moves)
    return games


@functools.lru_cache(maxsize=None)
def positions(kind="hash", n_games=6, seed=20261019, tail=None, cfg=DEFAULT):
    """The references of every non-terminal prefix (from the two opening plies on; with `tail`, only the last `tail`
    prefixes of each game) of `n_games` greedy games, ties dropped.  Returns (refs, dropped)."""
    refs, dropped = [], 0
    for moves in greedy_games(kind, n_games, seed, cfg):
        lengths = list(range(2, len(moves)))
        for n in (lengths if tail is None else lengths[-tail:]):
            r = reference(moves[:n], kind, cfg)
            if r is None:
                dropped += 1
            else:
                refs.append(r)
    return tuple(refs), dropped


def counts_of(refs, cfg=DEFAULT):
    """What azx_early_stop_stats reports after one ply of every reference position under the option."""
    stopped = [r for r in refs if r["b_star"] < cfg.nb]
    return dict(t0_plies=len(refs), stopped_plies=len(stopped), batches_skipped=sum(cfg.nb - r["b_star"] for r in stopped))
