"""Forced playouts at the root and policy target pruning (include/azx.h, "Forced playouts at the root and policy target
pruning") restated on the CPU.  The oracle's C search cannot express the rule, so this file holds a small numpy float32
restatement of its osearch (oracle/mcts.c:87-260: score_and_pick, virtual loss, dedup, expand, backup) with the rule as a
parameter, plus the prune function.  Rules come from the unmodified oracle.Hex; evaluations are restated: uniform prior
from the float32 1/k table, value 0 ("uniform") or the oracle's fnv1a hash of the mover's-view board ("hash").  With the
rule off the restatement equals the unmodified oracle bit for bit on every position (tests/test_forced_playouts_api.py
pins that).

Setup: a frozen Settings (tests/early_stop_reference.py: board, simulations, batch, c_puct, the oracle tree's capacity;
the float32 1/k table follows from the board), by default 5x5, 200 simulations, batch 10, c_puct 0.5; no noise.
Positions of the default setup: the prefixes of 6 games from RandomState(20261020), each opening with two random plies
and then following the UNFORCED search's first most-visited child, to at most 14 plies.  Other boards' positions are
tests/option_positions.py's, through position().

Shared by tests/test_forced_playouts_api.py (CPU) and tests/test_gpu_forced_playouts.py; the references are computed once
per process and never changed."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from early_stop_reference import DEFAULT, Settings, game_at  # noqa: E402,F401
from early_stop_reference import evaluator as oracle_evaluator  # noqa: E402,F401

f32 = np.float32
N, CELLS = DEFAULT.n, DEFAULT.cells
SIMS, BS, C_PUCT = DEFAULT.sims, DEFAULT.bs, DEFAULT.c_puct
NB = DEFAULT.nb                         # select batches of a full search (mcts.py:268)
K_FORCED = 2.0
SEED, N_GAMES, MAX_PLIES = 20261020, 6, 14
TABLE = DEFAULT.table                   # float32 1/k
KINDS = ("hash", "uniform")


def evaluate(h, kind):
    """(value, k) of a non-terminal position: the oracle's built-in evaluators restated (oracle/mcts.c:270-285)."""
    from oracle import oracle as orc
    moves = h.legal_moves()
    if kind == "uniform":
        return f32(0.0), len(moves)
    board = h.board
    if h.color == 1:                                            # the second player moves: the mover's view is the flip
        board, _ = orc.flip_board_moves(board, moves)
    return f32(float(orc.fnv1a(board) & 0xffff) / 32768.0 - 1.0), len(moves)


class Search:
    """One search of `prefix` on a fresh tree: osearch op by op in float32, with the forcing rule (k > 0) in the root
    level of every select.  Afterwards: n, w, p (the root children's visits, values and priors), forced (selects
    whose forced set was non-empty) and overrode (of those, the selects whose forced child was not the argmax)."""

    def __init__(self, prefix, kind, k=0.0, sims=None, bs=None, c_puct=None, cfg=DEFAULT):
        sims = cfg.sims if sims is None else sims
        bs = cfg.bs if bs is None else bs
        c_puct = cfg.c_puct if c_puct is None else c_puct
        self.table = cfg.table
        cap = 1 + cfg.cells + (sims // bs + 1) * bs * cfg.cells
        self.parent = np.full(cap, -1, np.int64)
        self.first = np.full(cap, -1, np.int64)
        self.nch = np.full(cap, -1, np.int64)
        self.nv, self.tv, self.pp = np.zeros(cap, f32), np.zeros(cap, f32), np.zeros(cap, f32)
        self.pp[0] = 1.0
        self.num_nodes = 1
        self.kind, self.k, self.c32 = kind, f32(k), f32(c_puct)
        self.forced = self.overrode = 0
        self.forced_at = []                                     # the forced child's index, one per forced select
        self.games = {0: game_at(prefix, cfg)}                  # node -> position
        self.moves = {}                                         # expanded node -> its legal moves
        root = self.games[0]
        assert root.result == 0
        _, k0 = evaluate(root, kind)                            # evaluate_root: the value is discarded (mcts.py:18-27)
        self.expand(0, k0)
        for _ in range(sims // bs + 1):
            self.batch(bs)
        sl = slice(self.first[0], self.first[0] + self.nch[0])
        self.n, self.w, self.p = self.nv[sl].copy(), self.tv[sl].copy(), self.pp[sl].copy()

    def expand(self, node, k):
        first = self.num_nodes
        self.num_nodes += k
        self.first[node], self.nch[node] = first, k
        self.parent[first:first + k] = node
        self.pp[first:first + k] = self.table[k]
        self.moves[node] = self.games[node].legal_moves()

    def pick(self, node):
        """score_actions + np.argmax (mcts.py:119-136, :112), and at the root the forced set's lowest member."""
        sl = slice(self.first[node], self.first[node] + self.nch[node])
        nv, tv, P = self.nv[sl], self.tv[sl], self.pp[sl]
        S = f32(nv.sum(dtype=np.float64))                       # integers: exact in any order
        gap = np.sqrt(S) / (f32(1.0) + nv)
        U = (self.c32 * P) * gap
        Q = (-tv) / np.maximum(nv, f32(1.0))
        best = int(np.argmax(Q + U))
        if node == 0 and self.k > 0:
            forced = np.flatnonzero((nv > 0) & (nv * nv < (self.k * P) * S))
            if len(forced):
                self.forced += 1
                self.forced_at.append(int(forced[0]))
                self.overrode += int(forced[0]) != best
                best = int(forced[0])
        return best

    def batch(self, bs):
        leaves = []
        for _ in range(bs):                                     # select_batch (mcts.py:62-70)
            node = 0
            while self.nch[node] > 0:
                child = self.pick(node)
                nxt = int(self.first[node]) + child
                if nxt not in self.games:
                    g = self.games[node].copy()
                    g.step(int(self.moves[node][child]))
                    self.games[nxt] = g
                node = nxt
            self.virtual_loss(node, f32(1.0))
            leaves.append(node)
        for node in leaves:                                     # mcts.py:72
            self.virtual_loss(node, f32(-1.0))
        unique = list(dict.fromkeys(leaves))                    # deduplicate_leaves keeps the first occurrence
        values = []
        for node in unique:
            g = self.games[node]
            if g.result != 0:
                values.append(f32(-1.0))                        # mcts.py:194-195
                k = 0
            else:
                v, k = evaluate(g, self.kind)
                values.append(v)
            if self.nch[node] != 0:                             # not already terminal
                self.expand(node, k)
        for node, v in zip(unique, values):                     # backup_batch (mcts.py:242-255)
            while True:
                self.tv[node] += v
                self.nv[node] += f32(1.0)
                v = -v
                if node == 0:
                    break
                node = int(self.parent[node])

    def virtual_loss(self, node, amount):
        while node != 0:
            self.nv[node] += amount
            self.tv[node] += amount
            node = int(self.parent[node])


def prune(n, w, P, k=K_FORCED, c=C_PUCT, b=None):
    """The pruned counts r of include/azx.h, float32 op by op: children below the maximum give back the visits PUCT,
    measured against the first most-visited child, would not have spent on them; a child reduced to one visit loses
    that too.  Maxima and unvisited children keep their count.  (`b`: measure against this most-visited child instead
    of the first -- NOT the rule; for the conditions on test inputs that must tell the two apart.)"""
    n, w, P = (np.asarray(a, f32) for a in (n, w, P))
    k, c = f32(k), f32(c)
    r = n.copy()
    if len(n) == 0 or not n.max() > 0:
        return r
    S = f32(n.sum(dtype=np.float64))
    sq = np.sqrt(S)
    n_max = n.max()
    if b is None:
        b = int(np.argmax(n))                                   # the first index with n_b == n_max
    assert n[b] == n_max
    puct_b = (-w[b]) / n[b] + (c * P[b]) * (sq / (f32(1.0) + n[b]))
    sel = (n > 0) & (n < n_max)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Q = (-w) / n
        gap = puct_b - Q
        f = np.sqrt((k * P) * S)
        need = ((c * P) * sq) / gap - f32(1.0)
        ri = np.ceil(np.maximum(n - f, need))
        ri = np.minimum(np.maximum(ri, f32(0.0)), n)
        ri = np.where((ri < n) & (ri <= 1), f32(0.0), ri)
    sel &= gap > 0
    r[sel] = ri[sel]
    return r.astype(f32)


def oracle_root(prefix, kind, cfg=DEFAULT):
    """(visits, values, priors) of the root's children after the UNMODIFIED oracle's search of `prefix`."""
    from oracle import oracle as orc
    t = orc.Tree(cfg.tree_cap)
    st = orc.search(t, game_at(prefix, cfg), oracle_evaluator(kind, cfg), cfg.sims, cfg.bs, cfg.c_puct)
    assert st.status == 0
    nv, tv, pp, _, _ = t.root_stats()
    return np.asarray(nv, f32), np.asarray(tv, f32), np.asarray(pp, f32)


@functools.lru_cache(maxsize=None)
def prefixes(kind):
    """Every non-terminal prefix, from the two opening plies on, of the N_GAMES unforced greedy games."""
    rng = np.random.RandomState(SEED)
    out = []
    for _ in range(N_GAMES):
        moves = [int(c) + 1 for c in rng.permutation(CELLS)[:2]]
        while not game_at(moves).result and len(moves) < MAX_PLIES:
            nv, _, _ = oracle_root(moves, kind)
            moves.append(int(game_at(moves).legal_moves()[int(np.argmax(nv))]))
        out += [tuple(moves[:n]) for n in range(2, len(moves)) if not game_at(moves[:n]).result]
    return tuple(out)


def position(prefix, kind, k=K_FORCED, cfg=DEFAULT):
    """One position's dict: prefix; off_* = the restatement's root with the rule off; n, w, p = its root under
    forcing with `k`; forced / overrode = its forced selects (forced_at: the forced child's index, select by select);
    r = prune(n, w, p); removed = visits the prune takes."""
    off, on = Search(prefix, kind, 0.0, cfg=cfg), Search(prefix, kind, k, cfg=cfg)
    r = prune(on.n, on.w, on.p, k, cfg.c_puct)
    return dict(prefix=list(prefix), off_n=off.n, off_w=off.w, off_p=off.p, n=on.n, w=on.w, p=on.p,
                forced=on.forced, overrode=on.overrode, forced_at=tuple(on.forced_at), r=r,
                removed=int((on.n - r).sum()))


@functools.lru_cache(maxsize=None)
def positions(kind, k=K_FORCED):
    """position() of every prefix of prefixes(kind), on the default 5x5 setup."""
    return tuple(position(prefix, kind, k) for prefix in prefixes(kind))


def shares(counts):
    """counts / sum(counts), one float32 division per child: the row of AZX_ROWS_VISITS, and the reference's at T = 1."""
    counts = np.asarray(counts, f32)
    return counts / f32(counts.sum(dtype=np.float64))
