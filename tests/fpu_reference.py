"""First-play urgency (include/azx.h, "First-play urgency (FPU) for the PUCT search") restated on the CPU:
tests/forced_playouts_reference.py's Search -- the numpy float32 restatement of the oracle's search, bit-equal to the
unmodified oracle with no rule set -- with `pick` replaced by the definition: a child with num_visits == 0 takes
Q = fpu.  The rule is a mixin (FpuRule), so that it composes with the forcing rule of forced_playouts_reference.Search and
with the Gumbel root search of gumbel_reference.Search (GumbelSearch below) without restating either.

Beyond the parent class, the restatement here
  - keeps the whole tree (the six arrays of azx_tree_dump: parent, first_child, num_children, num_visits, total_value,
    prior_prob) and can move its root to a child and search again on the carried subtree (the never-free arena of the
    reference: AZX_FLAG_NO_COMPACT on the device);
  - mixes uploaded root noise rows into the root's priors as the tree kernels do (mcts.py:128-130);
  - has a third evaluator, "skew", with NON-UNIFORM priors: value as "hash", prior j proportional to
    1 + ((fnv1a(mover's-view board) >> j) & 3) (0 beyond bit 31), normalised in float64 and rounded to float32.  Uniform
    priors make the visited mass a multiple of 1/k and would hide an error in the fixed-point sum.  On the device the same
    function goes in through Engine.search_external (skew_host_evaluator);
  - counts what azx_fpu_stats counts.

Shared by tests/test_fpu_api.py (CPU) and tests/test_gpu_fpu.py; the references are computed once per process and never
changed."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from azalea_amd import _lib  # noqa: E402

# the restatement is the reference OF the library's option: without its entry points there is nothing to be the reference of
_lib.lib().azx_set_fpu, _lib.lib().azx_fpu_score

import forced_playouts_reference as fp  # noqa: E402
import gumbel_reference as gr  # noqa: E402
from early_stop_reference import DEFAULT, Settings, game_at  # noqa: E402,F401

f32 = np.float32
KINDS = ("uniform", "hash", "skew")
TWO24 = f32(16777216.0)
INV_TWO24 = f32(1.0) / TWO24

OFF = ("off", 0.0, 0.0, 0.0)
# (mode, value, reduction, root_reduction): the settings the issue names
MODES = (("absolute", -1.0, 0.0, 0.0), ("absolute", 0.25, 0.0, 0.0), ("reduction", 0.0, 0.25, 0.0),
         ("reduction", 0.0, 0.5, 0.5), ("reduction", 0.0, 0.0, 0.0))


def mode_id(m):
    return "%s_%g_%g_%g" % m


def fpu_value(mode, nv_p, tv_p, nv, P, r):
    """Q of the unvisited children: the definition, one float32 operation at a time."""
    name, value = mode[0], mode[1]
    if name == "absolute":
        return f32(value)
    qp = f32(tv_p) / np.maximum(f32(nv_p), f32(1.0))
    vis = nv > 0
    M = int((P[vis] * TWO24).astype(np.uint32).sum(dtype=np.uint64))
    assert M < 1 << 32
    mass = f32(M) * INV_TWO24
    return f32(qp - f32(f32(r) * np.sqrt(mass)))


def pick_child(mode, nv_p, tv_p, nv, tv, P_stored, P_scored, c32, is_root):
    """(argmax, Q + U) of one node under `mode`: score_actions + np.argmax (mcts.py:119-136, :112) op by op in float32
    with the unvisited children's Q from the definition.  P_stored is the stored prior (the mass), P_scored the prior
    the select scores with (the noise-mixed one at a noisy root)."""
    S = f32(nv.sum(dtype=np.float64))                           # integers: exact in any order
    gap = np.sqrt(S) / (f32(1.0) + nv)
    U = (c32 * P_scored) * gap
    Q = (-tv) / np.maximum(nv, f32(1.0))
    if mode[0] != "off":
        r = mode[3] if is_root else mode[2]
        Q = np.where(nv == 0, fpu_value(mode, nv_p, tv_p, nv, P_stored, r), Q).astype(f32)
    score = Q + U
    return int(np.argmax(score)), score


def skew_prior(h32, k):
    """float32 w / sum(w), w_j = 1 + ((h32 >> j) & 3) for j < k (shifts past bit 31 give 0): one float64 division per
    child, rounded to float32 once."""
    w = np.array([1 + ((int(h32) >> j) & 3) for j in range(k)], np.float64)
    return (w / w.sum()).astype(f32)


def mover_view(h):
    from oracle import oracle as orc
    board = h.board
    if h.color == 1:                                            # the second player moves: the mover's view is the flip
        board, _ = orc.flip_board_moves(board, h.legal_moves())
    return board


def evaluate(h, kind):
    """(value, k, priors or None) of a non-terminal position; None = the float32 1/k table."""
    from oracle import oracle as orc
    if kind != "skew":
        v, k = fp.evaluate(h, kind)
        return v, k, None
    k = len(h.legal_moves())
    h32 = orc.fnv1a(mover_view(h))
    return f32(float(h32 & 0xffff) / 32768.0 - 1.0), k, skew_prior(h32, k)


def skew_host_evaluator():
    """The "skew" evaluator for Engine.search_external: evaluate(boards, legal_moves, slot, k) -> (value, prior)."""
    from oracle import oracle as orc

    def fn(boards, lm, slot, k):
        v = np.zeros(len(k), f32)
        p = np.zeros((len(k), lm.shape[1]), f32)
        for i in range(len(k)):
            h32 = orc.fnv1a(boards[i])
            v[i] = f32(float(h32 & 0xffff) / 32768.0 - 1.0)
            p[i, :k[i]] = skew_prior(h32, int(k[i]))
        return v, p
    return fn


class FpuRule:
    """The rule and what goes with it, for a class derived from fp.Search: root-aware select / backup (so that the root
    can move), root noise, the "skew" evaluator, the statistics.  set_rule() must be called before the parent class's
    __init__ runs the first search."""

    def set_rule(self, fpu=OFF, eval_kind="uniform", noise=None, noise_scale=0.0):
        self.fpu, self.eval_kind = tuple(fpu), eval_kind
        self.root_id, self.sel = 0, 0
        self.noise = None if noise is None else np.asarray(noise, np.float64)     # [n_select, >= k]
        self.eps = float(noise_scale)
        self.keep32 = f32(1.0 - self.eps)
        self.stat_selects = self.stat_levels = self.stat_unvisited = 0

    # ---- one node ----
    def children(self, node):
        sl = slice(self.first[node], self.first[node] + self.nch[node])
        return self.nv[sl], self.tv[sl], self.pp[sl]

    def fpu_pick(self, node):
        """(argmax, the priors the select scored with) under the rule."""
        nv, tv, P = self.children(node)
        Ps = P
        if node == self.root_id and self.noise is not None and self.eps != 0.0:
            row = self.noise[self.sel, :len(P)]
            Ps = ((self.keep32 * P).astype(np.float64) + self.eps * row).astype(f32)          # mcts.py:130
        best, _ = pick_child(self.fpu, self.nv[node], self.tv[node], nv, tv, P, Ps, self.c32, node == self.root_id)
        if self.fpu[0] != "off" and (nv == 0).any():
            self.stat_levels += 1
        return best, Ps

    def pick(self, node):
        if node == self.root_id and getattr(self, "m", 0):         # the Gumbel root search replaces the root's selection
            return gr.Search.pick(self, node)
        best, Ps = self.fpu_pick(node)
        if node == self.root_id and self.k > 0:                    # forced playouts override the argmax computed with FPU
            nv, _, _ = self.children(node)
            S = f32(nv.sum(dtype=np.float64))
            forced = np.flatnonzero((nv > 0) & (nv * nv < (self.k * Ps) * S))
            if len(forced):
                self.forced += 1
                self.forced_at.append(int(forced[0]))
                self.overrode += int(forced[0]) != best
                best = int(forced[0])
        return best

    # ---- the search around it (fp.Search.batch with a movable root and the third evaluator) ----
    def expand_priors(self, node, k, priors):
        fp.Search.expand(self, node, k)
        if priors is not None and k:
            first = int(self.first[node])
            self.pp[first:first + k] = priors

    def batch(self, bs):
        if getattr(self, "m", 0):
            self.boundary()
        leaves = []
        for _ in range(bs):                                     # select_batch (mcts.py:62-70)
            node = self.root_id
            while self.nch[node] > 0:
                child = self.pick(node)
                nxt = int(self.first[node]) + child
                if nxt not in self.games:
                    g = self.games[node].copy()
                    g.step(int(self.moves[node][child]))
                    self.games[nxt] = g
                node = nxt
            self.sel += 1
            if self.fpu[0] != "off":
                self.stat_selects += 1
                self.stat_unvisited += int(self.nv[node] == 0)
            self.virtual_loss(node, f32(1.0))
            leaves.append(node)
        for node in leaves:                                     # mcts.py:72
            self.virtual_loss(node, f32(-1.0))
        unique = list(dict.fromkeys(leaves))                    # deduplicate_leaves keeps the first occurrence
        values, kids = [], []
        for node in unique:
            g = self.games[node]
            if g.result != 0:
                values.append(f32(-1.0))                        # mcts.py:194-195
                kids.append((0, None))
            else:
                v, k, pri = evaluate(g, self.eval_kind)
                values.append(v)
                kids.append((k, pri))
        for node, (k, pri) in zip(unique, kids):
            if self.nch[node] != 0:                             # not already terminal
                self.expand_priors(node, k, pri)
        for node, v in zip(unique, values):                     # backup_batch (mcts.py:242-255)
            while True:
                self.tv[node] += v
                self.nv[node] += f32(1.0)
                v = -v
                if node == self.root_id:
                    break
                node = int(self.parent[node])
        if getattr(self, "m", 0):
            self.b += 1

    def virtual_loss(self, node, amount):
        while node != self.root_id:
            self.nv[node] += amount
            self.tv[node] += amount
            node = int(self.parent[node])

    def expand(self, node, k):
        """(the root's expansion in fp.Search.__init__ comes through here)"""
        pri = None
        if self.eval_kind == "skew" and k:
            pri = evaluate(self.games[node], "skew")[2]
        self.expand_priors(node, k, pri)

    # ---- results ----
    def root_children(self):
        nv, tv, pp = self.children(self.root_id)
        return nv.copy(), tv.copy(), pp.copy()

    def dump(self):
        """The six arrays of azx_tree_dump, num_nodes and root_id."""
        n = self.num_nodes
        return dict(num_nodes=n, root_id=self.root_id, parent=self.parent[:n].astype(np.int32),
                    first_child=self.first[:n].astype(np.int32), num_children=self.nch[:n].astype(np.int32),
                    num_visits=self.nv[:n].copy(), total_value=self.tv[:n].copy(), prior_prob=self.pp[:n].copy())

    def stats(self):
        return dict(selects=self.stat_selects, levels_with_unvisited=self.stat_levels,
                    ended_unvisited=self.stat_unvisited, differs_from_off=0)


class Search(FpuRule, fp.Search):
    """One search of `prefix` on a fresh tree under `fpu` = (mode, value, reduction, root_reduction); `forced_k`: the
    forcing rule beside it.  move_and_search(child) plays a root child and searches the carried subtree."""

    def __init__(self, prefix, kind, fpu=OFF, forced_k=0.0, sims=None, bs=None, c_puct=None, cfg=DEFAULT, noise=None,
                 noise_scale=0.0):
        self.set_rule(fpu, kind, noise, noise_scale)
        self.cfg, self.sims_, self.bs_ = cfg, (cfg.sims if sims is None else sims), (cfg.bs if bs is None else bs)
        fp.Search.__init__(self, prefix, "uniform" if kind == "skew" else kind, forced_k, sims=sims, bs=bs,
                           c_puct=c_puct, cfg=self.cfg)

    def move_and_search(self, child, noise=None):
        """tree.move(child) (search_tree.py: the root becomes that child, nothing is freed) and one more search."""
        need = self.num_nodes + (self.sims_ // self.bs_ + 1) * self.bs_ * self.cfg.cells + 1
        if need > len(self.nv):
            grow = need - len(self.nv)
            self.parent = np.concatenate([self.parent, np.full(grow, -1, np.int64)])
            self.first = np.concatenate([self.first, np.full(grow, -1, np.int64)])
            self.nch = np.concatenate([self.nch, np.full(grow, -1, np.int64)])
            self.nv, self.tv, self.pp = (np.concatenate([a, np.zeros(grow, f32)]) for a in (self.nv, self.tv, self.pp))
        nxt = int(self.first[self.root_id]) + int(child)
        if nxt not in self.games:
            g = self.games[self.root_id].copy()
            g.step(int(self.moves[self.root_id][child]))
            self.games[nxt] = g
        self.root_id, self.sel = nxt, 0
        if noise is not None:
            self.noise = np.asarray(noise, np.float64)
        assert self.games[nxt].result == 0
        if self.nch[nxt] < 0:                                   # evaluate_root of an unexpanded root (value discarded)
            _, k, pri = evaluate(self.games[nxt], self.eval_kind)
            self.expand_priors(nxt, k, pri)
        for _ in range(self.sims_ // self.bs_ + 1):
            self.batch(self.bs_)
        self.n, self.w, self.p = self.root_children()


class GumbelSearch(FpuRule, gr.Search):
    """gumbel_reference.Search (the Gumbel root search) with the FPU rule below the root."""

    def __init__(self, prefix, kind, fpu=OFF, **kw):
        self.set_rule(fpu, kind)
        gr.Search.__init__(self, prefix, kind, **kw)

    def expand(self, node, k):
        gr.Search.expand(self, node, k)


def oracle_dump(prefix, kind, cfg, sims, bs, follow=()):
    """The UNMODIFIED oracle's tree dump after searching `prefix` (and, for each child of `follow`, moving to it and
    searching again)."""
    from oracle import oracle as orc
    import early_stop_reference as es
    t = orc.Tree(cfg.tree_cap)
    h = game_at(prefix, cfg)
    ev = es.evaluator(kind, cfg)
    st = orc.search(t, h, ev, sims, bs, cfg.c_puct)
    assert st.status == 0
    for child in follow:
        mv = int(h.legal_moves()[child])
        t.move(child)
        h.step(mv)
        st = orc.search(t, h, ev, sims, bs, cfg.c_puct)
        assert st.status == 0
    return t.dump()


def prefix_third(n, seed=0):
    """A legal, unfinished prefix of about a third of the board's cells."""
    import option_positions as op
    rng = np.random.RandomState(9000 + 17 * n + seed)
    return op.random_prefix(rng, Settings(n=n), (n * n) // 3)


def most_visited(search):
    return int(np.argmax(search.root_children()[0]))


@functools.lru_cache(maxsize=None)
def tree_case(n, bs, sims, kind, mode, prefix, c_puct=0.5):
    """dump() and stats() of one search under `mode`."""
    cfg = Settings(n=n, sims=sims, bs=bs, c_puct=c_puct, tree_cap=1 << 17)
    s = Search(prefix, kind, mode, cfg=cfg)
    return s.dump(), s.stats()
