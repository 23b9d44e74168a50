"""The policy temperature of the search's priors (include/azx.h, "Policy temperature for the search's priors") restated
on the CPU: tests/fpu_reference.py's Search / FpuRule -- the numpy float32 restatement of the oracle's search, bit-equal
to the unmodified oracle with no rule set -- with `expand_priors` and the root's scored priors replaced by the
definition, written op by op in numpy float32 (temper below).  With (8, 8) it is fpu_reference.Search, and through it the
unmodified oracle, bit for bit on the whole tree (tests/test_policy_temp_api.py asserts it).

Beyond the parent class, the restatement here
  - has a fourth evaluator, "skewbad": "skew" whose prior row is replaced, for boards chosen by their hash, by a bad row
    of one of five kinds (a NaN, an inf, -0.1, 1.5, all zero): the rows the guard must hand on as delivered.  On the device
    the same function goes in through Engine.search_external (host_evaluator);
  - has a fifth, "skewones": "skew" whose row is ALL ONES for one board in three -- a row that passes the guard and sums
    to k, so that Z passes 2^31 on 13x13;
  - has the "skew" evaluator as a REGISTERED device evaluator too (skew_device_evaluator: torch tensors), which delivers
    prior rows in play-mode launches, where forced playouts and the Gumbel root search act; GumbelSearch composes the
    rule with gumbel_reference.Search as Search composes it with the forcing rule;
  - counts what azx_policy_temp_stats counts;
  - searches a row with a NaN or an infinite prior, which the guard hands on as delivered and the reference would have
    refused (mcts.py:211-213), as the library's search does: see fpu_pick.

Shared by tests/test_policy_temp_api.py (CPU) and tests/test_gpu_policy_temp.py; the references are computed once per
process and never changed."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpu_reference as ref  # noqa: E402
import gumbel_reference as gr  # noqa: E402
from fpu_reference import Settings, prefix_third, most_visited  # noqa: E402,F401

f32 = np.float32
TWO24 = f32(16777216.0)
INV_TWO24 = f32(1.0) / TWO24
OFF = (8, 8)
# (eighths, root_eighths): the settings the issue names
SETTINGS = ((6, 8), (4, 8), (1, 8), (8, 4), (6, 7), (3, 5))
ROW_KINDS = ("skew", "skewbad", "skewones")  # evaluators that deliver a prior ROW; the others give one table prior
ZERO_STATS = dict(tempered=0, left_as_delivered=0, root_searches=0, reserved=0)
BAD_KINDS = ("nan", "inf", "negative", "above_one", "all_zero")


def temper(P, m):
    """(row, tempered): the definition, one float32 operation at a time."""
    P = np.ascontiguousarray(P, f32)
    if m == 8:
        return P, False
    if not np.isfinite(P).all() or (P < f32(0.0)).any() or (P > f32(1.0)).any():      # the guard
        return P, False
    s1 = np.sqrt(P)
    s2 = np.sqrt(s1)
    s3 = np.sqrt(s2)
    assert s1.dtype == s2.dtype == s3.dtype == f32
    q = None
    for bit, s in ((4, s1), (2, s2), (1, s3)):
        if m & bit:
            q = s if q is None else q * s
    Z = int((q * TWO24).astype(np.uint32).sum(dtype=np.uint64))
    assert Z < 1 << 32
    if Z == 0:
        return P, False
    Zf = f32(Z) * INV_TWO24                 # (an integer below 2^32 is exact in float64: one rounding, to nearest even)
    out = q / Zf
    assert out.dtype == f32
    return out, True


def bad_row(h32, row, ones=False):
    """"skewbad": the row as delivered for a board with hash h32 -- one board in three gets a bad row.  `ones`
    ("skewones"): that row is all ones instead, which is no bad row: it is tempered."""
    if (h32 >> 5) % 3 != 0:
        return row
    row = row.copy()
    if ones:
        row[:] = 1
        return row
    kind = BAD_KINDS[(h32 >> 9) % 5]
    j = (h32 >> 13) % len(row)
    if kind == "nan":
        row[j] = np.nan
    elif kind == "inf":
        row[j] = np.inf
    elif kind == "negative":
        row[j] = f32(-0.1)
    elif kind == "above_one":
        row[j] = f32(1.5)
    else:
        row[:] = 0
    return row


def host_evaluator(kind):
    """The "skew" / "skewbad" evaluator for Engine.search_external."""
    from oracle import oracle as orc
    skew = ref.skew_host_evaluator()
    if kind == "skew":
        return skew

    def fn(boards, lm, slot, k):
        v, p = skew(boards, lm, slot, k)
        for i in range(len(k)):
            p[i, :k[i]] = bad_row(orc.fnv1a(boards[i]), p[i, :k[i]], ones=kind == "skewones")
        return v, p
    return fn


def skew_device_evaluator(device):
    """The "skew" evaluator as a registered device evaluator (Engine.set_external_evaluator; torch tensors on
    `device`): evaluate(board, legal) -> (value[n], prior[n, cells]).  The hash is fnv1a of the network-input board, the
    value (h & 0xffff) / 32768 - 1 and prior j of the k legal moves w_j / sum(w), w_j = 1 + ((h >> j) & 3): integers, one
    float64 division per child rounded to float32 once, so numpy and the device agree to the bit."""
    import torch
    p4 = pow(0x01000193, 4, 1 << 32)

    def evaluate(board, legal):
        b = board.reshape(len(board), -1).to(torch.int64)
        h = torch.full((len(b),), 0x811C9DC5, dtype=torch.int64, device=device)
        for c in range(b.shape[1]):
            h = ((h ^ b[:, c]) * p4) & 0xFFFFFFFF
        value = ((h & 0xFFFF).to(torch.float64) / 32768.0 - 1.0).to(torch.float32)
        j = torch.arange(legal.shape[1], dtype=torch.int64, device=device)[None, :]
        w = 1 + ((h[:, None] >> torch.clamp(j, max=40)) & 3)              # (h < 2^32: shifts past bit 31 give 0)
        w = torch.where(legal != 0, w, torch.zeros((), dtype=torch.int64, device=device)).to(torch.float64)
        return value, (w / w.sum(1, keepdim=True)).to(torch.float32)
    return evaluate


class TempRule:
    """The rule as a mixin in front of fpu_reference.FpuRule.  set_temp() must be called before the parent class's
    __init__ runs the first search."""

    def set_temp(self, temp=OFF, bad=False, ones=False):
        self.eighths, self.root_eighths = int(temp[0]), int(temp[1])
        self.bad, self.ones = bool(bad) or bool(ones), bool(ones)
        self.stat_tempered = self.stat_guarded = self.stat_root_searches = 0
        self._root_rows = {}

    def expand_priors(self, node, k, priors):
        if priors is not None and k:
            if self.bad:
                from oracle import oracle as orc
                priors = bad_row(orc.fnv1a(ref.mover_view(self.games[node])), priors, ones=self.ones)
            if self.eighths != 8:
                priors, done = temper(priors, self.eighths)
                self.stat_tempered += int(done)
                self.stat_guarded += int(not done)
        ref.FpuRule.expand_priors(self, node, k, priors)

    def root_row(self, P):
        """R = temper(stored priors of the root's children, root_eighths), once per root."""
        if self.root_id not in self._root_rows:
            self._root_rows[self.root_id] = temper(P, self.root_eighths)
        return self._root_rows[self.root_id]

    def fpu_pick(self, node):
        nv, tv, P = self.children(node)
        Ps = P
        if node == self.root_id and self.root_eighths != 8 and self.row_kind:
            Ps, done = self.root_row(P)
            if self.sel == 0:                                   # the first select of a search
                self.stat_root_searches += 1
                self.stat_guarded += int(not done)
        if node == self.root_id and self.noise is not None and self.eps != 0.0:
            row = self.noise[self.sel, :len(P)]
            Ps = ((self.keep32 * Ps).astype(np.float64) + self.eps * row).astype(f32)         # mcts.py:130 over R
        best, _ = ref.pick_child(self.fpu, self.nv[node], self.tv[node], nv, tv, P, Ps, self.c32, node == self.root_id)
        if node != self.root_id and not (nv != 0).any() and not np.isfinite(P).all():
            # A row the guard handed on as delivered is searched as the search has always searched it (include/azx.h):
            # below the root a node whose children have no visit yet takes its first child unscored -- every score is
            # -0 + 0 while the priors are finite -- so a NaN or an infinite prior is first scored at the node's second
            # visit.  (The reference refuses such rows, mcts.py:211-213; nothing changes for a finite row.)
            best = 0
        if self.fpu[0] != "off" and (nv == 0).any():
            self.stat_levels += 1
        return best, Ps

    def temp_stats(self):
        return dict(tempered=self.stat_tempered, left_as_delivered=self.stat_guarded,
                    root_searches=self.stat_root_searches, reserved=0)


class Search(TempRule, ref.Search):
    """One search of `prefix` on a fresh tree under `temp` = (eighths, root_eighths), beside first-play urgency `fpu`
    and the forcing rule `forced_k`.  move_and_search(child) plays a root child and searches the carried subtree."""

    def __init__(self, prefix, kind, temp=OFF, fpu=ref.OFF, **kw):
        self.row_kind = kind in ROW_KINDS
        self.set_temp(temp if self.row_kind else OFF, bad=kind == "skewbad", ones=kind == "skewones")
        ref.Search.__init__(self, prefix, "skew" if self.row_kind else kind, fpu, **kw)


class GumbelSearch(TempRule, ref.FpuRule, gr.Search):
    """gumbel_reference.Search (the Gumbel root search) over the "skew" rows under `temp`: the candidates' ln P, sigma's
    prior-weighted mean and the keys are made from the STORED, tempered priors; root_eighths is unused (the root select
    reads no prior) and not counted."""

    def __init__(self, prefix, kind, temp=OFF, fpu=ref.OFF, **kw):
        self.row_kind = kind in ROW_KINDS
        self.set_temp(temp if self.row_kind else OFF)
        self.set_rule(fpu, "skew" if self.row_kind else kind)
        gr.Search.__init__(self, prefix, "hash" if self.row_kind else kind, **kw)


@functools.lru_cache(maxsize=None)
def tree_case(n, bs, sims, kind, temp, prefix, fpu=ref.OFF, c_puct=0.5):
    """dump(), temp_stats() and stats() of one search under `temp` (and `fpu`)."""
    cfg = Settings(n=n, sims=sims, bs=bs, c_puct=c_puct, tree_cap=1 << 17)
    s = Search(prefix, kind, temp, fpu, cfg=cfg)
    return s.dump(), s.temp_stats(), s.stats()


def entropy(p):
    p = np.asarray(p, np.float64)
    p = p[p > 0]
    return float(-(p * np.log(p)).sum())
