"""Gumbel root search with sequential halving (include/azx.h, "Gumbel root search with sequential halving") restated on
the CPU: tests/forced_playouts_reference.py's Search -- the numpy float32 restatement of the oracle's search, bit-equal
to the unmodified oracle with no rule set -- with the Gumbel rule as a parameter.  The same Settings, evaluators
("uniform", "hash") and 5x5 positions; positions of tests/option_positions.py for other boards.

Noise comes from engine.gumbel_variate (a host function: no GPU).  Keys and the softmax are computed in float64 from the
float32 n, w, P of the tree.  Every decision -- a cut between kept and dropped children, or the final pick -- records
whether it is SAFE: every straddling pair has |delta key| > MARGIN, or identical (g, P, n, w) (an exact tie on both
sides, which the index breaks).  A position whose decisions are all safe is compared exactly with the device; the others
are left out, and at most MAX_UNSAFE_SHARE of any case's positions may be.

MARGIN = 1e-3: keys stay below 1000 in these setups, so float32 spacing is at most 6.1e-5, and a key is three rounded
sums and two logarithms -- a few times 1e-4 at worst, under 2e-4 at the 5x5 setup.

Shared by tests/test_gumbel_api.py (CPU) and tests/test_gpu_gumbel.py; the references are computed once per process and
never changed."""
import dataclasses
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
_lib.lib().azx_gumbel_variate, _lib.lib().azx_set_gumbel

import forced_playouts_reference as fp  # noqa: E402
from early_stop_reference import DEFAULT, Settings, game_at  # noqa: E402,F401

f32 = np.float32
MARGIN = 1e-3
MAX_UNSAFE_SHARE = 0.10
SEED = 4242                             # the engines' seed in tests/test_gpu_gumbel.py
KINDS = fp.KINDS


@dataclasses.dataclass(frozen=True)
class Setup:
    """One parametrised case: the search Settings, the option's values, whether the ply is greedy (g = 0), and which
    positions."""
    name: str
    cfg: Settings
    m: int
    c_visit: float = 50.0
    c_scale: float = 1.0
    greedy: bool = False
    family: str = "5x5"                 # "5x5": fp.prefixes(kind); "late": those with k < m; "9" / "13": option_positions
    kinds: tuple = KINDS                # the evaluators the case runs with

    @property
    def nbt(self):
        return self.cfg.nb


def _small(n):
    return Settings(n=n, sims=60, bs=10, c_puct=0.5, tree_cap=1 << 17)


SETUPS = (
    Setup("m8_200", DEFAULT, 8),                                             # NBt 21, R 3: halvings at b = 7 and 14
    Setup("m16_20", Settings(n=5, sims=20, bs=10, c_puct=0.5), 16),          # NBt 3, R 4: a halving at b = 0
    Setup("m16_late", DEFAULT, 16, family="late"),                           # k < m
    # exploration_depth = 0: g = 0.  ("uniform" is left out: with g = 0, one prior and value 0 nearly every key ties
    # EXACTLY between children whose visit counts differ, which the safe-decision rule does not admit.)
    Setup("m8_greedy", DEFAULT, 8, greedy=True, kinds=("hash",)),
    # "uniform" on these boards is what runs k_mcts<2, FAST> / k_play<2> with two live register slots and the <3, ...>
    # instantiations with three ("hash" runs the generic kernel whatever the path)
    Setup("m16_9x9", _small(9), 16, family="9"),                             # two register slots
    Setup("m16_13x13", _small(13), 16, family="13"),                         # three, k > 128
)
SETUP = {s.name: s for s in SETUPS}
CASES = tuple((s.name, kind) for s in SETUPS for kind in s.kinds)
# Non-uniform priors through a registered external evaluator: value 0 and, for the legal cell in row i, column j, the
# prior w / sum(w) with w = 2^-(1 + (i - j) mod 4) -- weights and sum exact, one float64 division rounded to float32, so
# numpy and the device agree to the bit; the same in the first player's view and the mover's (the perspective flip
# keeps i - j).  With the stub
# evaluators every child of a node has one prior, so ln P cancels in the improved row; here it does not.
POW2 = Setup("m8_pow2", DEFAULT, 8, kinds=("pow2",))
SETUP[POW2.name] = POW2
# The same with exact zeros among the priors ("pow2z": w = 0 where (i - j) mod 4 == 3): ln P = -inf for those children, in
# the candidates' keys, in sigma's prior-weighted mean and in the improved row.  m = 8 on the 5x5 positions, and m = 16 on
# the positions with fewer than min(16, k) children of nonzero prior, where zero-prior children must become candidates.
POW2Z = (Setup("m8_pow2z", DEFAULT, 8, kinds=("pow2z",)), Setup("m16_pow2z", DEFAULT, 16, family="few", kinds=("pow2z",)))
SETUP.update({s.name: s for s in POW2Z})
POW2Z_MAX_PLIES = 10                    # prefixes this short keep a legal cell of nonzero weight at every expanded node


def philox_block(k0, k1, counter):
    """Philox4x32-10 of one counter (four words) under the key (k0, k1): four uint64 arrays holding 32-bit words."""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, np.uint64) for x in counter]
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & M, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def philox_words(seed, uid, ply, children):
    """The raw 32-bit words of rule 1 for an array of child indices: Philox4x32-10 under the game's key
    (seed + uid; the second key word xor 0x5bd1e995) at the counter (0x47554D42, ply, child >> 2, 0x4E4F4953), word
    child & 3.  A numpy restatement, independent of the library."""
    children = np.asarray(children, np.uint64)
    s = (int(seed) + int(uid)) & 0xFFFFFFFFFFFFFFFF
    c = philox_block(s & 0xFFFFFFFF, ((s >> 32) ^ 0x5bd1e995) & 0xFFFFFFFF,
                     [np.full(children.shape, 0x47554D42, np.uint64), np.full(children.shape, int(ply), np.uint64),
                      children >> np.uint64(2), np.full(children.shape, 0x4E4F4953, np.uint64)])
    words = np.stack(c, -1)
    return np.take_along_axis(words, (children & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0].astype(np.uint32)


def gumbel_of_words(words):
    """g = -ln(-ln u), u = ((word >> 8) + 1/2) / 2^24, in float64."""
    u = ((np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) / 16777216.0
    return -np.log(-np.log(u))


def variates(seed, uid, ply, k, greedy):
    from azalea_amd import engine as eng
    if greedy:
        return np.zeros(k)
    return np.array([eng.gumbel_variate(seed, uid, ply, j) for j in range(k)])


def sigma_of(n, w, P, c_visit, c_scale):
    """sigma_j in float64 from the float32 n, w, P: ((c_visit + n_max) * c_scale) * qh_j."""
    n, w, P = (np.asarray(a, np.float64) for a in (n, w, P))
    vis = n > 0
    qh = np.full(len(n), 0.5)
    qh[vis] = 0.5 * ((-w[vis]) / n[vis]) + 0.5
    vh = float((P[vis] * qh[vis]).sum() / P[vis].sum()) if vis.any() else 0.5
    qh[~vis] = vh
    return ((c_visit + (n.max() if len(n) else 0.0)) * c_scale) * qh


def top(keys, members, count):
    """The `count` members with the largest keys, ties to the lower index: (kept, dropped), index arrays."""
    members = np.asarray(members, np.int64)
    order = members[np.lexsort((members, -keys[members]))]
    return np.sort(order[:count]), np.sort(order[count:])


def safe_cut(keys, kept, dropped, ident):
    """Whether every (kept, dropped) pair is MARGIN apart in key, or identical in (g, P, n, w)."""
    for i in kept:
        for j in dropped:
            if keys[i] == keys[j] == -np.inf:                   # two zero priors: ln 0 is -inf in any precision, an exact
                continue                                        # tie on both sides, which the index breaks
            if abs(keys[i] - keys[j]) <= MARGIN and ident[i] != ident[j]:
                return False
    return True


def pow2_prior(tiles, n):
    """float32 w / sum(w), w = 2^-(1 + (i - j) mod 4) for the legal cells tile - 1 = i * n + j: the weights and their sum
    are exact, the one division is made in float64 and rounded to float32 once."""
    t = np.asarray(tiles, np.int64) - 1
    w = np.ldexp(np.float64(1.0), -(1 + ((t // n - t % n) % 4)))
    return (w / w.sum()).astype(f32)


def pow2z_prior(tiles, n):
    """pow2_prior with w = 0 where (i - j) mod 4 == 3: exact zeros among the priors.  Defined only while some legal cell
    has a nonzero weight."""
    t = np.asarray(tiles, np.int64) - 1
    d = (t // n - t % n) % 4
    w = np.where(d == 3, 0.0, np.ldexp(np.float64(1.0), -(1 + d)))
    assert w.sum() > 0, tiles
    return (w / w.sum()).astype(f32)


PRIORS = {"pow2": pow2_prior, "pow2z": pow2z_prior}


def pow2z_device_evaluator(n, device):
    """The "pow2z" stub as a registered external evaluator (torch tensors on `device`): value 0, prior pow2z_prior of the
    row's legal cells.  pow2z_prior is defined only while some legal cell has a nonzero weight, which holds at every node
    the restatement expands; the GPU tests then play the games to their ends for the harvest, and a late row without such
    a cell gets the uniform row here."""
    import torch

    def evaluate(board, legal):
        t = legal.to(torch.int64) - 1
        d = torch.remainder(torch.div(t, n, rounding_mode="floor") - torch.remainder(t, n), 4)
        one = torch.ones((), dtype=torch.float64, device=device)
        zero = torch.zeros((), dtype=torch.float64, device=device)
        w = torch.where((legal != 0) & (d != 3), torch.ldexp(one, -(1 + d)), zero)
        w = torch.where(w.sum(1, keepdim=True) > 0, w, torch.where(legal != 0, one, zero))
        return torch.zeros(len(board), dtype=torch.float32, device=device), (w / w.sum(1, keepdim=True)).to(torch.float32)
    return evaluate


class Search(fp.Search):
    """fp.Search with the Gumbel rule: m = 0 is the parent class's search (no rule; forced_k: its forcing rule).  kinds
    "pow2" / "pow2z": value 0 and pow2_prior / pow2z_prior in place of the 1/k table."""

    def __init__(self, prefix, kind, m=0, c_visit=50.0, c_scale=1.0, seed=SEED, uid=0, greedy=False, cfg=DEFAULT,
                 sims=None, bs=None, forced_k=0.0):
        self.m, self.c_visit, self.c_scale = int(m), float(c_visit), float(c_scale)
        self.seed, self.uid, self.ply, self.greedy = seed, uid, len(prefix), greedy
        self.nbt = (cfg.sims if sims is None else sims) // (cfg.bs if bs is None else bs) + 1
        self.b = 0
        self.halvings = self.root_selects = 0
        self.root_picks = []                                    # the child every root select descended into
        self.survivor_sets = []                                 # S after the candidates and after each halving
        self.safe = True
        self.pow2, self.board_n = PRIORS.get(kind), cfg.n
        assert not (m and forced_k)
        super().__init__(prefix, "uniform" if self.pow2 else kind, forced_k, sims=sims, bs=bs, cfg=cfg)
        if self.m:
            self.finish()

    def expand(self, node, k):
        first = self.num_nodes
        super().expand(node, k)
        if self.pow2 and k:
            self.pp[first:first + k] = self.pow2(self.moves[node], self.board_n)

    def root(self):
        sl = slice(self.first[0], self.first[0] + self.nch[0])
        return self.nv[sl], self.tv[sl], self.pp[sl]

    def ident(self, n, w, P):
        return [(float(self.g[j]), float(P[j]), float(n[j]), float(w[j])) for j in range(len(n))]

    def boundary(self):
        n, w, P = self.root()
        k = len(n)
        b = self.b
        if b == 0:
            self.g = variates(self.seed, self.uid, self.ply, k, self.greedy)
            with np.errstate(divide="ignore"):
                self.lnp = np.log(P.astype(np.float64))
            self.a = self.g + self.lnp
            self.m0 = min(self.m, k)
            self.R = max(1, int(np.ceil(np.log2(self.m0)))) if self.m0 > 1 else 1
            kept, dropped = top(self.a, np.arange(k), self.m0)
            self.safe &= safe_cut(self.a, kept, dropped, self.ident(n, w, P))
            self.candidates = self.S = kept
            self.survivor_sets.append(kept)
        for r in range(1, self.R):
            if (r * self.nbt) // self.R == b:
                keys = self.a + sigma_of(n, w, P, self.c_visit, self.c_scale)
                kept, dropped = top(keys, self.S, (len(self.S) + 1) // 2)
                self.safe &= safe_cut(keys, kept, dropped, self.ident(n, w, P))
                self.S = kept
                self.survivor_sets.append(kept)
                self.halvings += 1

    def batch(self, bs):
        if self.m:
            self.boundary()
        super().batch(bs)
        self.b += 1

    def pick(self, node):
        if node != 0 or not self.m:
            return super().pick(node)
        n, _, _ = self.root()
        S = self.S
        best = int(S[np.argmin(n[S])])                          # np.argmin: the first minimum, S is ascending
        self.root_selects += 1
        self.root_picks.append(best)
        return best

    def finish(self):
        n, w, P = self.n, self.w, self.p
        sig = sigma_of(n, w, P, self.c_visit, self.c_scale)
        keys = self.a + sig
        kept, dropped = top(keys, self.S, 1)
        self.safe &= safe_cut(keys, kept, dropped, self.ident(n, w, P))
        self.move = int(kept[0])
        self.survivors = self.S
        x = self.lnp + sig
        e = np.exp(x - x.max())
        self.pi = e / e.sum()


def prefixes_of(setup, kind):
    if kind == "pow2":
        return fp.prefixes("uniform")[:40]
    if kind == "pow2z":
        out = tuple(p for p in fp.prefixes("uniform") if len(p) <= POW2Z_MAX_PLIES)
        if setup.family == "few":
            out = tuple(p for p in out if nonzero_pow2z(p) < min(setup.m, DEFAULT.cells - len(p)))
        assert len(out) >= 8
        return out
    if setup.family == "5x5":
        return fp.prefixes(kind)
    if setup.family == "late":
        out = tuple(p for p in fp.prefixes(kind) if DEFAULT.cells - len(p) < setup.m)
        assert out
        return out
    import option_positions as op
    n = int(setup.family)
    more = ()
    if n == 9:                                                  # more positions than option_positions has for the board,
        rng = np.random.RandomState(7000 + n)                   # all with k > 64: two live register slots
        more = tuple(op.random_prefix(rng, setup.cfg, plies) for plies in (1, 3, 5, 7, 8, 9, 10, 12, 14))
    return tuple(op.sweep_prefixes(n)) + tuple(op.wide_hash_prefixes(n)) + more


def nonzero_pow2z(prefix):
    """The number of root children of `prefix` (default 5x5 setup) whose pow2z prior is not zero."""
    return int(np.count_nonzero(pow2z_prior(game_at(prefix, DEFAULT).legal_moves(), DEFAULT.n)))


@functools.lru_cache(maxsize=None)
def forced_positions_pow2z(k=fp.K_FORCED):
    """fp.position()'s dicts (without the rule-off root) for the forcing rule under the pow2z priors, on the "m8_pow2z"
    prefixes."""
    out = []
    for prefix in prefixes_of(SETUP["m8_pow2z"], "pow2z"):
        on = Search(prefix, "pow2z", forced_k=k)
        r = fp.prune(on.n, on.w, on.p, k, DEFAULT.c_puct)
        out.append(dict(prefix=list(prefix), n=on.n, w=on.w, p=on.p, forced=on.forced, overrode=on.overrode,
                        forced_at=tuple(on.forced_at), r=r, removed=int((on.n - r).sum())))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def positions(name, kind):
    """One dict per position of the case: an engine with seed SEED and one slot per prefix, reset once to the prefixes,
    plays prefix g as game uid G + g (azx_create used up the slots' first generation)."""
    s = SETUP[name]
    out = []
    prefixes = prefixes_of(s, kind)
    for uid, prefix in enumerate(prefixes, len(prefixes)):
        r = Search(prefix, kind, s.m, s.c_visit, s.c_scale, SEED, uid, s.greedy, cfg=s.cfg)
        out.append(dict(prefix=list(prefix), uid=uid, k=len(r.n), n=r.n, w=r.w, p=r.p, g=r.g, candidates=r.candidates,
                        survivor_sets=tuple(r.survivor_sets), survivors=r.survivors, move=r.move, pi=r.pi,
                        halvings=r.halvings, root_selects=r.root_selects, root_picks=tuple(r.root_picks),
                        safe=bool(r.safe), m0=r.m0, R=r.R))
    return tuple(out)


def mask_words(indices):
    """uint64[3]: bit c & 63 of word c >> 6 for every child index c (azx_gumbel_state's layout)."""
    out = [0, 0, 0]
    for c in indices:
        out[int(c) >> 6] |= 1 << (int(c) & 63)
    return np.array(out, np.uint64)
