"""Evaluator outputs at the edges of what the ABI accepts (no test in this module; tests/test_evaluator_edge_cases.py
checks it on the CPU, tests/test_gpu_evaluator_edges.py runs the engine against it).

azx_put_evals and the device hand-over take any finite value and any prior row with p >= 0 and |sum - 1| < 1e-4.  The
evaluator here is a pure function of (board row, legal list, dirty), keyed on a CRC of the board, so that the oracle
(orc.CallbackEval), the host phase API (Engine.search_external) and the device hand-over (Engine.set_external_evaluator)
see the same outputs for the same row:

  value   a multiple of 2^-15 in [-1, 1); in a dirty game about one row in four takes a value from a fixed list instead:
          "out"      OUT_OF_RANGE: values outside the range value_in_fast_range (mcts_kernels.hip) keeps a game on the
                     unscaled divide for -- denormals, tiny normals, the neighbours of both bounds, 3e35;
          "edge-in"  EDGE_IN: exactly the bounds, +-2^-60 and +-1e30, which are inside: the flag must stay clear;
          "negzero"  -0.0 in place of every second value (inside the range as well).
  prior   uniform over the legal moves; about one row in three has every second legal entry exactly 0, about one in seven
          is one-hot.  Every row is w / sum(w) in float64 with w in {0, 1}, rounded once to float32.
"""
import functools
import zlib
from fractions import Fraction

import numpy as np

F32 = np.float32
LO = F32(2.0 ** -60)                  # value_in_fast_range: v == 0 or LO <= |v| <= HI
HI = F32(1.0e30)
OUT_OF_RANGE = np.array([1e-40, -1e-40, 1.4e-45, 1e-30, -3e-25, 2.0 ** -61,
                         np.nextafter(LO, F32(0)), -np.nextafter(HI, F32(np.inf)), 3e35], F32)
EDGE_IN = np.array([LO, -LO, HI, -HI], F32)
VALUE_CLASSES = ("out", "edge-in", "negzero")
SIMS, ROUNDS, C_PUCT = 60, 4, 0.5


def in_fast_range(v):
    """value_in_fast_range of mcts_kernels.hip, elementwise on float32."""
    a = np.abs(np.asarray(v, F32))
    return (a == 0) | ((a >= LO) & (a <= HI))


def _value(h, dirty, value_class):
    base = F32((h & 0xFFFF) / 32768.0 - 1.0)
    if not dirty:
        return base
    if value_class == "negzero":
        return F32(-0.0) if (h >> 16) & 1 else base
    if (h >> 16) & 3:
        return base
    table = OUT_OF_RANGE if value_class == "out" else EDGE_IN
    return table[(h >> 18) % len(table)]


def _prior(h, k, K):
    w = np.zeros(K, np.float64)
    t = h % 21
    if t < 3:                                       # one row in seven: one-hot
        w[(h >> 8) % k] = 1.0
    elif t < 10:                                    # one row in three: every second legal entry exactly 0
        w[(h >> 8) & 1:k:2] = 1.0
        if not w.any():                             # (k == 1 and the odd phase)
            w[0] = 1.0
    else:
        w[:k] = 1.0
    return (w / w.sum()).astype(F32)


def evaluate(boards, legal, dirty, value_class="out"):
    """(value[B], prior[B, K]) for boards int32 [B, n, n] and legal int32 [B, K] (tile + 1, 0-padded) as every evaluator
    of the engine and of the oracle receives them; dirty: one bool, or one per row."""
    assert value_class in VALUE_CLASSES
    boards = np.ascontiguousarray(boards, np.int32)
    legal = np.asarray(legal)
    B, K = legal.shape
    dirty = np.broadcast_to(np.asarray(dirty, bool), (B,))
    value = np.zeros(B, F32)
    prior = np.zeros((B, K), F32)
    for i in range(B):
        raw = boards[i].tobytes()
        k = int(np.count_nonzero(legal[i]))
        assert k > 0 and legal[i, :k].all()
        value[i] = _value(zlib.crc32(raw), bool(dirty[i]), value_class)
        prior[i] = _prior(zlib.crc32(raw, 0x9E3779B9), k, K)
    return value, prior


def pool_size(n):
    return 8 if n >= 13 else 12


def is_dirty(slot):
    return np.asarray(slot) % 2 == 0


@functools.lru_cache(maxsize=None)
def prefixes(n):
    """pool_size(n) random non-terminal prefixes of 0 .. n^2 / 3 stones (tile + 1), both colours to move among the dirty
    (even) slots and among the clean ones; slots 0 and 2 start from 0 and 1 stones, the widest roots."""
    from oracle import oracle as orc
    G = pool_size(n)
    rng = np.random.RandomState(1000 + n)
    lens = rng.randint(0, n * n // 3 + 1, G)
    lens[0], lens[2] = 0, min(1, n * n // 3)
    out = []
    for g in range(G):
        h, mv = orc.Hex(n), []
        while len(mv) < lens[g]:
            lm = h.legal_moves()
            m = int(lm[rng.randint(len(lm))])
            h2 = h.copy()
            h2.step(m)
            if h2.result:
                continue
            h, mv = h2, mv + [m]
        out.append(tuple(mv))
    return tuple(out)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def canonical(d):
    """tests/test_gpu_tree_parity.py's canonical(): a six-array tree relabelled breadth-first from its root."""
    order = [d["root_id"]]
    i = 0
    while i < len(order):
        v = order[i]
        i += 1
        if d["num_children"][v] > 0:
            fc = d["first_child"][v]
            order.extend(range(fc, fc + d["num_children"][v]))
    order = np.array(order)
    return (d["num_children"][order], bits(d["num_visits"][order]), bits(d["total_value"][order]),
            bits(d["prior_prob"][order]))


class OracleRun:
    """What the oracle did with one pool: per round r and game g, rounds[r][g] = dict(canon, visits, num_nodes, k_root,
    root_prior, total_value, values (what its evaluator returned during that search), zero_prior (per returned row),
    move, board, result (both after the move))."""

    def __init__(self, n, value_class, batch):
        from oracle import oracle as orc
        self.n, self.value_class, self.batch = n, value_class, batch
        self.prefixes = prefixes(n)
        G = self.G = len(self.prefixes)
        self.dirty = is_dirty(np.arange(G))
        games, trees, evals, seen = [], [], [], [[] for _ in range(G)]
        for g in range(G):
            h = orc.Hex(n)
            for m in self.prefixes[g]:
                h.step(m)
            assert not h.result
            games.append(h)
            trees.append(orc.Tree(1 << 17))

            def fn(boards, lm, g=g):
                v, p = evaluate(boards, lm, self.dirty[g], value_class)
                k = np.count_nonzero(lm, axis=1)
                seen[g].append((v.copy(), np.array([(p[i, :k[i]] == 0).any() for i in range(len(k))])))
                return v, p
            evals.append(orc.CallbackEval(fn))
        self.colors = [h.color for h in games]
        self.rounds = []
        for rnd in range(ROUNDS):
            row = []
            for g in range(G):
                assert not games[g].result, "game %d ended before search %d" % (g, rnd)
                seen[g].clear()
                st = orc.search(trees[g], games[g], evals[g], SIMS, batch, C_PUCT)
                assert st.status == 0
                d = trees[g].dump()
                nv, _, pp = trees[g].root_stats()[:3]
                mid = int(np.argmax(nv))
                lm = games[g].legal_moves()
                rec = dict(canon=canonical(d), visits=nv.copy(), num_nodes=trees[g].num_nodes, k_root=len(nv),
                           root_prior=pp.copy(), total_value=d["total_value"].copy(),
                           values=np.concatenate([s[0] for s in seen[g]]) if seen[g] else np.zeros(0, F32),
                           zero_prior=np.concatenate([s[1] for s in seen[g]]) if seen[g] else np.zeros(0, bool),
                           move=mid)
                trees[g].move(mid)
                games[g].step(int(lm[mid]))
                rec["board"], rec["result"] = games[g].board, games[g].result
                row.append(rec)
            self.rounds.append(row)

    def flags(self, rnd):
        """bool [G]: the game has received a value outside the fast range in searches 0 .. rnd."""
        return np.array([any((~in_fast_range(self.rounds[r][g]["values"])).any() for r in range(rnd + 1))
                         for g in range(self.G)])


@functools.lru_cache(maxsize=None)
def oracle_run(n, value_class="out", batch=10):
    """The oracle's four searches + moves of the pool, computed once per process and shared (read-only)."""
    return OracleRun(n, value_class, batch)


# ---- div2_unscaled (mcts_kernels.hip) in exact rational arithmetic ----------------------------------------------------
def round_f32(x):
    """The float32 nearest to the Fraction x (ties to even, gradual underflow), as a Fraction."""
    if x == 0:
        return Fraction(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                       # 2^e <= a < 2^(e+1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    q = a / quantum
    fl = q.numerator // q.denominator
    rem = q - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    r = fl * quantum
    assert r < Fraction(2) ** 128
    return r if x > 0 else -r


def ulp_f32(x):
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    return Fraction(2) ** (max(e, -126) - 23)


def div_unscaled_exact(n, d, rcp_ulps=0):
    """div2_unscaled's chain on Fractions n, d (float32 values): every fma rounded once, denormal intermediates kept;
    rcp = the correctly rounded 1/d moved by rcp_ulps units in its last place (v_rcp_f32 is good to one)."""
    fma = lambda a, b, c: round_f32(a * b + c)      # noqa: E731
    r = round_f32(1 / d)
    r += rcp_ulps * ulp_f32(r)
    e = fma(-d, r, Fraction(1))
    r = fma(e, r, r)
    q = round_f32(n * r)
    e = fma(-d, q, n)
    q = fma(e, r, q)
    e = fma(-d, q, n)
    return fma(e, r, q)


def guard_divide_cases(count, seed=3):
    """{class: (num float32[count], den float32[count])}: the numerators value_in_fast_range admits beyond the +-2000 of
    tests/test_gpu_tree_parity.py -- total_value sums are multiples of 2^-83 (2^-60 with a 24-bit mantissa) and reach
    2^24 backups of 1e30 -- over the denominators 1 .. 4096 and random integers up to 2^24."""
    rng = np.random.RandomState(seed)
    den = np.where(np.arange(count) % 2 == 0, 1 + np.arange(count) % 4096, rng.randint(1, (1 << 24) + 1, count))
    den = den.astype(F32)
    m = rng.permutation(1 + np.arange(count) % 4096).astype(np.float64) * rng.choice([-1.0, 1.0], count)
    small = np.exp2(rng.uniform(-83, -60, count)).astype(F32).clip(F32(2.0 ** -83), LO)
    big = np.exp(rng.uniform(np.log(1e30), np.log(1.7e37), count)).astype(F32).clip(HI, F32(1.7e37))
    return {"multiples of 2^-83": (np.ldexp(m, -83).astype(F32), den),
            "2^-83 .. 2^-60": (small * rng.choice([-1.0, 1.0], count).astype(F32), den),
            "1e30 .. 1.7e37": (big * rng.choice([-1.0, 1.0], count).astype(F32), den)}
