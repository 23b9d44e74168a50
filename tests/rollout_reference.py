"""The rollout evaluator's definition (include/azx.h, "Rollout evaluator") restated in pure Python: integers only, a
stack flood fill.  Written from the text of the definition, not from the C.  Also the exact win probability of a
position by enumerating every fill, and the positions the CPU and GPU tests share."""
import itertools
import struct

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def sm(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def lb(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def position_key(seed, board):
    h = sm(seed & M64)
    for c, v in enumerate(board):
        if v:
            h ^= sm((seed + 4 * c + v) & M64)
    return h


def neighbours(c, N):
    i, j = divmod(c, N)
    for a, b in ((i - 1, j), (i - 1, j + 1), (i, j - 1), (i, j + 1), (i + 1, j - 1), (i + 1, j)):
        if 0 <= a < N and 0 <= b < N:
            yield a * N + b


def one_connects(full, N):
    """Colour 1 connects row 0 to row N-1 on the full board."""
    stack = [c for c in range(N) if full[c] == 1]
    seen = set(stack)
    while stack:
        c = stack.pop()
        if c // N == N - 1:
            return True
        for d in neighbours(c, N):
            if full[d] == 1 and d not in seen:
                seen.add(d)
                stack.append(d)
    return False


def two_connects(full, N):
    """Colour 2 connects column 0 to column N-1 on the full board."""
    stack = [i * N for i in range(N) if full[i * N] == 2]
    seen = set(stack)
    while stack:
        c = stack.pop()
        if c % N == N - 1:
            return True
        for d in neighbours(c, N):
            if full[d] == 2 and d not in seen:
                seen.add(d)
                stack.append(d)
    return False


def fill(seed, N, board, r, key=None):
    """The filled board of rollout r."""
    board = [int(v) for v in np.asarray(board).ravel()]
    H = position_key(seed, board) if key is None else key
    k = lb((H & M32) ^ lb(((H >> 32) + r) & M32))
    empties = [c for c, v in enumerate(board) if v == 0]
    need, rem = (len(empties) + 1) >> 1, len(empties)
    full = list(board)
    for c in empties:
        w = lb((k + c * 0x9E3779B9) & M32)
        if ((w * rem) >> 32) < need:
            full[c] = 1
            need -= 1
        else:
            full[c] = 2
        rem -= 1
    assert need == 0 and rem == 0
    return full


def rollout_wins(seed, N, board, R):
    board = [int(v) for v in np.asarray(board).ravel()]
    assert len(board) == N * N
    H = position_key(seed, board)
    return sum(one_connects(fill(seed, N, board, r, key=H), N) for r in range(R))


def value_bits(wins, R):
    """The bits of (float)(2*wins - R) / (float)R: the quotient of two exactly representable integers, rounded once."""
    return struct.unpack("<I", struct.pack("<f", np.float32(2 * wins - R) / np.float32(R)))[0]


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def exact_win_probability(N, board):
    """The mover's win probability under a uniformly random fill, by enumeration (small boards only)."""
    board = [int(v) for v in np.asarray(board).ravel()]
    empties = [c for c, v in enumerate(board) if v == 0]
    need = (len(empties) + 1) >> 1
    won = total = 0
    for sub in itertools.combinations(empties, need):
        full = [2 if v == 0 else v for v in board]
        for c in sub:
            full[c] = 1
        won += one_connects(full, N)
        total += 1
    return won / total


# ---- shared positions ------------------------------------------------------------------------------------------
def random_position(rng, N, empties):
    """N x N position with `empties` empty cells, the stones dealt alternately over a random cell order."""
    cells = N * N
    b = np.zeros(cells, np.int32)
    order = rng.permutation(cells)[:cells - empties]
    b[order[0::2]] = 1
    b[order[1::2]] = 2
    return b


def position_family(N, seed=7):
    """Random positions with e = 1, small, odd, even, and all-empty."""
    rng = np.random.RandomState(seed + N)
    cells = N * N
    es = sorted({1, min(3, cells), min(cells, 4 if cells > 4 else 2), cells // 2 | 1, (cells // 2) & ~1 or 2, cells - 1, cells})
    return [(e, random_position(rng, N, e)) for e in es if 1 <= e <= cells]


def small_family():
    """The empty 3x3 and 4x4 boards and twelve random 3x3 / 4x4 positions with 4 to 14 empty cells, for the
    unbiasedness test (exact probabilities by enumeration)."""
    rng = np.random.RandomState(1)
    out = [(3, np.zeros(9, np.int32)), (4, np.zeros(16, np.int32))]
    for N, lo, hi in ((3, 4, 8), (4, 4, 14)):
        for _ in range(6):
            out.append((N, random_position(rng, N, int(rng.randint(lo, hi + 1)))))
    return out


def spiral_board(N):
    """A full board whose only colour-1 path from row 0 to row N-1 winds in a rectangular spiral: the flood fill needs
    many more steps than N.  Colour 1 runs along a spiral of rows and columns two apart; the rest is colour 2."""
    g = np.full((N, N), 2, np.int32)
    top, left, bottom, right = 0, 0, N - 1, N - 1
    i, j = 0, 0
    g[0, 0] = 1
    # walk right, down, left, up with shrinking bounds, leaving a colour-2 lane between the turns
    while True:
        moved = False
        while j < right:
            j += 1; g[i, j] = 1; moved = True
        top += 2
        if not moved or top > bottom:
            break
        moved = False
        while i < bottom:
            i += 1; g[i, j] = 1; moved = True
        right -= 2
        if not moved or left > right:
            break
        moved = False
        while j > left:
            j -= 1; g[i, j] = 1; moved = True
        bottom -= 2
        if not moved or top > bottom:
            break
        moved = False
        while i > top:
            i -= 1; g[i, j] = 1; moved = True
        left += 2
        if not moved or left > right:
            break
    return g.ravel()


def wrapping_connects(full, N):
    """one_connects with the four wrapped steps allowed as well (c + 1 from column N-1, c + N - 1 from column 0 and
    their mirror images): what a shifted-mask flood fill computes when it forgets to clear the column-wrap bits."""
    cells = N * N
    stack = [c for c in range(N) if full[c] == 1]
    seen = set(stack)
    while stack:
        c = stack.pop()
        if c // N == N - 1:
            return True
        for d in (c - N, c - N + 1, c - 1, c + 1, c + N - 1, c + N):
            if 0 <= d < cells and full[d] == 1 and d not in seen:
                seen.add(d)
                stack.append(d)
    return False


def wrap_boards(N):
    """Full boards whose only colour-1 "connection" runs through a wrapped neighbour, so colour 1 must lose each.  The
    two wrapped pairs are (i, N-1) ~ (i+1, 0), which is c + 1 from column N-1 or c - 1 from column 0, and (i, 0) ~
    (i, N-1), which is c + N - 1 from column 0 or c - N + 1 from column N-1; one board per pair and direction."""
    out = []
    if N < 4:
        return out
    mid = N // 2
    g = np.full((N, N), 2, np.int32)        # c + 1 from column N-1: down column N-1, on from (mid, 0) down column 0
    g[:mid, N - 1] = 1
    g[mid:, 0] = 1
    out.append(g.ravel().copy())
    g = np.full((N, N), 2, np.int32)        # c + N - 1 from column 0: down column 0 to row mid, on down column N-1
    g[:mid + 1, 0] = 1
    g[mid:, N - 1] = 1
    out.append(g.ravel().copy())
    g = np.full((N, N), 2, np.int32)        # c - 1 from column 0: (mid, 0) -> (mid-1, N-1), on down column N-2
    g[:mid + 1, 0] = 1
    g[mid - 1, N - 1] = 1
    g[mid:, N - 2] = 1
    out.append(g.ravel().copy())
    if N >= 5:
        g = np.full((N, N), 2, np.int32)    # c - N + 1 from column N-1: (mid, N-1) -> (mid, 0), on down column 1
        g[:mid + 1, N - 2] = 1
        g[mid, N - 1] = 1
        g[mid, 0] = 1
        g[mid:, 1] = 1
        out.append(g.ravel().copy())
    return out


def two_wins_boards(N):
    """Full boards where colour 2 has its own win (a row of colour 2, straight and as a staircase)."""
    g = np.full((N, N), 1, np.int32)
    g[N // 2, :] = 2
    out = [g.ravel().copy()]
    g = np.full((N, N), 1, np.int32)
    i = N - 1
    for j in range(N):          # (i, j) -> (i-1, j+1) is a neighbour: a rising diagonal, doubled where it steps
        g[i, j] = 2
        if j % 2 == 1 and i > 0:
            i -= 1
            g[i, j] = 2
    out.append(g.ravel().copy())
    return out


def full_boards(N):
    """[(name, board, colour 1 wins)] hand-built full boards."""
    out = []
    if N >= 5:
        s = spiral_board(N)
        out.append(("spiral", s, one_connects(list(s), N)))
    for i, b in enumerate(wrap_boards(N)):
        out.append(("wrap%d" % i, b, False))
    for i, b in enumerate(two_wins_boards(N)):
        out.append(("two%d" % i, b, False))
    return out
