"""Opening books of device matches and tournaments, as far as they can be held without a GPU: the C ABI's three entry
points (declared, bound, the argument checks that come before any device work), azx_openings_check against the host
rules (azalea_amd.game.hex.HexGame), engine.all_openings, and the Player's refusal.  The games themselves are
tests/test_gpu_match_openings.py's."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from option_api_stubs import _Agent, _cpu_policy, no_engines  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("azx_openings_check", "azx_match_set_openings", "azx_tournament_set_openings")
EINVAL = -1
_i16p, _i32p = C.POINTER(C.c_int16), C.POINTER(C.c_int32)


def header():
    return open(os.path.join(ROOT, "include", "azx.h")).read()


def L():
    from azalea_amd import _lib
    return _lib.lib()


def table(openings, stride=None):
    """(n, stride, moves int16[n, stride], lengths int32[n]) of a list of move lists."""
    n = len(openings)
    stride = max([1] + [len(o) for o in openings]) if stride is None else stride
    mv = np.zeros((max(n, 1), max(stride, 1)), np.int16)
    ln = np.zeros(max(n, 1), np.int32)
    for i, o in enumerate(openings):
        mv[i, :min(len(o), stride)] = o[:stride]
        ln[i] = len(o)
    return n, stride, mv, ln


def check(board_size, openings, stride=None):
    """(return code, bad_opening, bad_ply, message) of azx_openings_check; the out-parameters start at -7."""
    n, stride, mv, ln = table(openings, stride)
    bo, bp = C.c_int32(-7), C.c_int32(-7)
    rc = L().azx_openings_check(board_size, n, stride, mv.ctypes.data_as(_i16p), ln.ctypes.data_as(_i32p),
                                C.byref(bo), C.byref(bp))
    return rc, bo.value, bp.value, L().azx_last_error().decode()


def test_the_header_declares_the_three_symbols_and_the_binding_requires_them():
    from azalea_amd import _lib
    text = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    assert L().azx_version() == 7
    assert EINVAL == int(re.search(r"AZX_EINVAL\s*=\s*(-?\d+)", text).group(1))
    # the play calls keep their signatures: the book is set beside them
    assert len(_lib.SYMBOLS["azx_match_play"][1]) == 7 and len(_lib.SYMBOLS["azx_tournament_play"][1]) == 11


def test_the_header_states_the_rule_and_that_the_reference_has_no_openings():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    sec = text[text.index("opening books: matches and tournaments"):text.index("int azx_openings_check(")]
    assert "azx_version stays 7" in sec and "dlsym azx_match_set_openings" in sec
    assert "(u >> 1) % n_openings" in sec and "u % n_openings" in sec and "absolute game index" in sec
    assert "NOT in the reference" in sec and "off by default" in sec
    assert "not enforced" in sec and "leaves the previous book in place" in sec
    assert "same kernels and returns the same bytes" in sec


def test_bad_arguments_are_einval_with_a_message_before_any_device_work():
    n, stride, mv, ln = table([[1, 2], [3]])
    pm, pl = mv.ctypes.data_as(_i16p), ln.ctypes.data_as(_i32p)
    lib = L()
    for fn in (lib.azx_match_set_openings, lib.azx_tournament_set_openings):
        for args in ((n, stride, pm, pl), (0, 0, None, None), (-1, stride, pm, pl)):
            assert fn(None, *args) == EINVAL
            assert b"null" in lib.azx_last_error()                      # the handle is looked at first
    for args, word in (((-1, stride, pm, pl), b"n_openings -1"),
                       (((1 << 20) + 1, stride, pm, pl), b"n_openings 1048577"),
                       ((n, -1, pm, pl), b"stride -1"),
                       ((n, stride, None, pl), b"null opening table"),
                       ((n, stride, pm, None), b"null opening table")):
        bo, bp = C.c_int32(-7), C.c_int32(-7)
        assert lib.azx_openings_check(5, *args, C.byref(bo), C.byref(bp)) == EINVAL, args
        assert word in lib.azx_last_error(), (args, lib.azx_last_error())
    for size in (1, 14, -3):
        assert lib.azx_openings_check(size, n, stride, pm, pl, None, None) == EINVAL
        assert b"board_size" in lib.azx_last_error()
    # success: the out-parameters are untouched, and may be null
    bo, bp = C.c_int32(-7), C.c_int32(-7)
    assert lib.azx_openings_check(5, n, stride, pm, pl, C.byref(bo), C.byref(bp)) == 0
    assert (bo.value, bp.value) == (-7, -7)
    assert lib.azx_openings_check(5, n, stride, pm, pl, None, None) == 0
    assert lib.azx_openings_check(5, 1, 2, table([[1, 1]])[2].ctypes.data_as(_i16p), table([[1, 1]])[3].ctypes.data_as(_i32p),
                                  None, None) == EINVAL                  # a refusal with null out-parameters


def test_an_empty_book_and_a_book_of_one_empty_opening_are_accepted():
    assert check(5, [])[:3] == (0, -7, -7)
    assert L().azx_openings_check(5, 0, 0, None, None, None, None) == 0
    assert check(5, [[]])[:3] == (0, -7, -7)
    assert check(5, [[]], stride=0)[:3] == (0, -7, -7)


@pytest.mark.parametrize("n", [2, 3, 5, 11, 13])
def test_the_check_is_the_host_rules(n):
    """Seeded random permutations of the board: with w the index of the first move after which HexGame reports a
    result, every prefix of at most w moves is an opening and the prefix of w + 1 moves is refused at ply w."""
    from azalea_amd.game.hex import HexGame
    rng = np.random.RandomState(20261019 + n)
    cells = n * n
    count = 300 if n <= 5 else 200
    book, first_win = [], []
    for _ in range(count):
        perm = (rng.permutation(cells) + 1).tolist()
        h = HexGame(n)
        w = None
        for p, mv in enumerate(perm):
            h.step(mv)
            if h.state.result != 0:
                w = p
                break
        assert w is not None                                            # Hex has no draws: a full board is decided
        first_win.append(w)
        book.append(perm)
    # every prefix of length <= w, all in one book: prefix lengths 0 .. w of the first 20 permutations, then length w
    # and a random shorter length of the others
    good = []
    for i, (perm, w) in enumerate(zip(book, first_win)):
        lens = range(w + 1) if i < 20 else (w, int(rng.randint(0, w + 1)))
        good += [perm[:k] for k in lens]
    rc, bo, bp, msg = check(n, good)
    assert (rc, bo, bp) == (0, -7, -7), msg
    for i, (perm, w) in enumerate(zip(book, first_win)):
        rc, bo, bp, msg = check(n, [perm[:w], perm[:w + 1]])
        assert (rc, bo, bp) == (EINVAL, 1, w), (i, msg)
        assert "opening 1, ply %d" % w in msg and "decides the game for colour %d" % (1 + (w & 1)) in msg, msg
    # the first offending opening is the one reported, whatever follows it
    w0 = first_win[0]
    rc, bo, bp, _ = check(n, [[], book[1][:first_win[1]], book[0][:w0 + 1], book[2][:first_win[2] + 1]])
    assert (rc, bo, bp) == (EINVAL, 2, w0)


@pytest.mark.parametrize("n", [2, 3, 5, 11, 13])
def test_repeats_moves_off_the_board_and_long_lengths_are_refused_where_they_stand(n):
    cells = n * n
    rc, bo, bp, msg = check(n, [[1], [2, 1, 2]] if n > 2 else [[1], [2, 2]])
    assert (rc, bo) == (EINVAL, 1) and bp == (2 if n > 2 else 1) and "played twice" in msg, msg
    for bad in (0, cells + 1, -1):
        rc, bo, bp, msg = check(n, [[], [cells, bad]])
        assert (rc, bo, bp) == (EINVAL, 1, 1) and "move %d outside [1, %d]" % (bad, cells) in msg, msg
    rc, bo, bp, msg = check(n, [[1], [1, 2]], stride=1)                  # lengths[1] = 2 > stride 1
    assert (rc, bo) == (EINVAL, 1) and "length 2" in msg and "stride 1" in msg, msg
    n_, stride, mv, ln = table([[1]])
    ln[0] = -1
    assert L().azx_openings_check(n, 1, stride, mv.ctypes.data_as(_i16p), ln.ctypes.data_as(_i32p), None, None) == EINVAL


def test_openings_check_raises_value_error_with_the_librarys_message():
    from azalea_amd import engine
    assert engine.openings_check(5, [[1, 2, 3], [], [25]]) is None
    assert engine.openings_check(5, None) is None and engine.openings_check(5, []) is None
    with pytest.raises(ValueError, match=r"opening 1, ply 1: tile 6 is played twice"):
        engine.openings_check(5, [[1], [7, 7]])
    with pytest.raises(ValueError, match=r"opening 0, ply 0: move 26 outside \[1, 25\]"):
        engine.openings_check(5, [[26]])
    engine.openings_check(7, [[26]])                                    # on 7x7 the same move is on the board
    with pytest.raises(ValueError, match=r"decides the game"):
        engine.openings_check(2, [[1, 2, 3]])                           # X on tiles 0 and 2: a column of the 2x2 board


def test_all_openings():
    from azalea_amd import engine
    one, two = engine.all_openings(5, 1), engine.all_openings(5, 2)
    assert one == [[t] for t in range(1, 26)]
    assert len(two) == 600 and len(set(map(tuple, two))) == 600
    assert two == sorted(two) and all(len(o) == 2 and o[0] != o[1] for o in two)
    engine.openings_check(5, one)
    engine.openings_check(5, two)
    engine.openings_check(3, engine.all_openings(3, 2))                 # nothing that shallow is decided from 3x3 up
    for plies in (0, 3):
        with pytest.raises(ValueError, match="plies must be 1 or 2"):
            engine.all_openings(5, plies)
    # on 2x2 two moves never decide either (a win needs two stones of one colour)
    assert len(engine.all_openings(2, 2)) == 12
    engine.openings_check(2, engine.all_openings(2, 2))


def test_openings_is_a_keyword_of_the_python_surface():
    from azalea_amd import engine, evaluation
    from azalea_amd.parallel_player import Player
    for fn in (engine.Match.play, engine.Tournament.play):
        assert inspect.signature(fn).parameters["openings"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    for fn in (evaluation.evaluate_throughput, Player.__init__):
        p = inspect.signature(fn).parameters["openings"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert callable(engine.Match.set_openings) and callable(engine.Tournament.set_openings)


# ---- the Player: the refusal comes before anything touches a GPU (the stubs of tests/option_api_stubs.py) -------
def test_player_refuses_openings_without_device_match(no_engines):
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    for agents, kw in (([a, b], {}), ([a], {}), ([a], dict(gather=False))):
        with pytest.raises(ValueError, match="openings are a device_match option"):
            Player(None, agents, openings=[[1], [2]], **kw)
    # no book, or an empty one, is no request
    assert Player(None, [a, b], openings=None).openings == []
    assert Player(None, [a, b], openings=[]).openings == []
