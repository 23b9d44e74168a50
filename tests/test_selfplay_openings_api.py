"""The weighted opening book of device self-play (azx_set_selfplay_openings), as far as it can be held without a GPU:
the bounds table against a numpy restatement of include/azx.h's formula, the draw's shares, the config normaliser's
forms and refusals, the Player's refusals and the book check.  The games are tests/test_gpu_selfplay_openings.py's."""
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
NEW_SYMBOLS = ("azx_set_selfplay_openings", "azx_selfplay_opening_word", "azx_selfplay_openings_bounds",
               "azx_selfplay_openings_slots", "azx_selfplay_openings_stats")
EINVAL = -1
SEED = 0xBAD5EED5                        # Engine's default seed: fixed before the shares below were looked at


def L():
    from azalea_amd import _lib
    return _lib.lib()


def numpy_bounds(weights):
    """ub[o] = (uint64) floor(ldexp(cum[o] / cum[n-1], 32)), cum the float64 running sum left to right, last 2^32."""
    cum = np.zeros(len(weights), np.float64)
    run = np.float64(0.0)
    for i, w in enumerate(weights):
        run = run + np.float64(w)
        cum[i] = run
    ub = np.floor(np.ldexp(cum / cum[-1], 32)).astype(np.uint64)
    ub[-1] = np.uint64(1 << 32)
    return ub


def test_the_header_declares_the_symbols_and_the_binding_requires_them():
    from azalea_amd import _lib
    text = open(os.path.join(ROOT, "include", "azx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    assert L().azx_version() == 7
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    sec = flat[flat.index("a weighted opening book for device self-play"):flat.index("int azx_set_selfplay_openings(")]
    assert "azx_version stays 7" in sec and "dlsym azx_set_selfplay_openings" in sec
    assert "NOT the reference's behaviour" in sec and "off by default" in sec
    assert "floor(ldexp(cum[o] / cum[n-1], 32))" in sec and "least o with word < ub[o]" in sec
    assert "THE LAST CALL WINS" in sec and "leaves the previous book in place" in sec
    assert "same kernels and returns the same bytes" in sec and "not measured" in sec


@pytest.mark.parametrize("weights", [
    [1.0] * 7, [1.0], [0.0, 1.0, 2.0], [1.0, 0.0, 0.0, 3.0], [1.0, 2.0, 0.0], [0.0, 0.0, 5.0, 0.0, 0.0],
    list(np.logspace(-12, 0, 41)), list(np.logspace(0, -12, 41)), [1e-12, 1.0, 1e-12], [3.0, 1e-300, 3.0],
    list(np.random.RandomState(5).rand(1000)),
])
def test_the_bounds_are_the_formula_bit_for_bit(weights):
    from azalea_amd import engine
    ub = engine.selfplay_openings_bounds(weights)
    assert ub.dtype == np.uint64 and np.array_equal(ub, numpy_bounds(weights))
    assert (np.diff(ub.astype(np.int64)) >= 0).all() and int(ub[-1]) == 1 << 32
    for o, w in enumerate(weights):                      # a zero weight owns no word
        if w == 0.0:
            assert int(ub[o]) == (int(ub[o - 1]) if o else 0)


@pytest.mark.parametrize("n", [1, 2, 3, 121, 14520])
def test_uniform_bounds_are_the_formula_with_equal_weights(n):
    from azalea_amd import engine
    assert np.array_equal(engine.selfplay_openings_bounds(n), numpy_bounds([1.0] * n))
    ub = np.zeros(n, np.uint64)
    assert L().azx_selfplay_openings_bounds(n, None, ub.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    assert np.array_equal(ub, numpy_bounds([1.0] * n))


@pytest.mark.parametrize("weights, word", [([0.0, 0.0], "all zero"), ([1.0, -0.5], "weight 1 (-0.5) is negative"),
                                           ([float("nan"), 1.0], "weight 0 (nan) is not finite"),
                                           ([1.0, float("inf")], "weight 1 (inf) is not finite"),
                                           ([1e308, 1e308], "sum is not finite")])
def test_bad_weights_are_a_value_error_with_the_librarys_message(weights, word):
    from azalea_amd import engine
    with pytest.raises(ValueError, match=re.escape(word)) as err:
        engine.selfplay_openings_bounds(weights)
    assert "selfplay openings" in str(err.value) and str(err.value) == L().azx_last_error().decode()
    for n in (0, -1, (1 << 20) + 1):
        with pytest.raises(ValueError, match="n_openings"):
            engine.selfplay_openings_bounds(n)
    assert L().azx_selfplay_openings_bounds(2, None, None) == EINVAL
    assert L().azx_selfplay_opening_word(1, 2, None) == EINVAL
    assert L().azx_set_selfplay_openings(None, 0, 0, None, None, None) == EINVAL and b"null" in L().azx_last_error()


def test_the_draws_shares_are_the_weights():
    """2^16 games of one seed over [0, 1, 1, 2, 4, 0, 1, 1]: the zero weights are never drawn and every other count is
    within six binomial standard deviations of n p."""
    from azalea_amd import engine
    w = np.array([0, 1, 1, 2, 4, 0, 1, 1], np.float64)
    n = 1 << 16
    uids = np.arange(n)
    idx = engine.selfplay_opening_index(SEED, uids, engine.selfplay_openings_bounds(w))
    counts = np.bincount(idx, minlength=8)
    assert counts.sum() == n and counts[0] == 0 and counts[5] == 0
    p = w / w.sum()
    sd = np.sqrt(n * p * (1 - p))
    for o in (1, 2, 3, 4, 6, 7):
        assert abs(counts[o] - n * p[o]) <= 6 * sd[o], (o, counts[o], n * p[o], sd[o])
    # the draw has no input but (seed, uid): the scalar form, any order and any subset give the same opening
    assert engine.selfplay_opening_index(SEED, 12345, engine.selfplay_openings_bounds(w)) == idx[12345]
    assert np.array_equal(engine.selfplay_opening_index(SEED, uids[::-7], engine.selfplay_openings_bounds(w)), idx[::-7])
    assert "n_games" not in inspect.signature(engine.selfplay_opening_index).parameters
    # ... keyed on seed + uid, as the game's key is
    assert engine.selfplay_opening_word(SEED, 77) == engine.selfplay_opening_word(SEED + 70, 7)
    assert engine.selfplay_opening_word(SEED, 77) != engine.selfplay_opening_word(SEED + 1, 77)


def test_the_words_are_a_stream_of_their_own():
    """Against the playout-cap word of the same (seed, uid, ply 0), restated from playout_cap.h: no word in common
    among 4096 games, and no common bit pattern beyond chance."""
    from azalea_amd import engine

    def mix32(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)

    def cap_word(seed, uid, ply):
        s = (seed + uid) & 0xFFFFFFFFFFFFFFFF
        k0, k1 = s & 0xFFFFFFFF, (s >> 32) ^ 0x5bd1e995
        return mix32(((k0 ^ 0x50434150) + mix32(((k1 ^ 0x43415021) + ply * 0x2c1b3c6d) & 0xFFFFFFFF)) & 0xFFFFFFFF)
    # the restatement is the library's: a ply is full iff word < ceil(p * 2^32)
    for u in range(64):
        assert engine.playout_cap_is_full(SEED, u, 0, 0.5) == (cap_word(SEED, u, 0) < (1 << 31))
    book = np.array([engine.selfplay_opening_word(SEED, u) for u in range(4096)], np.uint64)
    cap = np.array([cap_word(SEED, u, 0) for u in range(4096)], np.uint64)
    assert not (book == cap).any() and len(set(book.tolist())) == 4096
    agree = ((book >> np.uint64(31)) == (cap >> np.uint64(31))).mean()        # the top bits are independent coins
    assert abs(agree - 0.5) < 6 * 0.5 / np.sqrt(4096)


# ---- the normaliser ---------------------------------------------------------------------------------------------------
def test_the_normaliser_takes_every_form():
    from azalea_amd import engine
    from azalea_amd.parallel_player import normalize_selfplay_openings as norm
    assert norm(None) is None
    assert norm([[1], [2, 3], []]) == ([[1], [2, 3], []], None)
    assert norm(((1,), (2, 3))) == ([[1], [2, 3]], None)
    assert norm({"book": [[1], [2]]}) == ([[1], [2]], None)
    assert norm({"book": [[1], [2]], "weights": [1, 3]}) == ([[1], [2]], [1.0, 3.0])
    assert norm({"all": 1}, 5) == (engine.all_openings(5, 1), None)
    assert norm({"all": 2}, 3) == (engine.all_openings(3, 2), None)
    book, w = norm({"all": 1, "empty_share": 0.25}, 3)
    assert book == [[]] + engine.all_openings(3, 1) and w == [0.25] + [0.75 / 9] * 9
    book, w = norm({"book": [[1], [2]], "empty_share": 0.5})
    assert book == [[], [1], [2]] and w == [0.5, 0.25, 0.25]
    assert norm({"book": [[4]], "empty_share": 0})[1] == [0.0, 1.0]
    assert norm({"book": [[4]], "empty_share": 1})[1] == [1.0, 0.0]


@pytest.mark.parametrize("spec, size, word", [
    ({"book": [[1]], "all": 1}, 5, "exactly one of 'book' and 'all'"),
    ({"weights": [1.0]}, 5, "exactly one of 'book' and 'all'"),
    ({"book": [[1]], "plies": 1}, 5, "takes the keys"),
    ({"all": 3}, 5, "'all' must be 1 or 2"),
    ({"all": True}, 5, "'all' must be 1 or 2"),
    ({"all": 1}, None, "needs the board size"),
    ([], 5, "the book is empty"),
    ({"book": []}, 5, "the book is empty"),
    ("12", 5, "list of move lists"),
    ([1, 2], 5, "list of move lists"),
    ([[1.5]], 5, "list of move lists"),
    ({"book": [[1], [2]], "weights": [1.0]}, 5, "1 weights for 2 openings"),
    ({"book": [[1], [2]], "weights": [1.0, -1.0]}, 5, "finite and >= 0"),
    ({"book": [[1], [2]], "weights": [1.0, float("nan")]}, 5, "finite and >= 0"),
    ({"book": [[1], [2]], "weights": [0.0, 0.0]}, 5, "all zero"),
    ({"book": [[1], [2]], "weights": "ab"}, 5, "list of numbers"),
    ({"book": [[1]], "weights": [1.0], "empty_share": 0.5}, 5, "cannot be given together"),
    ({"book": [[1]], "empty_share": 1.5}, 5, r"empty_share must be a number in \[0, 1\]"),
    ({"book": [[1]], "empty_share": -0.1}, 5, r"empty_share must be a number in \[0, 1\]"),
    ({"book": [[1]], "empty_share": "half"}, 5, r"empty_share must be a number in \[0, 1\]"),
])
def test_the_normaliser_refuses(spec, size, word):
    from azalea_amd.parallel_player import normalize_selfplay_openings as norm
    with pytest.raises(ValueError, match=word):
        norm(spec, size)


# ---- the Player: the refusals come before anything touches a GPU (the stubs of tests/option_api_stubs.py) ------
def test_selfplay_openings_is_a_new_keyword_and_openings_keeps_its_refusal(no_engines):
    from azalea_amd.parallel_player import Player
    for name in ("selfplay_openings", "selfplay_opening_weights", "openings"):
        p = inspect.signature(Player.__init__).parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert callable(Player.opening_stats)
    a = _Agent(_cpu_policy())
    with pytest.raises(ValueError, match="openings are a device_match option"):
        Player(None, [a], openings=[[1], [2]])
    assert Player(None, [a]).selfplay_openings is None and Player(None, [a]).opening_stats() is None


def test_player_refuses_selfplay_openings_where_no_self_play_engine_runs(no_engines, monkeypatch):
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    book = [[1], [2, 3]]
    monkeypatch.setattr(Player, "_match_policies", lambda self: None)    # (a device match wants CUDA networks first)
    with pytest.raises(ValueError, match=r"selfplay_openings is a self-play option: a device match .*\(use openings="):
        Player(None, [a, b], device_match=True, gather=False, selfplay_openings=book)
    with pytest.raises(ValueError, match="selfplay_openings is a self-play option: it needs a single agent, got 2"):
        Player(None, [a, b], selfplay_openings=book)
    with pytest.raises(ValueError, match="selfplay_openings needs the games to run in a device engine"):
        Player(None, [_Agent(object())], selfplay_openings=book)           # no Policy with a HexNetwork: the host loop
    with pytest.raises(ValueError, match="selfplay_opening_weights given without selfplay_openings"):
        Player(None, [a], selfplay_opening_weights=[1.0])


def test_a_book_the_check_refuses_is_refused_with_the_same_message():
    """Engine.set_selfplay_openings runs azx_openings_check first: these are the messages it then raises
    (tests/test_gpu_selfplay_openings.py holds that it does, and that the book before stays)."""
    from azalea_amd import engine
    for book, word in (([[1, 1]], "is played twice"), ([[26]], "outside [1, 25]"),
                       ([[1, 2, 6, 3, 11, 4, 16, 7, 21]], "decides the game for colour 1")):
        with pytest.raises(ValueError, match=re.escape(word)) as err:
            engine.openings_check(5, book)
        assert str(err.value) == L().azx_last_error().decode()


def test_player_checks_the_book_before_any_engine(no_engines, monkeypatch):
    from azalea_amd import parallel_player
    a = _Agent(_cpu_policy())
    monkeypatch.setattr(parallel_player.Player, "_device_policy", lambda self: a.policy)
    with pytest.raises(ValueError, match="tile 0 is played twice"):
        parallel_player.Player(None, [a], selfplay_openings=[[1, 1]])
    with pytest.raises(ValueError, match="2 weights for 1 openings"):
        parallel_player.Player(None, [a], selfplay_openings=[[1]], selfplay_opening_weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="weights given twice"):
        parallel_player.Player(None, [a], selfplay_openings={"book": [[1]], "weights": [1.0]},
                               selfplay_opening_weights=[1.0])
    p = parallel_player.Player(None, [a], selfplay_openings={"all": 1, "empty_share": 0.5})
    assert p.selfplay_openings[0][0] == [] and len(p.selfplay_openings[0]) == 26
    assert p.selfplay_openings[1][0] == 0.5
    p = parallel_player.Player(None, [a], selfplay_openings=[[1], [2]], selfplay_opening_weights=[1, 0])
    assert p.selfplay_openings == ([[1], [2]], [1.0, 0.0])


def test_train_names_the_config_key_in_its_refusal():
    from azalea_amd.policy_trainer import train
    with pytest.raises(ValueError, match=r"config\['selfplay_openings'\]: .*'all' must be 1 or 2"):
        train(None, dict(selfplay_openings={"all": 4}, board_size=5), None)
