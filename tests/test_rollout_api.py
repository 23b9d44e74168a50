"""The rollout evaluator (azx_set_rollout_evaluator; NOT the reference's behaviour, off unless asked for), as far as it
can be held without a GPU: the C ABI's entry points, their argument checks, the host definition (azx_rollout_value)
against the pure-Python restatement of include/azx.h's text (tests/rollout_reference.py) in `wins` and in the bits of
`value`, hand-built full boards, unbiasedness against exact win probabilities, and RolloutNet under the reference's
network contract.  The kernel and the searches on the device are tests/test_gpu_rollout.py's."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rollout_reference as ref  # noqa: E402

NEW_SYMBOLS = ("azx_set_rollout_evaluator", "azx_rollout_value", "azx_selftest_rollout", "azx_rollout_stats")
SIZES = (2, 3, 5, 8, 9, 11, 13)         # one, two and three mask words; 8x8 is exactly 64 cells
SEED = 0x1234_5678_9ABC_DEF1
i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)


def L():
    from azalea_amd import _lib
    return _lib.lib()


def raw_value(seed, N, board, R, wins=True, value=True):
    b = None if board is None else np.ascontiguousarray(board, np.int32)
    w, v = C.c_int32(-1), C.c_float(9.0)
    rc = L().azx_rollout_value(seed, N, None if b is None else b.ctypes.data_as(i32p), R,
                               C.byref(w) if wins else None, C.byref(v) if value else None)
    return rc, w.value, v.value


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_symbols_and_the_binding_requires_them():
    from azalea_amd import _lib
    text = open(os.path.join(ROOT, "include", "azx.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    S = _lib.SYMBOLS
    vp = C.c_void_p
    assert S["azx_set_rollout_evaluator"][1] == [vp, C.c_int, C.c_uint64]
    assert S["azx_rollout_value"][1] == [C.c_uint64, C.c_int, i32p, C.c_int, i32p, f32p]
    assert S["azx_selftest_rollout"][1] == [C.c_int, C.c_int, C.c_int, i32p, C.c_int, C.c_uint64, i32p, f32p, f32p,
                                            C.POINTER(C.c_uint8)]
    assert S["azx_rollout_stats"][1] == [vp, C.POINTER(C.c_int64)]
    assert L().azx_version() == 7
    assert len(_lib.Config._fields_) == 18 and len(_lib.PlayStats._fields_) == 20     # both unchanged


def test_the_header_states_the_definition_and_that_it_is_not_the_reference():
    text = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "azx.h")).read())
    sec = text[text.index("Rollout evaluator: a network-free MCTS opponent"):text.index("int azx_set_rollout_evaluator(")]
    for phrase in ("NOT the reference's behaviour", "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB",
                   "0x7feb352d", "0x846ca68b", "sm(seed + 4*c + board[c])", "lb((u32)H ^ lb((u32)(H >> 32) + r))",
                   "lb(k_r + c * 0x9E3779B9)", "((u64)w * rem) >> 32 < need", "(float)(2*wins - R) / (float)R",
                   "1.0f / (float)e", "AZX_FLAG_RANDOM_REFLECT", "the last call wins", "eval=rollout(R)"):
        assert phrase in sec, phrase


def test_argument_checks_return_errors_without_a_gpu():
    empty = np.zeros(9, np.int32)
    assert raw_value(1, 3, empty, 64)[0] == 0
    for R in (0, 4097, -1):
        assert raw_value(1, 3, empty, R)[0] == -1, R
    for N in (1, 14, 0, -3):
        assert raw_value(1, N, np.zeros(196, np.int32), 8)[0] == -1, N
    bad = empty.copy()
    bad[4] = 3
    assert raw_value(1, 3, bad, 8)[0] == -1
    bad[4] = -1
    assert raw_value(1, 3, bad, 8)[0] == -1
    assert raw_value(1, 3, None, 8)[0] == -1
    assert raw_value(1, 3, empty, 8, wins=False)[0] == -1
    assert raw_value(1, 3, empty, 8, value=False)[0] == -1
    assert b"rollout" in L().azx_last_error() or b"null" in L().azx_last_error()
    # the engine entry points and the self-test refuse their arguments before any device work
    out4 = (C.c_int64 * 4)()
    assert L().azx_set_rollout_evaluator(None, 8, 1) == -1
    assert L().azx_rollout_stats(None, out4) == -1
    w, v, p = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(9, np.float32)
    args = lambda N, b, R, ww=w, vv=v, pp=p: L().azx_selftest_rollout(      # noqa: E731
        0, N, 1, None if b is None else b.ctypes.data_as(i32p), R, 1,
        None if ww is None else ww.ctypes.data_as(i32p), None if vv is None else vv.ctypes.data_as(f32p),
        None if pp is None else pp.ctypes.data_as(f32p), None)
    bad[4] = 3
    for N, b, R in ((3, empty, 0), (3, empty, 4097), (1, empty, 8), (14, np.zeros(196, np.int32), 8), (3, bad, 8),
                    (3, None, 8)):
        assert args(N, b, R) == -1, (N, R)
    assert args(3, empty, 8, ww=None) == -1 and args(3, empty, 8, vv=None) == -1 and args(3, empty, 8, pp=None) == -1
    from azalea_amd import engine
    with pytest.raises(engine.AzxError):
        engine.rollout_value(1, empty, 0)
    with pytest.raises(ValueError):
        engine.rollout_value(1, np.zeros(10, np.int32), 8)


# ---- the host definition against the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_rollout_value_equals_the_reference_in_wins_and_value_bits(N):
    from azalea_amd import engine
    seen = set()
    for e, board in ref.position_family(N):
        assert int((board == 0).sum()) == e
        seen.add(e)
        for R in (1, 7, 64, 100, 4096):
            want = ref.rollout_wins(SEED, N, board, R)
            wins, value = engine.rollout_value(SEED, board.reshape(N, N), R)
            assert wins == want, (N, e, R)
            assert ref.bits(value) == ref.value_bits(want, R), (N, e, R)
    assert {1, N * N} <= seen and any(e % 2 for e in seen) and any(e % 2 == 0 for e in seen)


def test_the_seed_and_the_position_both_enter_the_key():
    from azalea_amd import engine
    board = ref.position_family(5)[4][1]
    a = [engine.rollout_value(s, board, 4096)[0] for s in (0, 1, 2 ** 63, 2 ** 64 - 1)]
    assert a == [ref.rollout_wins(s, 5, board, 4096) for s in (0, 1, 2 ** 63, 2 ** 64 - 1)]
    assert len(set(a)) > 1
    other = board.copy()
    i, j = np.flatnonzero(board == 1)[0], np.flatnonzero(board == 2)[0]
    other[i], other[j] = 2, 1
    assert engine.rollout_value(5, other, 64)[0] == ref.rollout_wins(5, 5, other, 64)


# ---- hand-built full boards (e = 0: all rollouts are the same board) ---------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_full_boards_spiral_wrapped_neighbours_and_wins_of_colour_two(N):
    from azalea_amd import engine
    boards = ref.full_boards(N)
    assert len(boards) >= 2
    for name, board, one_wins in boards:
        full = [int(v) for v in board]
        assert 0 not in full
        assert ref.one_connects(full, N) == one_wins and ref.two_connects(full, N) == (not one_wins), name
        if name.startswith("wrap"):      # the board would be a win to a flood fill that steps across the board's edge
            assert not one_wins and ref.wrapping_connects(full, N), name
        if name.startswith("two"):
            assert ref.two_connects(full, N), name
        for R in (1, 64, 100):
            wins, value = engine.rollout_value(SEED, board, R)
            assert wins == (R if one_wins else 0), (N, name, R)
            assert value == (1.0 if one_wins else -1.0), (N, name, R)
    if N >= 5:                           # the spiral's path is far longer than N: a fill capped at N steps would lose it
        name, board, one_wins = boards[0]
        assert name == "spiral" and one_wins and int((board == 1).sum()) > 2 * N


# ---- unbiasedness ---------------------------------------------------------------------------------------------------
def test_the_estimate_is_unbiased_on_the_small_family():
    from azalea_amd import engine
    R = 4096
    family = ref.small_family()
    assert len(family) == 14
    for N, board in family:
        p = ref.exact_win_probability(N, board)
        wins, _ = engine.rollout_value(12345, board, R)
        print("N=%d e=%d p=%.4f wins/R=%.4f" % (N, int((board == 0).sum()), p, wins / R))
        if p in (0.0, 1.0):
            assert wins == int(p) * R, (N, board)
        else:
            assert abs(wins / R - p) <= 5 * math.sqrt(p * (1 - p) / R), (N, board, p, wins / R)


# ---- RolloutNet under the reference's network contract ------------------------------------------------------------------
def test_rolloutnet_run_equals_the_reference_on_a_cpu_batch():
    import torch
    from azalea_amd.rollout import RolloutNet
    N, R, seed = 5, 32, 99
    net = RolloutNet(rollouts=R, seed=seed)
    assert net.device == torch.device("cpu") and net.eval() is net
    fam = ref.position_family(N)
    kmax = max(e for e, _ in fam)
    board = torch.tensor(np.stack([b.reshape(N, N) for _, b in fam]))
    legal = torch.zeros((len(fam), kmax), dtype=torch.int32)
    for i, (e, b) in enumerate(fam):
        legal[i, :e] = torch.tensor(np.flatnonzero(b == 0) + 1, dtype=torch.int32)
    out = net.run({"board": board, "legal_moves": legal})
    assert set(out) >= {"value", "moves_logprob"}
    assert out["value"].dtype == torch.float32 and out["value"].shape == (len(fam),)
    assert out["moves_logprob"].shape == (len(fam), kmax)
    prior = torch.exp(out["moves_logprob"]).numpy()
    for i, (e, b) in enumerate(fam):
        want = ref.rollout_wins(seed, N, b, R)
        assert ref.bits(out["value"][i].item()) == ref.value_bits(want, R), i
        assert abs(prior[i].sum() - 1.0) < 1e-6, i
        assert np.allclose(prior[i, :e], 1.0 / e, rtol=1e-6) and (prior[i, e:] == 0).all(), i
    with pytest.raises(ValueError):
        RolloutNet(rollouts=0)
    with pytest.raises(ValueError):
        RolloutNet(rollouts=4097)


def test_a_policy_accepts_a_rolloutnet():
    from azalea_amd.policy import Policy
    from azalea_amd.rollout import RolloutNet, is_rollout_net
    pol = Policy()
    pol.initialize(dict(device="cpu", network="azalea_amd.rollout.RolloutNet", board_size=5, num_blocks=0, base_chans=0,
                        simulations=20, search_batch_size=4, exploration_coef=0.5, exploration_depth=4,
                        exploration_noise_alpha=0.03, exploration_noise_scale=0.25, exploration_temperature=1.0))
    assert is_rollout_net(pol.net) and pol.net.rollouts == 64 and not pol._uses_device_net() and pol._uses_rollouts()
    pol.net = RolloutNet(rollouts=16, seed=3)
    assert pol.net.rollouts == 16 and pol._uses_rollouts()
    state = pol.state_dict()
    assert state["net"] == {} and state["network_type"] == "azalea_amd.rollout.RolloutNet"
    # the throughput surface takes it without external_batch and without a CUDA device
    from azalea_amd.evaluation import _throughput_policy

    class Agent:
        policy = pol
    assert _throughput_policy(Agent()) is pol
