"""Forced playouts at the root and policy target pruning (azx_set_forced_playouts; NOT the reference's behaviour, off
by default), as far as they can be held without a GPU: the C ABI's three entry points (declared, bound), the header's
statement of the rule, the Python surface, the refusals of Player and train, which come before any engine is made, and
the CPU restatement of the rule (tests/forced_playouts_reference.py): pinned, rule off, to the unmodified oracle bit for
bit, with the conditions on its positions asserted.  The searches on the device are tests/test_gpu_forced_playouts.py's."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forced_playouts_reference as ref  # noqa: E402
from option_api_stubs import _Agent, _RandomAgent, _cpu_policy, no_engines  # noqa: E402,F401

NEW_SYMBOLS = ("azx_set_forced_playouts", "azx_get_forced_playouts", "azx_forced_playouts_stats")
f32 = np.float32


def header():
    return open(os.path.join(ROOT, "include", "azx.h")).read()


@pytest.fixture(autouse=True)
def the_option_exists():
    """The restatement and the prune function are the reference OF the library's option: without its entry points
    there is nothing for them to be the reference of."""
    from azalea_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name


def L():
    from azalea_amd import _lib
    return _lib.lib()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_header_declares_the_three_symbols_and_the_binding_requires_them():
    from azalea_amd import _lib
    text = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    assert L().azx_version() == 7
    # azx_config and azx_play_stats are unchanged: the option is set beside them
    assert len(_lib.Config._fields_) == 18 and len(_lib.PlayStats._fields_) == 20


def test_the_header_states_the_rule_and_that_it_is_not_the_reference():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    sec = text[text.index("Forced playouts at the root and policy target pruning"):text.index("int azx_set_forced_playouts(")]
    sec = re.sub(r" +", " ", sec)                               # (the formulas are aligned in columns)
    assert "NOT the reference's behaviour" in sec and "off by default" in sec
    assert "azx_version stays 7" in sec and "dlsym azx_set_forced_playouts" in sec
    # forcing, in the issue's words
    assert "{ j : n_j > 0 and n_j * n_j < (k * P_j) * S }" in sec
    assert "virtual losses of the batch in flight included" in sec
    assert "lowest-index member instead of the PUCT argmax" in sec
    assert "fast plies never force" in sec and "Below the root nothing changes" in sec
    # pruning
    assert "puct_b = (-w_b) / n_b + (c * P_b) * (sq / (1 + n_b))" in sec
    assert "gap = puct_b - Q_i" in sec and "f_i = sqrtf((k * P_i) * S)" in sec
    assert "need = ((c * P_i) * sq) / gap - 1" in sec
    assert "r_i = ceilf(max(n_i - f_i, need)), clamped to [0, n_i]" in sec
    assert "if r_i < n_i and r_i <= 1: r_i = 0" in sec
    assert "BOTH the move draw and the row" in sec and "r_i / sum r" in sec
    assert "Row metrics stay on the raw counts" in sec
    assert "float32 and unfused" in sec and "integers held in float32" in sec
    # arguments, scope, siblings
    assert "k == 0 with prune == 1 is AZX_EINVAL" in sec and "[0, 64]" in sec
    assert "leaves the setting in place" in sec
    assert "refuse an engine with the option set with AZX_EINVAL before touching any engine" in sec
    assert "early stop stays sound" in sec and "resignation judges the raw root" in sec
    assert "same kernels and returns the same bytes" in sec
    assert "forced=off or forced=<k>/<prune|noprune>" in sec
    assert "not measured" in sec


def test_the_python_surface():
    from azalea_amd import engine, policy_trainer
    from azalea_amd.parallel_player import Player
    for name in ("set_forced_playouts", "forced_playouts_stats", "forced_playouts", "clear_forced_playouts"):
        assert callable(getattr(engine.Engine, name)), name
    sig = inspect.signature(engine.Engine.set_forced_playouts).parameters
    assert sig["k"].default == 2.0 and sig["prune"].default is True
    p = inspect.signature(Player.__init__).parameters["forced_playouts"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for doc in (engine.Engine.set_forced_playouts.__doc__, Player.__init__.__doc__, policy_trainer.train.__doc__):
        assert "NOT the reference's behaviour" in doc and "not measured" in doc
    assert 'config["forced_playouts"]' in policy_trainer.train.__doc__
    assert engine.Engine.FORCED_PLAYOUTS_STATS == ("full_plies", "forced_selects", "rows_pruned", "visits_removed")


def test_normalize_forced_playouts():
    from azalea_amd.parallel_player import normalize_forced_playouts as norm
    assert norm(None) is None and norm(False) is None and norm((0, False)) is None
    assert norm(True) == (2.0, True)
    assert norm((1.5, False)) == (1.5, False) and norm([3, True]) == (3.0, True)
    assert norm({"k": 2.0, "prune": True}) == (2.0, True)
    for bad in ("on", 2.0, (2.0,), (2.0, True, 1), {"k": 2.0}, {"k": 2.0, "prune": True, "x": 1}):
        with pytest.raises(ValueError, match="forced_playouts"):
            norm(bad)
    for bad in ((-1.0, False), (65.0, True), (float("nan"), True), (float("inf"), False), ("2", True), (True, True)):
        with pytest.raises(ValueError, match="forced_playouts: k must be"):
            norm(bad)
    for bad in ((2.0, 1), (2.0, None), (2.0, "yes")):
        with pytest.raises(ValueError, match="forced_playouts: prune must be True or False"):
            norm(bad)
    with pytest.raises(ValueError, match="pruning needs forcing"):
        norm((0.0, True))


# ---- Player and train: the refusal comes before anything touches a GPU (the stubs of tests/option_api_stubs.py) --------
def test_player_takes_the_option_for_device_self_play_and_refuses_it_elsewhere(no_engines):
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    assert Player(None, [a]).forced_playouts is None
    assert Player(None, [a], forced_playouts=True).forced_playouts == (2.0, True)
    assert Player(None, [a], forced_playouts=(1.0, False)).forced_playouts == (1.0, False)
    assert Player(None, [a], forced_playouts=True).forced_playouts_stats() is None       # no engine yet
    # agents that play on the host: two agents, a random mover -- refused only when the option is on
    for agents in ([a, b], [_RandomAgent()]):
        assert Player(None, agents, forced_playouts=None).forced_playouts is None
        with pytest.raises(ValueError, match="forced_playouts needs the games to run in a device engine"):
            Player(None, agents, forced_playouts=True)
    with pytest.raises(ValueError):
        Player(None, [a, b], device_match=True, forced_playouts=True)
    for bad in ("yes", 0.5, (True,), (2.0, 1)):
        with pytest.raises(ValueError, match="forced_playouts"):
            Player(None, [a], forced_playouts=bad)


def test_device_match_refuses_the_option_by_name(no_engines, monkeypatch):
    """With the match's own requirements met (stubbed: they need networks on a GPU), the option is what is refused."""
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    monkeypatch.setattr(Player, "_match_policies", lambda self: [a.policy, b.policy])
    assert Player(None, [a, b], device_match=True).forced_playouts is None
    with pytest.raises(ValueError, match="forced_playouts is a self-play option"):
        Player(None, [a, b], device_match=True, forced_playouts=True)


def test_train_refuses_a_bad_value_before_it_builds_anything(no_engines, tmp_path, monkeypatch):
    from azalea_amd import policy_trainer

    def refuse(*a, **kw):
        raise AssertionError("train went on after a bad config['forced_playouts']")
    monkeypatch.setattr(policy_trainer, "initialize_replay_buffer", refuse)
    monkeypatch.setattr(policy_trainer, "Player", refuse)
    policy = _cpu_policy()
    base = dict(seed=1, device="cpu", game="azalea_amd.game.hex.HexGame", board_size=5)
    for bad in ("on", 0.5, {"k": 2.0}, {"k": 100.0, "prune": True}, {"k": 0.0, "prune": True}, {"k": 2.0, "prune": 1}):
        with pytest.raises(ValueError, match=r"config\['forced_playouts'\]: forced_playouts"):
            policy_trainer.train(policy, dict(base, forced_playouts=bad), str(tmp_path / "run"))
    assert not (tmp_path / "run").exists()


# ---- the CPU restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
def test_the_restatement_with_the_rule_off_is_the_unmodified_oracle_bit_for_bit(kind):
    refs = ref.positions(kind)
    assert len(refs) >= 60
    for r in refs:                                              # every position: none may be dropped
        nv, tv, pp = ref.oracle_root(r["prefix"], kind)
        assert np.array_equal(bits(nv), bits(r["off_n"])), r["prefix"]
        assert np.array_equal(bits(tv), bits(r["off_w"])), r["prefix"]
        assert np.array_equal(bits(pp), bits(r["off_p"])), r["prefix"]
        assert 0 < r["off_n"].sum() <= ref.SIMS + ref.BS and 0 < r["n"].sum() <= ref.SIMS + ref.BS     # (duplicates in a batch back up once)


@pytest.mark.parametrize("kind", ref.KINDS)
def test_the_positions_meet_their_conditions(kind):
    refs = ref.positions(kind)
    with_forced = sum(r["forced"] > 0 for r in refs)
    pruned = sum(r["removed"] > 0 for r in refs)
    print("%s: positions %d, with forced selects %d, forced selects %d (overriding the argmax %d), root counts changed "
          "%d, rows pruned %d, visits removed %d"
          % (kind, len(refs), with_forced, sum(r["forced"] for r in refs), sum(r["overrode"] for r in refs),
             sum(not np.array_equal(r["n"], r["off_n"]) for r in refs), pruned, sum(r["removed"] for r in refs)))
    assert with_forced >= 0.9 * len(refs)
    assert any(r["overrode"] > 0 for r in refs)
    if kind == "hash":
        assert pruned >= 0.5 * len(refs)
    for r in refs:
        assert 0 <= r["overrode"] <= r["forced"] <= ref.SIMS + ref.BS
        assert (r["r"] <= r["n"]).all() and (r["r"] >= 0).all() and r["r"].max() == r["n"].max()


# ---- the prune function on hand-made cases ---------------------------------------------------------------------------
def test_prune_keeps_a_child_that_looks_no_worse_than_the_best():
    # gap <= 0: child 1's mean value (-w / n = 0.8) is above the leader's whole PUCT score: nothing is given back
    n, w, P = [10, 5, 0], [0.0, -4.0, 0.0], [0.3, 0.3, 0.4]
    S, sq = f32(15), np.sqrt(f32(15))
    puct_b = f32(0.0) / f32(10) + (f32(0.5) * f32(0.3)) * (sq / f32(11))
    assert puct_b - f32(0.8) <= 0
    assert ref.prune(n, w, P).tolist() == [10, 5, 0]


def test_prune_takes_a_child_reduced_to_one_visit_out():
    # a bad child (Q = -1) with a small prior: need < 0 and n - f <= 1, so the single playout left goes too
    n, w, P = [50, 2, 0], [-10.0, 2.0, 0.0], [0.5, 0.1, 0.4]
    f = np.sqrt((f32(2.0) * f32(0.1)) * f32(52))
    assert f32(2) - f <= 1 and f32(2) - f > -2
    assert ref.prune(n, w, P).tolist() == [50, 0, 0]
    # the same child with more visits than its quota covers keeps the rest: ceil(9 - f) = 6 > 1
    n = [50, 9, 0]
    f = np.sqrt((f32(2.0) * f32(0.1)) * f32(59))
    assert ref.prune(n, [-10.0, 9.0, 0.0], P).tolist() == [50, float(np.ceil(f32(9) - f)), 0] == [50, 6, 0]


def test_prune_leaves_maxima_ties_and_unvisited_children_alone():
    n, w, P = [20, 20, 3, 0, 20], [-2.0, 5.0, 3.0, 0.0, 19.0], [0.2, 0.2, 0.2, 0.2, 0.2]
    r = ref.prune(n, w, P)
    assert r[[0, 1, 4]].tolist() == [20, 20, 20] and r[3] == 0 and r[2] < 3
    assert ref.prune([0, 0, 0], [0, 0, 0], [0.3, 0.3, 0.4]).tolist() == [0, 0, 0]
    assert ref.prune([7], [1.0], [1.0]).tolist() == [7]
    assert ref.prune([], [], []).tolist() == []


def test_a_larger_k_removes_no_fewer_visits():
    rng = np.random.RandomState(5)
    removed_any = 0
    for _ in range(200):
        k = rng.randint(2, 26)
        n = rng.randint(0, 60, k).astype(f32)
        w = (rng.uniform(-1, 1, k) * n).astype(f32)
        P = rng.dirichlet(np.ones(k)).astype(f32)
        last = None
        for kk in (0.5, 1.0, 2.0, 4.0, 16.0, 64.0):
            r = ref.prune(n, w, P, k=kk)
            assert (r <= n).all() and (r >= 0).all() and (r == np.rint(r)).all()
            if last is not None:
                assert (r <= last).all()                         # child by child
            last = r
        removed_any += int((n - last).sum() > 0)
    assert removed_any > 100


def test_the_restatement_counts_a_forced_select_only_at_the_root_of_a_visited_child():
    """One batch by hand on the empty 5x5 board, value 0 everywhere: the first select has no visited child (no forced
    set); from the second on child 0, visited once with n * n = 1 < (2 / 25) * S only once S > 12.5, is not forced
    within the first batch of 10, so the batch spreads over children 0..9 as PUCT alone would."""
    s = ref.Search([], "uniform", k=2.0, sims=0, bs=10)
    assert s.forced == 0 and s.n[:10].tolist() == [1] * 10 and s.n[10:].sum() == 0
    s = ref.Search([], "uniform", k=2.0, sims=10, bs=10)        # two batches: S reaches 13 in the second
    assert s.forced > 0 and s.n.sum() == 20
