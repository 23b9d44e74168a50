"""Gumbel root search with sequential halving (azx_set_gumbel; NOT the reference's behaviour, off by default), as far as
it can be held without a GPU: the C ABI's entry points (declared, bound, their argument types), the Python surface, the
refusals of Player, evaluate_throughput and train, which come before any engine is made, the noise's host function
(azx_gumbel_variate) against a numpy restatement of Philox and against the Gumbel distribution, and the CPU restatement
of the rule (tests/gumbel_reference.py): pinned, rule off, to the unmodified oracle bit for bit, with the schedule's
properties and the condition on its positions asserted.  The searches on the device are tests/test_gpu_gumbel.py's."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forced_playouts_reference as fp  # noqa: E402
import gumbel_reference as ref  # noqa: E402
from option_api_stubs import _Agent, _RandomAgent, _cpu_policy  # noqa: E402,F401

NEW_SYMBOLS = ("azx_set_gumbel", "azx_get_gumbel", "azx_gumbel_stats", "azx_gumbel_variate", "azx_selftest_gumbel",
               "azx_gumbel_state")
f32 = np.float32


def header():
    return open(os.path.join(ROOT, "include", "azx.h")).read()


def L():
    from azalea_amd import _lib
    return _lib.lib()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_symbols_and_the_binding_requires_them():
    from azalea_amd import _lib
    text = header()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    S = _lib.SYMBOLS
    vp, i64p, u64p, f32p = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    assert S["azx_set_gumbel"][1] == [vp, C.c_int, C.c_float, C.c_float, C.c_int]
    assert S["azx_get_gumbel"][1] == [vp, C.POINTER(C.c_int), f32p, f32p, C.POINTER(C.c_int)]
    assert S["azx_gumbel_stats"][1] == [vp, i64p]
    assert S["azx_gumbel_variate"][1] == [C.c_uint64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_double)]
    assert S["azx_selftest_gumbel"][1] == [C.c_int, C.c_int, C.POINTER(C.c_uint32), f32p]
    assert S["azx_gumbel_state"][1] == [vp, u64p, u64p]
    assert L().azx_version() == 7
    # azx_config and azx_play_stats are unchanged: the option is set beside them
    assert len(_lib.Config._fields_) == 18 and len(_lib.PlayStats._fields_) == 20


def test_the_header_states_the_definition_its_deviations_and_that_it_is_not_the_reference():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    sec = text[text.index("Gumbel root search with sequential halving"):text.index("int azx_set_gumbel(")]
    for phrase in ("NOT the reference's behaviour", "0x47554D42", "0x4E4F4953", "g_j = -ln(-ln u)", "DEVIATION 1",
                   "DEVIATION 2", "floor(r * NBt / R) == b", "ceil(|S| / 2)", "sigma_j = ((c_visit + n_max) * c_scale) * qh_j",
                   "softmax_j(ln P_j + sigma_j)", "No Dirichlet noise", "NOT measured", "AZX_EINVAL",
                   "azx_match_play / azx_tournament_play refuse"):
        assert phrase in sec, phrase


def test_null_arguments_and_bad_variate_inputs_are_einval_without_a_gpu():
    g = C.c_double(0)
    assert L().azx_set_gumbel(None, 8, 50.0, 1.0, 1) == -1
    assert L().azx_gumbel_stats(None, None) == -1 and L().azx_gumbel_state(None, None, None) == -1
    assert L().azx_gumbel_variate(1, 2, 3, 4, None) == -1
    assert L().azx_gumbel_variate(1, 2, -1, 4, C.byref(g)) == -1
    assert L().azx_gumbel_variate(1, 2, 3, -1, C.byref(g)) == -1 and L().azx_gumbel_variate(1, 2, 3, 192, C.byref(g)) == -1
    from azalea_amd import engine
    for bad in ((1, 2, -1, 0), (1, 2, 0, 192)):
        with pytest.raises(ValueError):
            engine.gumbel_variate(*bad)


# ---- the Python surface ----------------------------------------------------------------------------------------------
def test_the_engine_has_the_methods_and_their_docstrings_say_what_is_not_checked():
    from azalea_amd import engine
    for name in ("set_gumbel", "clear_gumbel", "gumbel", "gumbel_stats", "gumbel_state"):
        assert callable(getattr(engine.Engine, name)), name
    assert callable(engine.gumbel_variate) and callable(engine.selftest_gumbel)
    doc = re.sub(r"\s+", " ", engine.Engine.set_gumbel.__doc__)
    assert "NOT the reference's behaviour" in doc and "recollection of the paper's board-game values" in doc
    assert "not checked here" in doc and "NOT measured" in doc
    assert engine.Engine.GUMBEL_STATS == ("plies", "halvings", "root_selects", "improved_rows")


def test_normalize_gumbel():
    from azalea_amd.parallel_player import normalize_gumbel as norm
    assert norm(None) is None and norm(False) is None and norm(0) is None and norm({"m": 0}) is None
    assert norm(True) == (16, 50.0, 1.0, True)
    assert norm(8) == (8, 50.0, 1.0, True) and norm(np.int64(32)) == (32, 50.0, 1.0, True)
    assert norm((8, 30, 0.5)) == (8, 30.0, 0.5, True) and norm([64, 0.0, 100.0]) == (64, 0.0, 100.0, True)
    assert norm({}) == (16, 50.0, 1.0, True) and norm({"m": 4, "improved_rows": False}) == (4, 50.0, 1.0, False)
    assert norm({"m": 4, "c_visit": 1, "c_scale": 2, "improved_rows": True}) == (4, 1.0, 2.0, True)
    doc = re.sub(r"\s+", " ", norm.__doc__)
    assert "recollection of the paper's board-game values" in doc and "not checked here" in doc
    for bad in ("on", 2.5, (8,), (8, 50.0), (8, 50.0, 1.0, True), {"m": 8, "x": 1}):
        with pytest.raises(ValueError, match="gumbel"):
            norm(bad)
    for bad in (1, 65, -3, (1, 50.0, 1.0), {"m": 2.0}, {"m": "8"}, {"m": True}):
        with pytest.raises(ValueError, match="gumbel: m must be"):
            norm(bad)
    for bad in ((8, -1.0, 1.0), (8, 2e4, 1.0), (8, float("nan"), 1.0), (8, "50", 1.0), (8, True, 1.0)):
        with pytest.raises(ValueError, match="gumbel: c_visit must be"):
            norm(bad)
    for bad in ((8, 50.0, 0.0), (8, 50.0, 101.0), (8, 50.0, float("inf")), (8, 50.0, float("nan")), (8, 50.0, None)):
        with pytest.raises(ValueError, match="gumbel: c_scale must be"):
            norm(bad)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="gumbel: improved_rows must be True or False"):
            norm({"m": 8, "improved_rows": bad})


# ---- Player, evaluate_throughput and train: the refusal comes before anything touches a GPU --------------------------
@pytest.fixture
def no_engines(monkeypatch):
    from azalea_amd import engine

    def refuse(*a, **kw):
        raise AssertionError("an engine was created before the arguments were checked")
    monkeypatch.setattr(engine, "Engine", refuse)
    monkeypatch.setattr(engine, "Match", refuse)
    monkeypatch.setattr(engine, "Tournament", refuse)


def test_player_takes_the_option_for_device_self_play_and_refuses_it_elsewhere(no_engines):
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    assert Player(None, [a]).gumbel is None and Player(None, [a], gumbel=False).gumbel is None
    assert Player(None, [a], gumbel=True).gumbel == (16, 50.0, 1.0, True)
    assert Player(None, [a], gumbel=8).gumbel == (8, 50.0, 1.0, True)
    assert Player(None, [a], gumbel=(8, 30.0, 2.0)).gumbel == (8, 30.0, 2.0, True)
    assert Player(None, [a], gumbel={"m": 8, "improved_rows": False}).gumbel == (8, 50.0, 1.0, False)
    assert Player(None, [a], gumbel=True).gumbel_stats() is None                          # no engine yet
    # agents that play on the host: two agents, a random mover -- refused only when the option is on
    for agents in ([a, b], [_RandomAgent()]):
        assert Player(None, agents, gumbel=None).gumbel is None
        with pytest.raises(ValueError, match="gumbel needs the games to run in a device engine"):
            Player(None, agents, gumbel=True)
    # together with the rules about PUCT visit leaders
    with pytest.raises(ValueError, match="gumbel cannot be set together with forced_playouts"):
        Player(None, [a], gumbel=True, forced_playouts=True)
    with pytest.raises(ValueError, match="gumbel cannot be set together with early_stop"):
        Player(None, [a], gumbel=16, early_stop=True)
    assert Player(None, [a], gumbel=True, forced_playouts=None, early_stop=False).gumbel is not None
    with pytest.raises(ValueError):
        Player(None, [a, b], device_match=True, gumbel=True)
    for bad in ("yes", 0.5, (True,), 1, 65):
        with pytest.raises(ValueError, match="gumbel"):
            Player(None, [a], gumbel=bad)


def test_device_match_refuses_the_option_by_name(no_engines, monkeypatch):
    """With the match's own requirements met (stubbed: they need networks on a GPU), the option is what is refused."""
    from azalea_amd.parallel_player import Player
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    monkeypatch.setattr(Player, "_match_policies", lambda self: [a.policy, b.policy])
    assert Player(None, [a, b], device_match=True).gumbel is None
    with pytest.raises(ValueError, match="gumbel is a self-play option"):
        Player(None, [a, b], device_match=True, gumbel=True)


def test_evaluate_throughput_refuses_the_option_before_any_engine_exists(no_engines, monkeypatch):
    from azalea_amd import evaluation

    def refuse(*a, **kw):
        raise AssertionError("evaluate_throughput looked at its agents before it refused the option")
    monkeypatch.setattr(evaluation, "_throughput_policy", refuse)
    for on in (True, 16, (8, 50.0, 1.0), {"m": 8}):
        with pytest.raises(ValueError, match="evaluate_throughput: gumbel is a self-play option"):
            evaluation.evaluate_throughput([object(), object()], 2, gumbel=on)
    with pytest.raises(ValueError, match="gumbel: m must be"):
        evaluation.evaluate_throughput([object(), object()], 2, gumbel=1)


def test_train_refuses_a_bad_value_before_it_builds_anything(no_engines, tmp_path, monkeypatch):
    from azalea_amd import policy_trainer

    def refuse(*a, **kw):
        raise AssertionError("train went on after a bad config['gumbel']")
    monkeypatch.setattr(policy_trainer, "initialize_replay_buffer", refuse)
    monkeypatch.setattr(policy_trainer, "Player", refuse)
    policy = _cpu_policy()
    base = dict(seed=1, device="cpu", game="azalea_amd.game.hex.HexGame", board_size=5)
    for bad in ("on", 0.5, 1, {"m": 100}, {"m": 8, "c_scale": 0.0}, {"m": 8, "improved_rows": 1}, (8, 50.0)):
        with pytest.raises(ValueError, match=r"config\['gumbel'\]: gumbel"):
            policy_trainer.train(policy, dict(base, gumbel=bad), str(tmp_path / "run"))
    # together with the rules about PUCT visit leaders: refused here too, not only where the Player is built
    for other, name in (({"forced_playouts": True}, "forced_playouts"), ({"early_stop": True}, "early_stop"),
                        ({"forced_playouts": (2.0, False), "early_stop": True}, "forced_playouts")):
        with pytest.raises(ValueError, match=r"config\['gumbel'\]: gumbel cannot be set together with config\['%s'\]" % name):
            policy_trainer.train(policy, dict(base, gumbel=16, **other), str(tmp_path / "run"))
    assert not (tmp_path / "run").exists()
    doc = re.sub(r"\s+", " ", policy_trainer.train.__doc__)
    assert 'config["gumbel"]' in doc and "recollection of the paper's board-game values" in doc


# ---- the noise: azx_gumbel_variate ---------------------------------------------------------------------------------------
def test_the_variate_is_a_pure_function_of_its_four_arguments():
    from azalea_amd.engine import gumbel_variate as gv
    base = (4242, 17, 3, 5)
    g = gv(*base)
    assert all(gv(*base) == g for _ in range(3))
    changed = [gv(4243, 17, 3, 5), gv(4242, 20, 3, 5), gv(4242, 17, 4, 5), gv(4242, 17, 3, 6), gv(4242, 17, 3, 4)]
    assert len(set(changed + [g])) == 6
    # only seed + uid enters the key (game_rng)
    assert gv(4242 + 5, 17 - 5, 3, 5) == g
    # a 64-bit seed is taken whole
    assert gv((1 << 63) + 4242, 17, 3, 5) != g


def test_the_variate_is_minus_ln_minus_ln_u_of_the_philox_words():
    from azalea_amd.engine import gumbel_variate as gv
    for seed, uid, ply in ((4242, 0, 0), (4242, 71, 13), (0, 0, 168), ((1 << 40) + 7, 1 << 33, 5), (2 ** 64 - 1, 3, 2)):
        children = np.arange(0, 169)
        words = ref.philox_words(seed, uid, ply, children)
        want = ref.gumbel_of_words(words)
        got = np.array([gv(seed, uid, ply, int(c)) for c in children])
        assert np.abs(got - want).max() <= 1e-12, (seed, uid, ply)
        assert len(set(words.tolist())) > 160                                    # four different words per Philox block
    # Philox4x32-10 itself, against the known-answer vector of the Random123 distribution (counter and key all ones)
    ones = ref.philox_block(0xFFFFFFFF, 0xFFFFFFFF, [0xFFFFFFFF] * 4)
    assert [int(x) for x in ones] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_the_variate_is_zero_on_no_input_by_accident_and_gumbel_distributed():
    from azalea_amd.engine import gumbel_variate as gv
    g = np.array([gv(20261020, uid, ply, child) for uid in range(625) for ply in (0, 7) for child in range(80)])
    assert len(g) == 100000 and (g != 0).all() and np.isfinite(g).all()
    assert g.min() > -2.86 and g.max() < 17.33
    n = len(g)
    mean, var = g.mean(), g.var()
    # Gumbel(0, 1): mean 0.5772, variance pi^2 / 6, fourth central moment (2.4 + 3) * variance^2
    sd2 = np.pi ** 2 / 6
    se_mean = np.sqrt(sd2 / n)
    se_var = np.sqrt((5.4 - 1.0) * sd2 ** 2 / n)
    print("mean %.5f (0.57722 +- %.5f), variance %.5f (%.5f +- %.5f)" % (mean, se_mean, var, sd2, se_var))
    assert abs(mean - 0.5772156649) <= 4 * se_mean and abs(var - sd2) <= 4 * se_var


# ---- the CPU restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
def test_the_restatement_with_the_option_off_is_the_unmodified_oracle_bit_for_bit(kind):
    prefixes = fp.prefixes(kind)
    assert len(prefixes) >= 60
    for prefix in prefixes:                                     # every position: none may be dropped
        s = ref.Search(prefix, kind, 0)
        nv, tv, pp = fp.oracle_root(prefix, kind)
        assert np.array_equal(bits(nv), bits(s.n)), prefix
        assert np.array_equal(bits(tv), bits(s.w)), prefix
        assert np.array_equal(bits(pp), bits(s.p)), prefix
        assert s.halvings == 0 and s.root_selects == 0 and s.survivor_sets == []


ALL_CASES = ref.CASES + ((ref.POW2.name, "pow2"),)


@pytest.mark.parametrize("name,kind", ALL_CASES)
def test_the_schedule_of_the_restatement(name, kind):
    setup, refs = ref.SETUP[name], ref.positions(name, kind)
    nbt, bs = setup.nbt, setup.cfg.bs
    for r in refs:
        k = r["k"]
        m0 = min(setup.m, k)
        R = max(1, int(np.ceil(np.log2(m0)))) if m0 > 1 else 1
        assert r["m0"] == m0 and r["R"] == R
        assert r["halvings"] == R - 1                                            # halvings per ply
        assert r["root_selects"] == nbt * bs == len(r["root_picks"])             # every select of the search
        sizes = [len(s) for s in r["survivor_sets"]]
        assert sizes[0] == m0 == len(r["candidates"]) and len(sizes) == R
        assert all(b == (a + 1) // 2 for a, b in zip(sizes, sizes[1:]))           # |S| follows ceil(|S| / 2)
        sets = [set(s.tolist()) for s in r["survivor_sets"]]
        assert all(b <= a for a, b in zip(sets, sets[1:])) and set(r["survivors"].tolist()) == sets[-1]
        assert r["move"] in sets[-1]
        # every root select lands on a survivor of its batch: walk the boundaries again
        at = [0] + [(q * nbt) // R for q in range(1, R)]                         # the batch each set takes effect at
        for i, pick in enumerate(r["root_picks"]):
            b = i // bs
            current = sets[max(j for j in range(R) if at[j] <= b)]
            assert pick in current, (r["prefix"], i, pick)
        assert abs(r["pi"].sum() - 1.0) <= 1e-12 and (r["pi"] >= 0).all() and len(r["pi"]) == k
        assert r["n"].sum() <= nbt * bs                                          # (duplicates in a batch back up once)
    if setup.family == "late":
        assert all(r["k"] < setup.m for r in refs)
    if setup.family == "9":
        assert all(64 < r["k"] <= 81 for r in refs)                              # two live register slots
    if kind == "pow2":
        assert all(len(set(r["p"].tolist())) > 1 for r in refs)
    if setup.family == "13":
        assert any(r["k"] > 128 for r in refs)
    if name == "m16_20":
        assert nbt == 3 and all(r["R"] == 4 for r in refs)                       # a halving at b = 0, before any visit
    if name == "m8_200":
        assert nbt == 21 and all(r["R"] == 3 for r in refs)                      # boundaries at 7 and 14
    if setup.greedy:
        assert all((r["g"] == 0).all() for r in refs)
    else:
        assert all((r["g"] != 0).all() for r in refs)


@pytest.mark.parametrize("name,kind", ALL_CASES)
def test_at_most_a_tenth_of_a_cases_positions_is_left_out(name, kind):
    refs = ref.positions(name, kind)
    unsafe = sum(not r["safe"] for r in refs)
    print("%s %s: %d positions, %d with a decision inside the margin of %g" % (name, kind, len(refs), unsafe, ref.MARGIN))
    assert len(refs) >= 5 and unsafe <= ref.MAX_UNSAFE_SHARE * len(refs)


@pytest.mark.parametrize("setup", ref.POW2Z, ids=[s.name for s in ref.POW2Z])
def test_the_zero_prior_positions_are_what_the_gpu_test_needs(setup):
    """Exact zeros among the priors ("pow2z"): every expanded node kept a legal cell of nonzero weight (pow2z_prior asserts
    it), every decision is safe, the improved row is finite and 0 exactly where P = 0; with m = 8 no zero-prior child is a
    candidate, on the "few" positions (m = 16) some must be, are visited and never survive.  The device stub computes the
    same rows to the bit (on the CPU here), and the forcing rule under these priors never forces a child with P = 0."""
    import torch
    refs = ref.positions(setup.name, "pow2z")
    assert len(refs) >= 8 and all(r["safe"] for r in refs)
    assert all(len(r["prefix"]) <= ref.POW2Z_MAX_PLIES for r in refs)
    for r in refs:
        z = r["p"] == 0
        assert z.any() and not z.all() and np.isfinite(r["pi"]).all() and abs(r["pi"].sum() - 1.0) <= 1e-12
        assert np.array_equal(r["pi"] == 0, z) and not z[r["survivors"]].any() and not z[r["move"]]
        if setup.family == "few":
            assert ref.nonzero_pow2z(r["prefix"]) < r["m0"] and z[r["candidates"]].any() and (r["n"][z] > 0).any()
        else:
            assert not z[r["candidates"]].any()
        legal = ref.game_at(r["prefix"], setup.cfg).legal_moves()
        row = np.zeros((1, setup.cfg.cells), np.int32)
        row[0, :len(legal)] = legal
        v, p = ref.pow2z_device_evaluator(setup.cfg.n, torch.device("cpu"))(torch.zeros(1, 5, 5), torch.tensor(row))
        assert float(v[0]) == 0 and np.array_equal(bits(p[0, :len(legal)].numpy()), bits(r["p"])) and not p[0, len(legal):].any()
    if setup.family != "few":
        fz = ref.forced_positions_pow2z()
        assert len(fz) == len(refs) and sum(r["forced"] for r in fz) > 100 and sum(r["removed"] for r in fz) > 100
        assert all(r["p"][j] > 0 for r in fz for j in r["forced_at"])
        assert any(((r["p"] == 0) & (r["n"] > 0)).any() for r in fz)            # bare Q does reach a zero-prior child


def test_the_safe_decision_rule_on_hand_made_keys():
    keys = np.array([3.0, 2.0005, 2.0, 1.0])
    ident = [(0.0, 0.25, 1.0, 0.0)] * 4
    kept, dropped = ref.top(keys, np.arange(4), 2)
    assert kept.tolist() == [0, 1] and dropped.tolist() == [2, 3]
    assert ref.safe_cut(keys, kept, dropped, ident)                              # identical (g, P, n, w): an exact tie on both sides
    other = list(ident)
    other[2] = (0.0, 0.25, 2.0, 0.0)
    assert not ref.safe_cut(keys, kept, dropped, other)                          # 5e-4 apart and not identical
    assert ref.safe_cut(np.array([3.0, 2.002, 2.0, 1.0]), kept, dropped, other)  # 2e-3 apart
    # ties go to the lower index
    kept, dropped = ref.top(np.array([1.0, 2.0, 2.0, 2.0]), np.arange(4), 2)
    assert kept.tolist() == [1, 2] and dropped.tolist() == [0, 3]
    # two zero priors (ln 0 = -inf on both sides) tie exactly whatever else differs; -inf against a finite key is safe
    ninf = np.array([1.0, -np.inf, -np.inf, -np.inf])
    kept, dropped = ref.top(ninf, np.arange(4), 2)
    assert kept.tolist() == [0, 1] and dropped.tolist() == [2, 3] and ref.safe_cut(ninf, kept, dropped, other)
    # sigma: the completion is the prior-weighted mean of the visited children's qh
    sig = ref.sigma_of([2, 0, 1], [1.0, 0.0, -1.0], [0.5, 0.25, 0.25], 50.0, 1.0)
    qh = [0.5 * (-1.0 / 2) + 0.5, None, 0.5 * (1.0 / 1) + 0.5]
    vh = (0.5 * qh[0] + 0.25 * qh[2]) / 0.75
    assert np.allclose(sig, [52 * qh[0], 52 * vh, 52 * qh[2]])
    assert np.allclose(ref.sigma_of([0, 0], [0, 0], [0.5, 0.5], 50.0, 2.0), [50.0, 50.0])       # no child visited: 0.5
