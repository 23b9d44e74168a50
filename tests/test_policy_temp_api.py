"""The policy temperature of the search's priors (azx_set_policy_temp; NOT the reference's behaviour, off by default), as
far as it can be held without a GPU: the C ABI's entry points (declared, bound, their argument types), the host function
azx_policy_temp_row against the numpy definition of tests/policy_temp_reference.py bit for bit on random rows, that
restatement pinned, rule off, to fpu_reference.Search bit for bit, the normaliser, the Python plumbing (Policy, Player,
config["policy_temp"]) and the documents.  The searches on the device are tests/test_gpu_policy_temp.py's."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpu_reference as fref  # noqa: E402
import policy_temp_reference as ref  # noqa: E402
from fpu_reference import Settings  # noqa: E402
from option_api_stubs import _Agent, _RandomAgent, _cpu_policy, no_engines  # noqa: E402,F401

NEW_SYMBOLS = ("azx_set_policy_temp", "azx_get_policy_temp", "azx_policy_temp_stats", "azx_policy_temp_row")
f32 = np.float32


def read(*path):
    return open(os.path.join(ROOT, *path)).read()


def L():
    from azalea_amd import _lib
    return _lib.lib()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_symbols_and_the_binding_requires_them():
    from azalea_amd import _lib
    text = read("include", "azx.h")
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and name not in _lib.OPTIONAL, name
        fn = getattr(L(), name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS[name][1], name
    S = _lib.SYMBOLS
    vp, i64p, f32p, ip = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int)
    assert S["azx_set_policy_temp"][1] == [vp, C.c_int, C.c_int]
    assert S["azx_get_policy_temp"][1] == [vp, ip, ip]
    assert S["azx_policy_temp_stats"][1] == [vp, i64p]
    assert S["azx_policy_temp_row"][1] == [C.c_int, C.c_int, f32p, f32p, ip]
    assert L().azx_version() == 7                               # an addition within the revision: found by symbol
    assert len(_lib.Config._fields_) == 18 and len(_lib.PlayStats._fields_) == 20
    assert "azx_set_policy_temp" in read("tools", "lib_bench.py")       # an older library is benchmarked without them


def test_the_header_states_the_definition_and_that_it_is_not_the_reference():
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", read("include", "azx.h")))
    sec = text[text.index("Policy temperature for the search's priors"):text.index("int azx_set_policy_temp(")]
    for phrase in ("NOT the reference's behaviour", "outside every parity claim", "not a self-play option",
                   "(8, 8) is off", "m = 7, 6, 5, 4 give 1.14, 1.33, 1.6, 2", "Each step is one float32 operation, unfused",
                   "If m = 8, the row is returned as it is", "is not finite, is below 0 or is above 1",
                   "s1 = sqrtf(P_j), s2 = sqrtf(s1), s3 = sqrtf(s2)", "bit 2 selects s1, bit 1 s2, bit 0 s3",
                   "(uint32_t)(q_j * 16777216.0f)", "If Z == 0, the row is returned as delivered",
                   "Zf = (float)Z * (1.0f / 16777216.0f)", "The result is q_j / Zf", "AT EXPANSION", "AT THE ROOT",
                   "ONE TABLE PRIOR", "The stored priors are not rewritten", "root_eighths is unused", "visited mass",
                   "ln P", "AZX_ESTATE", "AZX_EINVAL", "leaving the setting in place", "visit-dependent c(s)",
                   "by symbol", "temp=off"):
        assert phrase in sec, phrase


def test_the_kernels_and_the_host_compile_one_text_of_the_rule():
    rule = read("azalea_amd", "csrc", "policy_temp.h")
    assert "__host__ __device__ inline float azx_pt_q(" in rule and "__host__ __device__ inline uint32_t azx_pt_word(" in rule
    assert "fp contract(off)" in rule
    for user in ("mcts_kernels.hip", "azx_capi.cpp"):
        text = read("azalea_amd", "csrc", user)
        assert '#include "policy_temp.h"' in text and "azx_pt_q(" in text and "azx_pt_word(" in text, user
        assert "azx_pt_zf(" in text and "azx_pt_bad(" in text, user
    make = read("azalea_amd", "csrc", "Makefile")
    assert make.count("policy_temp.h") >= 2                     # in the digest of the kernel sources and in the unit's rule
    # the option is an engine's search property: not among the self-play options
    capi = read("azalea_amd", "csrc", "azx_capi.cpp")
    table = capi[capi.index("static const OptionInfo SELFPLAY_OPTIONS[]"):capi.index("static std::string selfplay_option_fields")]
    assert "policy_temp" not in table.lower() and "policy temp" not in table.lower()
    from azalea_amd import selfplay_options
    assert "policy_temp" not in selfplay_options.BY_NAME
    # the fields go at the end of the struct every launch carries
    dev = read("azalea_amd", "csrc", "azx_dev.h")
    struct = dev[dev.index("struct DevEngine {"):dev.index("// expansions tempered")]
    assert struct.index("fpu_ctr;") < struct.index("pt_eighths;") < struct.index("pt_ctr;")
    assert struct.rstrip().endswith("};") and "pt_ctr;" in struct.rstrip().splitlines()[-2]


def row_call(m, p):
    out = np.full(len(p), f32(-7.0), f32)
    flag = C.c_int(-7)
    fp_ = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    assert L().azx_policy_temp_row(m, len(p), fp_(p), fp_(out), C.byref(flag)) == 0
    return out, flag.value


def test_null_arguments_and_bad_values_are_einval_without_a_gpu():
    p = np.full(3, f32(1.0) / f32(3.0), f32)
    out = np.zeros(3, f32)
    flag = C.c_int(-7)
    fp_ = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    assert L().azx_set_policy_temp(None, 6, 8) == -1 and L().azx_policy_temp_stats(None, None) == -1
    assert L().azx_get_policy_temp(None, None, None) == -1
    ok = (6, 3, fp_(p), fp_(out), C.byref(flag))
    assert L().azx_policy_temp_row(*ok) == 0 and flag.value == 1
    for i, bad in ((0, 0), (0, 9), (0, -1), (1, 0), (1, 193), (2, None), (3, None), (4, None)):
        args = list(ok)
        args[i] = bad
        assert L().azx_policy_temp_row(*args) == -1, (i, bad)
        assert b"policy temperature" in L().azx_last_error()


# ---- the definition --------------------------------------------------------------------------------------------------
KS = (1, 2, 63, 64, 65, 128, 129, 169)


def random_rows(count, seed=20261021):
    rng = np.random.RandomState(seed)
    for i in range(count):
        k = KS[i % len(KS)]
        m = 1 + (i // len(KS)) % 8
        alpha = 0.03 if (i // 64) % 2 == 0 else 1.0
        p = rng.dirichlet([alpha] * k).astype(f32) if k > 1 else np.ones(1, f32)
        yield k, m, alpha, p


def test_the_host_function_is_the_numpy_definition_bit_for_bit_on_random_rows():
    n = worst = 0
    seen = set()
    for k, m, alpha, p in random_rows(2000):
        want, done = ref.temper(p, m)
        got, flag = row_call(m, p)
        assert flag == int(done) == int(m != 8), (k, m, alpha)
        assert np.array_equal(bits(got), bits(want)), (k, m, alpha)
        if done:
            err = abs(float(got.astype(np.float64).sum()) - 1.0)
            worst = max(worst, err)
            assert err <= 1e-5, (k, m, alpha, err)
        else:
            assert np.array_equal(bits(got), bits(p))
        seen.add((k, m, alpha))
        n += 1
    print(n, "rows; the largest |row sum - 1| of a tempered row:", worst)
    assert n == 2000 and len(seen) == len(KS) * 8 * 2           # every k with every m at both alphas
    # rows inside the guard that sum far above 1: Z = k * 2^24 passes 2^31 from k = 128 on
    for k in (127, 128, 169, 192):
        for m in (1, 4, 7):
            ones = np.ones(k, f32)
            got, flag = row_call(m, ones)
            want, done = ref.temper(ones, m)
            assert flag == 1 and done and np.array_equal(bits(got), bits(want)), (k, m)
            assert np.array_equal(bits(got), bits(np.full(k, f32(1.0) / f32(k), f32))), (k, m)
    # in place
    p = np.random.RandomState(1).dirichlet([0.5] * 40).astype(f32)
    want = ref.temper(p, 5)[0]
    q = p.copy()
    flag = C.c_int(0)
    ptr = q.ctypes.data_as(C.POINTER(C.c_float))
    assert L().azx_policy_temp_row(5, 40, ptr, ptr, C.byref(flag)) == 0 and flag.value == 1
    assert np.array_equal(bits(q), bits(want))


def test_guard_rows_come_back_as_delivered():
    rng = np.random.RandomState(5)
    n = 0
    for k in KS:
        for m in range(1, 9):
            base = rng.dirichlet([1.0] * k).astype(f32) if k > 1 else np.ones(1, f32)
            for what, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf), ("negative", -0.1), ("above", 1.5)):
                p = base.copy()
                p[rng.randint(k)] = v
                got, flag = row_call(m, p)
                assert flag == 0 and np.array_equal(bits(got), bits(p)), (k, m, what)
                assert ref.temper(p, m)[1] is False
                n += 1
            zero = np.zeros(k, f32)
            got, flag = row_call(m, zero)
            assert flag == 0 and np.array_equal(bits(got), bits(zero)), (k, m, "all zero")
            n += 1
    assert n == len(KS) * 8 * 6


def test_the_peaked_row_of_the_issue_flattens_as_stated():
    """A 0.97-peaked row of 120 moves: 0.28 nats as delivered, 1.43 nats at m = 6 and 3.78 nats at m = 4."""
    p = np.full(120, 0.03 / 119, np.float64)
    p[0] = 0.97
    p = p.astype(f32)
    assert abs(ref.entropy(p) - 0.28) < 0.005
    assert abs(ref.entropy(ref.temper(p, 6)[0]) - 1.43) < 0.005
    assert abs(ref.entropy(ref.temper(p, 4)[0]) - 3.78) < 0.005
    from azalea_amd import engine
    out, done = engine.policy_temp_row(6, p)
    assert done and np.array_equal(bits(out), bits(ref.temper(p, 6)[0]))
    with pytest.raises(ValueError):
        engine.policy_temp_row(6, np.zeros((2, 2), f32))


# ---- the restatement -------------------------------------------------------------------------------------------------
def same_dump(a, b, what):
    assert a["num_nodes"] == b["num_nodes"] and a["root_id"] == b["root_id"], what
    for k in ("parent", "first_child", "num_children"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("num_visits", "total_value", "prior_prob"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


def test_with_the_rule_off_the_restatement_is_fpu_references_search():
    """(8, 8): the whole tree of fpu_reference.Search -- which tests/test_fpu_api.py pins to the unmodified oracle -- for
    every evaluator, with and without first-play urgency, and once more after two moves on the carried subtree."""
    for n, sims in ((5, 60), (9, 40)):
        cfg = Settings(n=n, sims=sims, bs=10, c_puct=0.5, tree_cap=1 << 17)
        for kind in fref.KINDS:
            for prefix in ((), ref.prefix_third(n)):
                for fpu in (fref.OFF, fref.MODES[3]):
                    a, b = ref.Search(prefix, kind, ref.OFF, fpu, cfg=cfg), fref.Search(prefix, kind, fpu, cfg=cfg)
                    same_dump(a.dump(), b.dump(), (n, kind, prefix, fpu))
                    assert a.temp_stats() == ref.ZERO_STATS and a.stats() == b.stats()
                    if fpu == fref.OFF and kind != "skew":
                        same_dump(a.dump(), fref.oracle_dump(prefix, kind, cfg, cfg.sims, cfg.bs), (n, kind, prefix, "oracle"))
                    if prefix == ():
                        c = fref.most_visited(b)
                        a.move_and_search(c)
                        b.move_and_search(c)
                        same_dump(a.dump(), b.dump(), (n, kind, fpu, "moved"))


def test_the_rule_changes_searches_of_row_evaluators_and_no_others():
    cfg = Settings(n=5, sims=100, bs=10, c_puct=0.5)
    off = ref.Search((), "skew", ref.OFF, cfg=cfg)
    for temp in ref.SETTINGS:
        on = ref.Search((), "skew", temp, cfg=cfg)
        assert not np.array_equal(on.n, off.n) or not np.array_equal(bits(on.dump()["prior_prob"]), bits(off.dump()["prior_prob"])), temp
        st = on.temp_stats()
        assert st["left_as_delivered"] == 0
        assert (st["tempered"] > 0) == (temp[0] != 8) and st["root_searches"] == int(temp[1] != 8), (temp, st)
        if temp[0] == 8:                                        # the root rule alone: the stored priors are the OFF run's rows
            first = int(on.first[0])
            assert np.array_equal(bits(on.pp[first:first + 25]), bits(off.pp[first:first + 25]))
        for kind in ("uniform", "hash"):                        # one table prior for all children: untouched
            a, b = ref.Search((), kind, temp, cfg=cfg), ref.Search((), kind, ref.OFF, cfg=cfg)
            same_dump(a.dump(), b.dump(), (kind, temp))
            assert a.temp_stats() == ref.ZERO_STATS
    bad = ref.Search((), "skewbad", (6, 4), cfg=cfg)
    st = bad.temp_stats()
    assert st["tempered"] > 0 and st["left_as_delivered"] > 0, st


# ---- the Python plumbing -----------------------------------------------------------------------------------------------
def test_normalize_policy_temp():
    from azalea_amd.policy_temp import normalize_policy_temp as norm
    for off in (None, False, (8, 8), [8, 8], 8, {}, {"eighths": 8}, {"eighths": 8, "root_eighths": 8}):
        assert norm(off) is None, off
    assert norm(6) == (6, 8) == norm((6, 8)) == norm([6, 8]) == norm({"eighths": 6}) == norm(np.int64(6))
    assert norm((8, 4)) == (8, 4) == norm({"root_eighths": 4})
    assert norm({"eighths": 3, "root_eighths": np.int32(5)}) == (3, 5)
    for bad in (True, 0, 9, -1, 6.0, "6", (6,), (6, 8, 8), (0, 8), (6, 9), (6.5, 8), {"m": 6}, {"eighths": "6"},
                {"eighths": True}, {"root_eighths": 0}):
        with pytest.raises(ValueError, match="policy_temp"):
            norm(bad)


class _RecordingEngine:
    def __init__(self):
        self.calls = []

    def set_policy_temp(self, *a):
        self.calls.append(a)

    def clear_policy_temp(self):
        self.calls.append("clear")


def test_apply_sets_an_engine_once_and_a_policy_carries_the_setting(no_engines):
    from azalea_amd import policy_temp as pt
    from azalea_amd.parallel_player import Player
    from azalea_amd.policy import Policy
    e = _RecordingEngine()
    pt.apply(e, None)
    assert e.calls == []                                        # off on a fresh engine: nothing to do
    pt.apply(e, (6, 8))
    pt.apply(e, (6, 8))                                         # unchanged: the statistics are not zeroed again
    pt.apply(e, None)
    assert e.calls == [(6, 8), "clear"]
    p = _cpu_policy()
    assert p.policy_temp is None and pt.policy_policy_temp(p) is None
    p.set_policy_temp(6)
    assert p.policy_temp == (6, 8)
    p.set_policy_temp((8, 8))
    assert p.policy_temp is None
    q = Policy()
    cfg = dict(device="cpu", network="HexNetwork", board_size=5, num_blocks=1, base_chans=32, simulations=10,
               search_batch_size=2, exploration_coef=0.5, exploration_depth=3, exploration_noise_alpha=0.3,
               exploration_noise_scale=0.25, exploration_temperature=1.0, policy_temp={"eighths": 4, "root_eighths": 7})
    q.initialize(cfg)
    assert q.policy_temp == (4, 7) and q.fpu is None
    assert "policy_temp" not in q.state_dict()                  # a setting of the search: checkpoints keep their format
    with pytest.raises(ValueError, match="policy_temp"):
        Policy().initialize(dict(cfg, policy_temp=9))
    # Player puts it on every agent's policy -- one agent, two agents, beside a random mover -- and refuses nonsense
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    assert Player(None, [a]).policy_temp is None and a.policy.policy_temp is None
    assert Player(None, [a, b], policy_temp=6).policy_temp == (6, 8) == a.policy.policy_temp == b.policy.policy_temp
    b.policy.set_policy_temp((4, 4))
    Player(None, [a, b])                                        # None leaves each policy's own setting
    assert a.policy.policy_temp == (6, 8) and b.policy.policy_temp == (4, 4)
    Player(None, [a, _RandomAgent()], policy_temp=(8, 8))
    assert a.policy.policy_temp == (6, 8)                       # off / None: nothing is pushed
    assert Player(None, [a], fpu=True, policy_temp=(3, 5)).fpu is not None and a.policy.policy_temp == (3, 5)
    with pytest.raises(ValueError, match="policy_temp"):
        Player(None, [a], policy_temp=0.75)
    for doc in (Player.__init__.__doc__, Policy.set_policy_temp.__doc__):
        doc = re.sub(r"\s+", " ", doc)
        assert "NOT the reference's behaviour" in doc and "policy_temp" in doc


class _StubLib:
    """Stands in for the loaded library under Engine.set_policy_temp / clear_policy_temp / policy_temp_stats."""

    def __init__(self):
        self.calls = []
        self.setting = (8, 8)

    def azx_set_policy_temp(self, h, m, r):
        self.calls.append((m, r))
        self.setting = (m, r)
        return 0

    def azx_get_policy_temp(self, h, m, r):
        m._obj.value, r._obj.value = self.setting
        return 0

    def azx_policy_temp_stats(self, h, out):
        for i, v in enumerate((5, 7, 3)):
            C.cast(out, C.POINTER(C.c_int64))[i] = v
        return 0


def test_engine_methods_check_their_arguments_and_a_refused_value_keeps_the_setting():
    from azalea_amd import engine

    class Stub:
        L, h = _StubLib(), None
        POLICY_TEMP_STATS, _stats = engine.Engine.POLICY_TEMP_STATS, engine.Engine._stats
    e = Stub()
    engine.Engine.set_policy_temp(e, 6, 8)
    engine.Engine.set_policy_temp(e, 4, 7)
    engine.Engine.set_policy_temp(e, np.int32(1), 8)
    assert e.L.calls == [(6, 8), (4, 7), (1, 8)]
    with pytest.raises(TypeError):                              # no default setting, as the normaliser has none
        engine.Engine.set_policy_temp(e)
    engine.Engine.set_policy_temp(e, 3, 5)
    n = len(e.L.calls)
    for bad in ((0, 8), (9, 8), (6, 0), (6, 9), (6.0, 8), ("6", 8), (True, 8), (6, None), (-1, -1)):
        with pytest.raises(ValueError, match="policy_temp"):
            engine.Engine.set_policy_temp(e, *bad)
    assert len(e.L.calls) == n and engine.Engine.policy_temp(e) == (3, 5)       # EINVAL keeps the setting
    engine.Engine.clear_policy_temp(e)
    assert e.L.calls[-1] == (8, 8) and engine.Engine.policy_temp(e) == (8, 8)
    assert engine.Engine.policy_temp_stats(e) == dict(tempered=5, left_as_delivered=7, root_searches=3, reserved=0)
    doc = re.sub(r"\s+", " ", engine.Engine.set_policy_temp.__doc__)
    assert "NOT the reference's behaviour" in doc and "outside every parity claim" in doc and "AZX_ESTATE" in doc
    # the library itself refuses them too, and says which
    capi = read("azalea_amd", "csrc", "azx_capi.cpp")
    body = capi[capi.index('extern "C" int azx_set_policy_temp('):capi.index('extern "C" int azx_get_policy_temp(')]
    assert body.index("pt_check(") < body.index("AZX_ESTATE") < body.index("e->pt_eighths = eighths")


def test_train_names_the_config_key_and_says_so_before_anything_is_built(no_engines):
    from azalea_amd import policy_trainer
    doc = re.sub(r"\s+", " ", policy_trainer.train.__doc__)
    assert 'config["policy_temp"]' in doc and "NOT the reference's behaviour" in doc and "NOT measured" in doc
    p = _cpu_policy()
    with pytest.raises(ValueError, match=r"config\['policy_temp'\]: policy_temp"):
        policy_trainer.train(p, dict(policy_temp=12), "/nonexistent")


# ---- the documents -------------------------------------------------------------------------------------------------------
def test_the_documents_name_the_option_where_they_name_the_others():
    design = read("DESIGN.md")
    assert re.search(r"^\*\*7\.22 Policy temperature", design, re.M)
    sec = re.sub(r"\s+", " ", design[design.index("**7.22 Policy temperature"):])
    for phrase in ("NOT the reference's behaviour", "azx_set_policy_temp", "profiles/policy_temp_resources.txt", "c(s)",
                   "k_mcts_pt", "12 600", "2.1e-6", "NOT measured"):
        assert phrase in sec, phrase
    readme = re.sub(r"\s+", " ", read("README.md"))
    i = readme.index("`azx_set_policy_temp` / `Engine.set_policy_temp`")
    item = readme[i:i + 4000]
    for phrase in ("NOT the reference's behaviour", "off by default", "outside every parity claim", "set_policy_temp"):
        assert phrase in item, phrase
    assert os.path.exists(os.path.join(ROOT, "profiles", "policy_temp_resources.txt"))
