"""First-play urgency (azx_set_fpu; NOT the reference's behaviour, off by default), as far as it can be held without a
GPU: the C ABI's entry points (declared, bound, their argument types), the host restatement azx_fpu_score against the
numpy restatement of tests/fpu_reference.py on random nodes, that restatement pinned, rule off, to the unmodified oracle
bit for bit, argument validation through a stub of the binding, the Python plumbing (Policy, Player, config["fpu"]),
and the documents.  The searches on the device are tests/test_gpu_fpu.py's."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpu_reference as ref  # noqa: E402
import option_positions as op  # noqa: E402
from fpu_reference import Settings  # noqa: E402
from option_api_stubs import _Agent, _RandomAgent, _cpu_policy, no_engines  # noqa: E402,F401

NEW_SYMBOLS = ("azx_set_fpu", "azx_get_fpu", "azx_fpu_stats", "azx_fpu_score")
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
    assert S["azx_set_fpu"][1] == [vp, C.c_int, C.c_float, C.c_float, C.c_float]
    assert S["azx_get_fpu"][1] == [vp, ip, f32p, f32p, f32p]
    assert S["azx_fpu_stats"][1] == [vp, i64p]
    assert S["azx_fpu_score"][1] == [C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, C.c_float,
                                     f32p, f32p, f32p, C.c_float, C.POINTER(C.c_int32)]
    assert re.search(r"#define AZX_FPU_OFF\s+0\b", text) and re.search(r"#define AZX_FPU_ABSOLUTE\s+1\b", text)
    assert re.search(r"#define AZX_FPU_REDUCTION\s+2\b", text)
    assert L().azx_version() == 7                               # an addition within the revision: found by symbol
    assert len(_lib.Config._fields_) == 18 and len(_lib.PlayStats._fields_) == 20


def test_the_header_states_the_definition_and_that_it_is_not_the_reference():
    text = re.sub(r"\s+", " ", re.sub(r"\s*\n \*\s*", " ", read("include", "azx.h")))
    sec = text[text.index("First-play urgency (FPU) for the PUCT search"):text.index("int azx_set_fpu(")]
    for phrase in ("NOT the reference's behaviour", "outside every parity claim", "nv_j == 0.0f takes Q_j = fpu",
                   "fpu = Qp - (r * sqrtf(mass))", "Qp = tv_p / max(nv_p, 1.0f)", "mass = (float)M * (1.0f / 16777216.0f)",
                   "(uint32_t)(prior_prob_j * 16777216.0f)", "STORED prior", "No clamp is applied",
                   "root_reduction at the search's root", "forced playouts still override the root argmax",
                   "root_reduction is unused there", "AZX_ESTATE", "AZX_EINVAL", "NOT computed", "visit-dependent c(s)",
                   "root policy temperature", "not a self-play option"):
        assert phrase in sec, phrase


def test_the_kernels_and_the_host_compile_one_text_of_the_rule():
    rule = read("azalea_amd", "csrc", "fpu.h")
    assert "__host__ __device__ inline float azx_fpu_q(" in rule and "__host__ __device__ inline uint32_t azx_fpu_mass_word(" in rule
    assert "fp contract(off)" in rule
    for user in ("mcts_kernels.hip", "azx_capi.cpp"):
        text = read("azalea_amd", "csrc", user)
        assert '#include "fpu.h"' in text and "azx_fpu_q(" in text and "azx_fpu_mass_word(" in text, user
    make = read("azalea_amd", "csrc", "Makefile")
    assert make.count("fpu.h") >= 2                             # in the digest of the kernel sources and in the unit's rule
    # the option is an engine's search property: not among the self-play options matches refuse
    capi = read("azalea_amd", "csrc", "azx_capi.cpp")
    table = capi[capi.index("static const OptionInfo SELFPLAY_OPTIONS[]"):capi.index("static std::string selfplay_option_fields")]
    assert "fpu" not in table.lower()
    from azalea_amd import selfplay_options
    assert "fpu" not in selfplay_options.BY_NAME


def test_null_arguments_and_bad_values_are_einval_without_a_gpu():
    out = C.c_int32(-7)
    nv, tv, p = (np.zeros(3, f32) for _ in range(3))
    fp_ = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))      # noqa: E731
    assert L().azx_set_fpu(None, 2, 0.0, 0.25, 0.0) == -1 and L().azx_fpu_stats(None, None) == -1
    assert L().azx_get_fpu(None, None, None, None, None) == -1
    ok = (2, 0.0, 0.25, 0.0, 0, 3, 1.0, 0.0, fp_(nv), fp_(tv), fp_(p), 0.5, C.byref(out))
    assert L().azx_fpu_score(*ok) == 0 and out.value == 0
    for i, bad in ((0, 3), (0, -1), (1, float("nan")), (1, 1.5), (1, -1.01), (2, -0.5), (2, float("nan")), (2, float("inf")),
                   (3, -1e-9), (3, float("nan")), (5, 0), (8, None), (9, None), (10, None), (12, None)):
        args = list(ok)
        if i == 1:
            args[0] = 1                                         # the value is checked in every mode but OFF
        args[i] = bad
        assert L().azx_fpu_score(*args) == -1, (i, bad)
        assert b"fpu" in L().azx_last_error()
    # mode OFF ignores the three parameters
    assert L().azx_fpu_score(0, 9.0, -1.0, float("nan"), 0, 3, 1.0, 0.0, fp_(nv), fp_(tv), fp_(p), 0.5, C.byref(out)) == 0


class _StubLib:
    """Stands in for the loaded library under Engine.set_fpu / clear_fpu / fpu_stats: records the calls."""

    def __init__(self):
        self.calls = []

    def azx_set_fpu(self, h, mode, value, reduction, root_reduction):
        self.calls.append((mode, value, reduction, root_reduction))
        return 0

    def azx_fpu_stats(self, h, out):
        C.cast(out, C.POINTER(C.c_int64))[0] = 5
        C.cast(out, C.POINTER(C.c_int64))[1] = 7
        C.cast(out, C.POINTER(C.c_int64))[2] = 3
        return 0


def test_engine_methods_check_their_arguments_before_the_library_sees_them():
    from azalea_amd import engine

    class Stub:
        L, h = _StubLib(), None
        FPU_MODES, FPU_STATS, _stats = engine.Engine.FPU_MODES, engine.Engine.FPU_STATS, engine.Engine._stats
    e = Stub()
    engine.Engine.set_fpu(e)
    engine.Engine.set_fpu(e, "absolute", -1)
    engine.Engine.set_fpu(e, "reduction", reduction=0.5, root_reduction=0.5)
    engine.Engine.set_fpu(e, "off", value=float("nan"))         # off: nothing is checked, zeros are what it means
    engine.Engine.clear_fpu(e)
    assert e.L.calls[:3] == [(2, 0.0, 0.25, 0.0), (1, -1.0, 0.25, 0.0), (2, 0.0, 0.5, 0.5)]
    assert e.L.calls[3][0] == 0 and e.L.calls[4] == (0, 0.0, 0.0, 0.0)
    n = len(e.L.calls)
    for bad in (dict(mode="on"), dict(mode=2), dict(mode="absolute", value=1.5), dict(mode="absolute", value=float("nan")),
                dict(reduction=-0.1), dict(reduction=float("inf")), dict(root_reduction=-1), dict(root_reduction=float("nan"))):
        with pytest.raises(ValueError, match="fpu"):
            engine.Engine.set_fpu(e, **bad)
    assert len(e.L.calls) == n
    assert engine.Engine.fpu_stats(e) == dict(selects=5, levels_with_unvisited=7, ended_unvisited=3, differs_from_off=0)
    doc = re.sub(r"\s+", " ", engine.Engine.set_fpu.__doc__)
    assert "NOT the reference's behaviour" in doc and "lc0's / KataGo's customary values as the author recalls them" in doc
    assert "not checked here" in doc and "outside every parity claim" in doc
    assert callable(engine.fpu_score) and callable(engine.Engine.fpu)
    with pytest.raises(ValueError):
        engine.fpu_score("reduction", [0, 1], [0, 0, 0], [0.5, 0.5], 1, 0, 0.5)
    with pytest.raises(ValueError):
        engine.fpu_score("sometimes", [0, 1], [0, 0], [0.5, 0.5], 1, 0, 0.5)


# ---- the restatement -------------------------------------------------------------------------------------------------
def same_dump(a, b, what):
    assert a["num_nodes"] == b["num_nodes"] and a["root_id"] == b["root_id"], what
    for k in ("parent", "first_child", "num_children"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("num_visits", "total_value", "prior_prob"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)


@pytest.mark.parametrize("n", (9, 13))
def test_with_the_rule_off_the_restatement_is_the_unmodified_oracle(n):
    """On tests/option_positions.py's positions (sweep: "uniform"; wide-hash: "hash"), the whole tree, and once more
    after two moves on the carried subtree."""
    cfg = Settings(n=n, sims=60, bs=10, c_puct=0.5, tree_cap=1 << 17)
    for kind, prefixes in (("uniform", op.sweep_prefixes(n)), ("hash", op.wide_hash_prefixes(n))):
        for i, prefix in enumerate(prefixes):
            s = ref.Search(prefix, kind, ref.OFF, cfg=cfg)
            same_dump(s.dump(), ref.oracle_dump(prefix, kind, cfg, cfg.sims, cfg.bs), (n, kind, prefix))
            assert s.stats() == dict(selects=0, levels_with_unvisited=0, ended_unvisited=0, differs_from_off=0)
            if i == 0:
                c1 = ref.most_visited(s)
                s.move_and_search(c1)
                c2 = ref.most_visited(s)
                s.move_and_search(c2)
                same_dump(s.dump(), ref.oracle_dump(prefix, kind, cfg, cfg.sims, cfg.bs, follow=(c1, c2)), (n, kind, prefix, "moved"))


def test_the_5x5_positions_and_the_forcing_rule_are_the_parent_classes():
    import forced_playouts_reference as fp
    for kind in fp.KINDS:
        for prefix in fp.prefixes(kind)[:6]:
            a, b = ref.Search(prefix, kind, ref.OFF, forced_k=fp.K_FORCED), fp.Search(prefix, kind, fp.K_FORCED)
            assert np.array_equal(bits(a.n), bits(b.n)) and np.array_equal(bits(a.w), bits(b.w))
            assert (a.forced, a.overrode, a.forced_at) == (b.forced, b.overrode, b.forced_at)


def test_the_rule_changes_searches_and_the_skew_priors_are_not_uniform():
    cfg = Settings(n=5, sims=100, bs=10, c_puct=0.5)
    changed = 0
    for mode in ref.MODES:
        for kind in ref.KINDS:
            on, off = ref.Search((), kind, mode, cfg=cfg), ref.Search((), kind, ref.OFF, cfg=cfg)
            changed += int(not np.array_equal(on.n, off.n))
            st = on.stats()
            assert st["selects"] == 110 and 0 < st["ended_unvisited"] <= 110 and st["levels_with_unvisited"] >= 110
    assert changed >= 10
    s = ref.Search((), "skew", ref.MODES[2], cfg=cfg)
    p = s.root_children()[2]
    assert len(np.unique(p)) >= 3 and abs(float(p.astype(np.float64).sum()) - 1.0) < 1e-6
    # the fixed-point mass of these priors is not a multiple of 1/k
    words = (p * ref.TWO24).astype(np.uint32)
    assert len(np.unique(words)) >= 3 and int(words.sum()) != 1 << 24


def random_nodes(count, seed=20261021):
    """(k, nv_p, tv_p, nv, tv, prior, c_puct, is_root) with every shape the issue names among them."""
    rng = np.random.RandomState(seed)
    for i in range(count):
        shape = i % 8
        k = 1 if shape == 0 else int(rng.randint(2, 170))
        nv = rng.randint(0, 40, k).astype(f32) * (rng.rand(k) < rng.uniform(0.1, 0.9)).astype(f32)
        if shape == 1:
            nv = np.maximum(nv, f32(1.0))                       # all children visited
        if shape == 2:
            nv[:] = 0                                           # no child visited
        tv = (rng.uniform(-1, 1, k) * nv).astype(f32)           # negative total values among them
        if shape == 3:
            tv = -np.abs(tv)
        tv[nv == 0] = 0
        w = rng.gamma(0.5, 1.0, k) + 1e-6
        prior = (w / w.sum()).astype(f32)                       # sums to 1 only after rounding
        if shape == 4:
            prior = ref.skew_prior(int(rng.randint(0, 1 << 32)), k)
        if shape == 5:
            prior = np.full(k, f32(1.0) / f32(k), f32)
        nv_p = f32(nv.sum() + 1)
        tv_p = f32(rng.uniform(-1, 1) * nv_p)
        is_root = bool(rng.rand() < 0.4)
        if shape == 6:                                          # a root with nv_p = 0 (a fresh root: its evaluation is not backed up)
            nv[:] = 0
            tv[:] = 0
            nv_p, tv_p, is_root = f32(0.0), f32(0.0), True
        yield k, nv_p, tv_p, nv, tv, prior, f32(rng.choice([0.25, 0.5, 1.0, 4.0])), is_root


def test_the_host_function_is_the_restatement_on_random_nodes():
    from azalea_amd import engine
    modes = (ref.OFF,) + ref.MODES + (("reduction", 0.0, 1.5, 0.125), ("absolute", 1.0, 0.0, 0.0))
    seen = dict(k1=0, all_visited=0, none_visited=0, fresh_root=0, negative=0, differs=0, inexact_sum=0)
    n = 0
    for k, nv_p, tv_p, nv, tv, prior, c, is_root in random_nodes(2400):
        mode = modes[n % len(modes)]
        n += 1
        want, score = ref.pick_child(mode, nv_p, tv_p, nv, tv, prior, prior, c, is_root)
        got = engine.fpu_score(mode[0], nv, tv, prior, nv_p, tv_p, c, is_root=is_root, value=mode[1], reduction=mode[2],
                               root_reduction=mode[3])
        assert got == want, (mode, k, nv_p, tv_p, got, want, score[got], score[want])
        off, _ = ref.pick_child(ref.OFF, nv_p, tv_p, nv, tv, prior, prior, c, is_root)
        seen["k1"] += k == 1
        seen["all_visited"] += bool((nv > 0).all())
        seen["none_visited"] += bool((nv == 0).all())
        seen["fresh_root"] += bool(nv_p == 0 and is_root)
        seen["negative"] += bool((tv < 0).any())
        seen["differs"] += want != off
        seen["inexact_sum"] += float(prior.astype(np.float64).sum()) != 1.0
    print(n, "nodes:", seen)
    assert n >= 2000 and all(v >= 50 for v in seen.values()), seen


# ---- the Python plumbing -----------------------------------------------------------------------------------------------
def test_normalize_fpu():
    from azalea_amd.fpu import normalize_fpu as norm
    assert norm(None) is None and norm(False) is None and norm("off") is None and norm({"mode": "off"}) is None
    assert norm(True) == ("reduction", 0.0, 0.25, 0.0) == norm("reduction") == norm({})
    assert norm("absolute") == ("absolute", 0.0, 0.25, 0.0)
    assert norm(("absolute", -1, 0, 0)) == ("absolute", -1.0, 0.0, 0.0)
    assert norm({"reduction": 0.5, "root_reduction": np.float32(0.5)}) == ("reduction", 0.0, 0.5, 0.5)
    doc = re.sub(r"\s+", " ", norm.__doc__)
    assert "lc0's / KataGo's customary values as the author recalls them" in doc and "not checked here" in doc
    for bad in (1, 0.25, "on", ("reduction", 0.25), {"r": 1}, {"mode": "fast"}, {"value": 2}, {"value": float("nan")},
                {"reduction": -1}, {"reduction": float("inf")}, {"root_reduction": "0"}, {"value": True}):
        with pytest.raises(ValueError, match="fpu"):
            norm(bad)


class _RecordingEngine:
    def __init__(self):
        self.calls = []

    def set_fpu(self, *a):
        self.calls.append(a)

    def clear_fpu(self):
        self.calls.append("clear")


def test_apply_sets_an_engine_once_and_a_policy_carries_the_setting(no_engines):
    from azalea_amd import fpu
    from azalea_amd.parallel_player import Player
    from azalea_amd.policy import Policy
    e = _RecordingEngine()
    fpu.apply(e, None)
    assert e.calls == []                                        # off on a fresh engine: nothing to do
    fpu.apply(e, ("reduction", 0.0, 0.25, 0.0))
    fpu.apply(e, ("reduction", 0.0, 0.25, 0.0))                 # unchanged: the statistics are not zeroed again
    fpu.apply(e, None)
    assert e.calls == [("reduction", 0.0, 0.25, 0.0), "clear"]
    p = _cpu_policy()
    assert p.fpu is None and fpu.policy_fpu(p) is None
    p.set_fpu()
    assert p.fpu == ("reduction", 0.0, 0.25, 0.0)
    p.set_fpu("off")
    assert p.fpu is None
    q = Policy()
    cfg = dict(device="cpu", network="HexNetwork", board_size=5, num_blocks=1, base_chans=32, simulations=10,
               search_batch_size=2, exploration_coef=0.5, exploration_depth=3, exploration_noise_alpha=0.3,
               exploration_noise_scale=0.25, exploration_temperature=1.0, fpu={"mode": "absolute", "value": -1})
    q.initialize(cfg)
    assert q.fpu == ("absolute", -1.0, 0.25, 0.0)
    assert "fpu" not in q.state_dict()                          # a setting of the search: checkpoints keep their format
    with pytest.raises(ValueError, match="fpu"):
        Policy().initialize(dict(cfg, fpu="sometimes"))
    # Player puts it on every agent's policy -- one agent, two agents, beside a random mover -- and refuses nonsense
    a, b = _Agent(_cpu_policy()), _Agent(_cpu_policy())
    assert Player(None, [a]).fpu is None and a.policy.fpu is None
    assert Player(None, [a, b], fpu=True).fpu == ("reduction", 0.0, 0.25, 0.0) == a.policy.fpu == b.policy.fpu
    b.policy.set_fpu("absolute")
    Player(None, [a, b])                                        # None leaves each policy's own setting
    assert a.policy.fpu[0] == "reduction" and b.policy.fpu[0] == "absolute"
    Player(None, [a, _RandomAgent()], fpu="off")
    assert a.policy.fpu[0] == "reduction"                       # off / None: nothing is pushed
    with pytest.raises(ValueError, match="fpu"):
        Player(None, [a], fpu=0.25)
    for doc in (Player.__init__.__doc__, Policy.set_fpu.__doc__):
        doc = re.sub(r"\s+", " ", doc)
        assert "NOT the reference's behaviour" in doc and "not checked here" in doc


def test_train_names_the_config_key_and_says_so_before_anything_is_built(no_engines):
    from azalea_amd import policy_trainer
    doc = re.sub(r"\s+", " ", policy_trainer.train.__doc__)
    assert 'config["fpu"]' in doc and "NOT the reference's behaviour" in doc and "not checked here" in doc
    p = _cpu_policy()
    with pytest.raises(ValueError, match=r"config\['fpu'\]: fpu"):
        policy_trainer.train(p, dict(fpu="sometimes"), "/nonexistent")


# ---- the documents -------------------------------------------------------------------------------------------------------
def test_the_documents_name_the_option_where_they_name_the_others():
    design = read("DESIGN.md")
    assert re.search(r"^\*\*7\.20 First-play urgency", design, re.M)
    sec = re.sub(r"\s+", " ", design[design.index("**7.20 First-play urgency"):])
    for phrase in ("NOT the reference's behaviour", "azx_set_fpu", "fpu = Qp - (r * sqrtf(mass))", "profiles/fpu_resources.txt",
                   "visit-dependent", "root policy temperature", "k_mcts_fpu"):
        assert phrase in sec, phrase
    readme = re.sub(r"\s+", " ", read("README.md"))
    i = readme.index("`azx_set_fpu` / `Engine.set_fpu`")
    item = readme[i:i + 4000]
    assert "First-play urgency" in item
    for phrase in ("NOT the reference's behaviour", "off by default", "outside every parity claim", "set_fpu", "NOT measured"):
        assert phrase in item, phrase
    integration = read("INTEGRATION.md")
    assert "set_fpu" in integration and 'config["fpu"]' in integration
    assert os.path.exists(os.path.join(ROOT, "profiles", "fpu_resources.txt"))
    for tool in ("bench_fpu.py", "strength_fpu.py"):
        assert os.path.exists(os.path.join(ROOT, "tools", tool)), tool
