"""The policy temperature of the search's priors (azx_set_policy_temp; NOT the reference's behaviour, off by default) on
the device.  The rule's reference is tests/policy_temp_reference.py: fpu_reference.Search with `expand_priors` and the
root's scored priors replaced by the definition of include/azx.h, pinned with (8, 8) to fpu_reference.Search and through
it to the unmodified oracle (tests/test_policy_temp_api.py).  Trees are compared through the six arrays of azx_tree_dump,
bit for bit, on never-compacted arenas (AZX_FLAG_NO_COMPACT), so node ids are the restatement's.  The evaluator of the
tree cases is fpu_reference's "skew" (non-uniform prior rows) through Engine.search_external."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import fpu_reference as fref  # noqa: E402
import policy_temp_reference as ref  # noqa: E402
import test_gpu_fpu as tgf  # noqa: E402  (helpers: tree_engine, same_dump, sorted_rows, small_net_weights, net_engine)
from fpu_reference import Settings  # noqa: E402

pytestmark = pytest.mark.gpu

SIMS = {5: 100, 9: 80, 13: 60}              # one, two and three register slots of children
BATCHES = (1, 7, 10)
ZERO = ref.ZERO_STATS
FPU_RED = ("reduction", 0.0, 0.25, 0.25)
bits = tgf.bits
same_dump = tgf.same_dump


def cfg_of(n, bs):
    return Settings(n=n, sims=SIMS[n], bs=bs, c_puct=0.5, tree_cap=1 << 17)


def positions(n):
    return ((), ref.prefix_third(n))


def add_stats(stats, zero=ZERO):
    return {k: sum(s[k] for s in stats) for k in zero}


def search(E, kind, noise=None, noise_scale=0.0):
    if kind in ref.ROW_KINDS:
        E.search_external(ref.host_evaluator(kind), noise=noise, noise_scale=noise_scale)
    else:
        E.search(noise=noise, noise_scale=noise_scale)


def engine_of(kind, cfg, G, **kw):
    return tgf.tree_engine("skew" if kind in ref.ROW_KINDS else kind, cfg, G, **kw)


def dumps_of_case(n, bs, kind, settings=ref.SETTINGS, fpu=None):
    """{(setting index, position index): tree_dump}, {setting index: policy_temp_stats} and {...: fpu_stats} of one
    engine with one slot per position."""
    cfg, pos = cfg_of(n, bs), positions(n)
    E = engine_of(kind, cfg, len(pos))
    if fpu is not None:
        E.set_fpu(*fpu)
    dumps, stats, fstats = {}, {}, {}
    for si, temp in enumerate(settings):
        E.set_policy_temp(*temp)
        assert E.policy_temp() == temp
        assert ("temp=%d/8,%d/8" % temp if temp != (8, 8) else "temp=off") in E.kernel_info()
        if fpu is not None:
            E.set_fpu(*fpu)                                     # (zeroes fpu_stats)
        E.reset(moves=[list(p) for p in pos])
        search(E, kind)
        assert (E.get_status() == 0).all()
        for g in range(len(pos)):
            dumps[(si, g)] = E.tree_dump(g)
        stats[si], fstats[si] = E.policy_temp_stats(), E.fpu_stats()
    E.close()
    return dumps, stats, fstats


def check_case(n, bs, kind, dumps, stats, settings=ref.SETTINGS, fpu=fref.OFF, fstats=None, what=""):
    pos = positions(n)
    moved = 0
    for si, temp in enumerate(settings):
        want_stats, want_fpu = [], []
        for g, prefix in enumerate(pos):
            want, st, fst = ref.tree_case(n, bs, SIMS[n], kind, temp, prefix, fpu)
            same_dump(dumps[(si, g)], want, (what, n, bs, kind, temp, prefix))
            want_stats.append(st)
            want_fpu.append(fst)
            off = ref.tree_case(n, bs, SIMS[n], kind, ref.OFF, prefix, fpu)[0]
            moved += int(off["num_nodes"] != want["num_nodes"] or not np.array_equal(off["num_visits"], want["num_visits"]))
        assert stats[si] == add_stats(want_stats), (what, temp, stats[si], add_stats(want_stats))
        if fstats is not None:
            assert fstats[si] == add_stats(want_fpu, tgf.ZERO_STATS), (what, temp)
    return moved


# ---- tree dumps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", BATCHES)
@pytest.mark.parametrize("n", sorted(SIMS))
def test_trees_are_the_restatements_bit_for_bit(n, bs):
    """Every setting of the issue, on the empty board and on a prefix of a third of the cells: the six arrays and the
    statistics, no node excluded."""
    dumps, stats, _ = dumps_of_case(n, bs, "skew")
    moved = check_case(n, bs, "skew", dumps, stats)
    for si, temp in enumerate(ref.SETTINGS):
        assert stats[si]["left_as_delivered"] == 0 and (stats[si]["tempered"] > 0) == (temp[0] != 8)
        assert stats[si]["root_searches"] == (2 if temp[1] != 8 else 0)
    print(n, bs, "searches that differ from the off rule's:", moved, "of", 2 * len(ref.SETTINGS))
    assert moved > 0                                            # the cases can tell the rule from the reference's


def test_root_noise_from_an_uploaded_array():
    """The noise is mixed into R, the tempered root priors, and the stored priors stay: 9x9, host Dirichlet rows."""
    n, bs = 9, 10
    cfg, pos = cfg_of(n, bs), positions(n)
    rng = np.random.RandomState(78)
    n_select = (cfg.sims // bs + 1) * bs
    noise = np.zeros((len(pos), n_select, cfg.cells))
    for g, prefix in enumerate(pos):
        k = cfg.cells - len(prefix)
        noise[g, :, :k] = rng.dirichlet([0.3] * k, n_select)
    E = engine_of("skew", cfg, len(pos))
    for temp in ((8, 4), (6, 7)):
        E.set_policy_temp(*temp)
        E.reset(moves=[list(p) for p in pos])
        search(E, "skew", noise=noise, noise_scale=0.25)
        for g, prefix in enumerate(pos):
            s = ref.Search(prefix, "skew", temp, cfg=cfg, noise=noise[g], noise_scale=0.25)
            same_dump(E.tree_dump(g), s.dump(), (temp, prefix))
            quiet = ref.tree_case(n, bs, cfg.sims, "skew", temp, prefix)[0]
            assert not np.array_equal(quiet["num_visits"][:60], s.dump()["num_visits"][:60])      # the noise acted
            plain = ref.Search(prefix, "skew", (temp[0], 8), cfg=cfg, noise=noise[g], noise_scale=0.25)
            assert not np.array_equal(plain.dump()["num_visits"][:60], s.dump()["num_visits"][:60])   # and so did R
    E.close()


def test_three_consecutive_plies_on_a_carried_subtree():
    """The root moves to its most-visited child twice: the new root's children keep the priors stored at their
    expansion, and R is made from them at the NEW root."""
    n, bs, temp = 9, 10, (6, 7)
    cfg, pos = cfg_of(n, bs), positions(n)
    E = engine_of("skew", cfg, len(pos))
    E.set_policy_temp(*temp)
    E.reset(moves=[list(p) for p in pos])
    refs = [ref.Search(p, "skew", temp, cfg=cfg) for p in pos]
    for ply in range(3):
        search(E, "skew")
        for g, s in enumerate(refs):
            same_dump(E.tree_dump(g), s.dump(), (ply, pos[g]))
        want = add_stats([s.temp_stats() for s in refs])
        if ply < 2:
            children = [ref.most_visited(s) for s in refs]
            E.advance(np.array(children, np.int32))
            for s, c in zip(refs, children):
                s.move_and_search(c)
    assert E.policy_temp_stats() == want and want["root_searches"] == 3 * len(pos)
    E.close()


@pytest.mark.parametrize("n", (5, 9))
def test_beside_fpu_reduction_the_visited_mass_is_of_the_stored_tempered_prior(n):
    bs, settings = 10, ((6, 8), (3, 5))
    dumps, stats, fstats = dumps_of_case(n, bs, "skew", settings, fpu=FPU_RED)
    check_case(n, bs, "skew", dumps, stats, settings, fpu=FPU_RED, fstats=fstats)
    # the mass of the delivered rows, or of R, would give other trees
    for si, temp in enumerate(settings):
        a = ref.tree_case(n, bs, SIMS[n], "skew", temp, (), FPU_RED)[0]
        b = ref.tree_case(n, bs, SIMS[n], "skew", ref.OFF, (), FPU_RED)[0]
        assert not np.array_equal(a["num_visits"], b["num_visits"])


# ---- the guard -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (5, 9))
def test_bad_rows_are_left_as_delivered_and_counted(n):
    """"skewbad": one board in three gets a row with a NaN, an inf, -0.1, 1.5 or all zeros."""
    bs, settings = 10, ((6, 8), (6, 4))
    dumps, stats, _ = dumps_of_case(n, bs, "skewbad", settings)
    check_case(n, bs, "skewbad", dumps, stats, settings)
    for si in range(len(settings)):
        assert stats[si]["left_as_delivered"] > 0 and stats[si]["tempered"] > 0, stats[si]


# ---- table-prior evaluators -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("uniform", "hash"))
def test_table_prior_evaluators_are_untouched(kind):
    from azalea_amd import engine as eng
    out = []
    for temp in (None, (6, 4), (1, 1)):
        E = eng.Engine(board_size=5, n_games=64, simulations=40, search_batch_size=4, exploration_coef=0.5,
                       exploration_depth=2, noise_alpha=0.3, noise_scale=0.25, temperature=1.0, seed=11,
                       evaluator=eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH)
        if temp is not None:
            E.set_policy_temp(*temp)
        info = E.kernel_info().split("; temp=")[0]
        E.reset()
        E.search()
        tree = {k: np.asarray(v).tobytes() for k, v in E.tree_dump(3).items()}
        E.reset()
        rows, st = E.play(200)
        played = tgf.sorted_rows(rows, E.play_row_metrics())
        out.append((info, tree, played, {k: v for k, v in st.items() if not k.endswith("seconds")},
                    E.debug_counters().tobytes()))
        assert E.policy_temp_stats() == ZERO
        E.close()
    assert out[0] == out[1] and out[0] == out[2]


# ---- the network path ------------------------------------------------------------------------------------------------------
def net_engine(n, G, w, **kw):
    conf = dict(board_size=n, sims=30, bs=6)
    conf.update(kw)
    return tgf.net_engine(G, w, **conf)


def root_priors(E, g=0):
    r = E.get_root()
    k = int(r["k"][g])
    return r["child_prior"][g, :k].copy(), r["legal_moves"][g, :k].copy()


@pytest.mark.parametrize("n", (5, 9))
def test_the_networks_row_is_stored_tempered(n):
    """A seeded 1x16 network.  Off: the root children's stored priors are the network's row -- exp of Engine.forward's
    log-probabilities; the search's heads kernel takes expf(x - lse) on the device and forward() the log-softmax on
    the host, so the two agree to rounding, not to the bit -- and with (6, 8) they are azx_policy_temp_row of the
    stored off row, bit for bit."""
    from azalea_amd import engine as eng
    w = tgf.small_net_weights(n=n)
    rows = {}
    for temp in ((8, 8), (6, 8), (8, 4)):
        E = net_engine(n, 2, w, noise_scale=0.0, flags=eng.FLAG_NO_COMPACT, nodes_per_game=1 << 15)
        if temp != (8, 8):
            E.set_policy_temp(*temp)
        E.reset()
        E.search()
        rows[temp], lm = root_priors(E)
        if temp == (8, 8):
            _, logprob = E.forward(np.zeros((1, n, n), np.int32), lm[None, :])
            assert np.allclose(rows[temp], np.exp(logprob[0].astype(np.float64)), rtol=1e-5, atol=1e-9)
            assert E.policy_temp_stats() == ZERO
        else:
            st = E.policy_temp_stats()
            assert st["left_as_delivered"] == 0 and (st["tempered"] > 0) == (temp[0] != 8)
        E.close()
    want, done = eng.policy_temp_row(6, rows[(8, 8)])
    assert done and np.array_equal(bits(rows[(6, 8)]), bits(want))
    assert ref.entropy(want) > ref.entropy(rows[(8, 8)])
    assert np.array_equal(bits(rows[(8, 4)]), bits(rows[(8, 8)]))      # the root rule does not rewrite the stored priors


CTR_EVALS, CTR_TERM_EVALS = 4, 5


def test_selfplay_is_deterministic_pipeline_independent_and_counts_every_expansion(monkeypatch):
    """256 games of the 1x16 network on 5x5, twice from one seed and once with AZX_PIPELINE=0: the same bytes.  Every
    evaluation request of a non-terminal position (CTR_EVALS; terminal leaves are CTR_TERM_EVALS and ask for none) is
    applied by an expansion from its row before play() returns, and with eighths != 8 every such expansion is either
    tempered or left as delivered: stats[0] + stats[1] == CTR_EVALS exactly (root_eighths = 8: no root rows in [1])."""
    w = tgf.small_net_weights()
    out = []
    for run in ("first", "second", "one stream"):
        if run == "one stream":
            monkeypatch.setenv("AZX_PIPELINE", "0")            # (read by azx_create)
        E = tgf.net_engine(256, w)
        E.set_policy_temp(6, 8)
        rows, st = E.play(1200)
        stats, ctr = E.policy_temp_stats(), E.debug_counters()
        out.append(tgf.sorted_rows(rows, E.play_row_metrics()))
        E.close()
        print(run, {k: st[k] for k in ("plies", "selects", "evals", "games")}, stats, ctr[:6])
        assert st["games"] > 0 and stats["tempered"] > 0 and stats["root_searches"] == 0
        assert stats["tempered"] + stats["left_as_delivered"] == int(ctr[CTR_EVALS]), (stats, ctr[:6])
        assert int(ctr[CTR_TERM_EVALS]) > 0
    assert out[0] == out[1]
    assert out[0] == out[2]


# ---- beside forced playouts, and beside the Gumbel root search -----------------------------------------------------------
# Both act in play-mode launches only.  There the "skew" rows come from a REGISTERED device evaluator
# (Engine.set_external_evaluator; policy_temp_reference.skew_device_evaluator), and the device's first rows are compared
# with restatements that compose the rules, the way tests/test_gpu_fpu.py composes them with first-play urgency.
def test_the_device_skew_evaluator_is_the_host_one():
    """The registered evaluator hands the search the host evaluator's rows: the same trees, bit for bit."""
    import torch
    cfg, pos = cfg_of(5, 10), positions(5)
    dumps = []
    for device in (False, True):
        E = engine_of("skew", cfg, len(pos))
        E.set_policy_temp(6, 4)
        E.reset(moves=[list(p) for p in pos])
        if device:
            E.set_external_evaluator(ref.skew_device_evaluator(torch.device("cuda", 0)))
            E.search()
        else:
            search(E, "skew")
        dumps.append([E.tree_dump(g) for g in range(len(pos))])
        E.close()
    for g, prefix in enumerate(pos):
        same_dump(dumps[1][g], dumps[0][g], prefix)
        same_dump(dumps[1][g], ref.tree_case(5, 10, SIMS[5], "skew", (6, 4), prefix)[0], prefix)


@pytest.mark.parametrize("temp", ((6, 4), (8, 4)))
def test_forced_playouts_read_the_tempered_root_priors(temp):
    """(k * Ps) * S is made from R = temper(stored priors, root_eighths): the visit counts of the first row and the
    forced selects are the composed restatement's, and not those of a restatement whose forced set reads the stored
    priors (root_eighths = 8)."""
    import forced_playouts_reference as fp
    import test_gpu_forced_playouts as tfp
    import torch
    from azalea_amd import engine as eng
    prefixes = fp.prefixes("hash")[:16]
    refs = [ref.Search(p, "skew", temp, forced_k=fp.K_FORCED) for p in prefixes]
    stored = [ref.Search(p, "skew", (temp[0], 8), forced_k=fp.K_FORCED) for p in prefixes]
    assert any(not np.array_equal(a.n, b.n) for a, b in zip(refs, stored))     # R changes what is forced
    E = tfp.make(eng.EVAL_EXTERNAL, len(prefixes))
    E.set_external_evaluator(ref.skew_device_evaluator(torch.device("cuda", 0)))
    E.set_train_targets("visits")
    E.set_forced_playouts(fp.K_FORCED, False)
    E.set_policy_temp(*temp)
    got, stats = tfp.first_rows(E, prefixes)
    E.close()
    for (row, m), r in zip(got, refs):
        k, S = len(r.n), tfp.raw_sum(m)
        assert S == int(r.n.sum()), (r.forced_at, S)
        assert np.array_equal(np.rint(row[:k].astype(np.float64) * S), r.n), (row[:k] * S, r.n)
    assert stats["forced_selects"] == sum(r.forced for r in refs) > 0


@pytest.mark.parametrize("temp", ((6, 4), (8, 4)))
def test_the_gumbel_root_search_reads_the_stored_tempered_priors(temp):
    """The candidates' ln P and sigma's prior-weighted mean are of the STORED priors -- tempered at the root's
    expansion with eighths -- and root_eighths is unused: (8, 4) is the run with the option off."""
    import gumbel_reference as gr
    import test_gpu_gumbel as tgg
    import torch
    from azalea_amd import engine as eng
    setup = gr.SETUP["m8_200"]
    prefixes = gr.prefixes_of(setup, "hash")[:16]
    G = len(prefixes)
    kw = dict(m=setup.m, seed=gr.SEED, cfg=setup.cfg)
    refs = [ref.GumbelSearch(p, "skew", temp, uid=G + g, **kw) for g, p in enumerate(prefixes)]
    plain = [ref.GumbelSearch(p, "skew", ref.OFF, uid=G + g, **kw) for g, p in enumerate(prefixes)]
    differs = any(not np.array_equal(a.n, b.n) or list(a.candidates) != list(b.candidates) for a, b in zip(refs, plain))
    assert differs == (temp[0] != 8)                            # an untempered ln P would give the plain run
    E = tgg.make(eng.EVAL_EXTERNAL, G, setup.cfg)
    E.set_external_evaluator(ref.skew_device_evaluator(torch.device("cuda", 0)))
    E.set_train_targets("visits")
    E.set_gumbel(setup.m, setup.c_visit, setup.c_scale, improved_rows=False)
    E.set_policy_temp(*temp)
    got, state, stats = tgg.first_rows(E, prefixes, setup.cfg)
    pstats = E.policy_temp_stats()
    E.close()
    cand, surv = state
    safe = 0
    for g, ((row, m, cell), r) in enumerate(zip(got, refs)):
        if not r.safe:
            continue
        safe += 1
        k, S = len(r.n), tgg.raw_sum(m)
        assert S == int(r.n.sum()), (prefixes[g], S)
        assert np.array_equal(np.rint(row[:k].astype(np.float64) * S), r.n), (prefixes[g], row[:k] * S, r.n)
        assert np.array_equal(cand[g], gr.mask_words(r.candidates)) and np.array_equal(surv[g], gr.mask_words(r.survivors))
    assert safe >= (1.0 - gr.MAX_UNSAFE_SHARE) * G
    assert stats["root_selects"] == sum(r.root_selects for r in refs)
    assert pstats["root_searches"] == 0 and (pstats["tempered"] > 0) == (temp[0] != 8)


# ---- a row that sums far above 1, and the rollout evaluator ---------------------------------------------------------------
def test_rows_of_ones_on_13x13_put_z_past_two_to_the_31():
    """"skewones": one board in three delivers a row of ones.  It passes the guard and is tempered: Z = k * 2^24, above
    2^31 for k >= 128 -- an unsigned sum."""
    n, bs, settings = 13, 10, ((6, 8), (4, 4))
    dumps, stats, _ = dumps_of_case(n, bs, "skewones", settings)
    check_case(n, bs, "skewones", dumps, stats, settings)
    for si in range(len(settings)):
        assert stats[si]["left_as_delivered"] == 0 and stats[si]["tempered"] > 0
    wide = sum(int((d["prior_prob"] == np.float32(1.0) / np.float32(k)).sum()) for d in dumps.values() for k in range(128, 170))
    assert wide >= 128                                          # rows of ones at least 128 wide were stored as 1/k each


def test_the_rollout_evaluator_is_untouched():
    """The rollout evaluator hands every child one table prior through the external path: while it is registered the
    setting in force is (8, 8), and self-play is the bytes of the engine that never set the option."""
    from azalea_amd import engine as eng
    out = []
    for temp in (None, (6, 4)):
        E = eng.Engine(board_size=5, n_games=64, simulations=40, search_batch_size=4, exploration_coef=0.5,
                       exploration_depth=2, noise_alpha=0.3, noise_scale=0.25, temperature=1.0, seed=11,
                       evaluator=eng.EVAL_EXTERNAL)
        if temp is not None:
            E.set_policy_temp(*temp)
        E.set_rollout_evaluator(16, seed=5)
        info = E.kernel_info()
        assert "k_mcts_pt" not in info and "eval=rollout(16)" in info
        assert info.endswith("; temp=6/8,4/8" if temp else "; temp=off")      # the setting as made stays readable
        rows, st = E.play(300)
        out.append((tgf.sorted_rows(rows, E.play_row_metrics()), {k: v for k, v in st.items() if not k.endswith("seconds")},
                    E.debug_counters().tobytes()))
        assert E.policy_temp_stats() == ZERO and E.policy_temp() == (temp or (8, 8))
        E.close()
    assert out[0] == out[1]


# ---- the other instantiations, each in a fresh process -----------------------------------------------------------------
CHILD_CASES = [(5, 7), (9, 10), (13, 7)]
CHILD_SETTINGS = ((6, 8), (3, 5))


def child(out):
    dump = {}
    for n, bs in CHILD_CASES:
        dumps, stats, _ = dumps_of_case(n, bs, "skew", CHILD_SETTINGS)
        for (si, g), d in dumps.items():
            for name, v in d.items():
                dump["t_%d_%d_%d_%d_%s" % (n, bs, si, g, name)] = np.asarray(v)
        for si, s in stats.items():
            dump["s_%d_%d_%d" % (n, bs, si)] = np.array([s[k] for k in ZERO], np.int64)
    E = tgf.net_engine(64, tgf.small_net_weights())
    E.set_policy_temp(6, 4)
    info = E.kernel_info()
    for k, v in tgf.pool_dump(E, 6).items():
        dump["p_%s" % k] = v
    dump["p_temp"] = np.array([E.policy_temp_stats()[k] for k in ZERO], np.int64)
    E.close()
    np.savez(out, info=np.array([info]), **dump)


def run_child(tmp_path, name, extra_env):
    out = str(tmp_path / (name + ".npz"))
    env = dict(os.environ, **extra_env)
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "child", out]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=270)
    assert r.returncode == 0, (name, r.returncode, r.stderr.decode()[-2000:])
    return dict(np.load(out))


def test_the_generic_and_the_per_move_paths_agree(tmp_path):
    """AZX_MCTS_GENERIC=1 and AZX_NO_PERSISTENT=1, each in a fresh child process: the same trees as the restatement, and
    the same pool after six plies of network self-play under (6, 4) as a third child with neither switch."""
    runs = {name: run_child(tmp_path, name, env) for name, env in
            (("default", {}), ("generic", {"AZX_MCTS_GENERIC": "1"}), ("no_persistent", {"AZX_NO_PERSISTENT": "1"}))}
    infos = {name: str(d.pop("info")[0]) for name, d in runs.items()}
    assert "AZX_MCTS_GENERIC=1" in infos["generic"] and "AZX_NO_PERSISTENT=1" in infos["no_persistent"], infos
    assert all(i.endswith("; temp=6/8,4/8") and "tree=k_mcts_pt<2>" in i for i in infos.values()), infos
    for name, d in runs.items():
        for n, bs in CHILD_CASES:
            dumps, stats = {}, {}
            for si in range(len(CHILD_SETTINGS)):
                for g in range(2):
                    pre = "t_%d_%d_%d_%d_" % (n, bs, si, g)
                    got = {k[len(pre):]: v for k, v in d.items() if k.startswith(pre)}
                    got["num_nodes"], got["root_id"] = int(got["num_nodes"]), int(got["root_id"])
                    dumps[(si, g)] = got
                stats[si] = dict(zip(ZERO, (int(x) for x in d["s_%d_%d_%d" % (n, bs, si)])))
            check_case(n, bs, "skew", dumps, stats, CHILD_SETTINGS, what=name)
    pool = {name: {k: v for k, v in d.items() if k.startswith("p_")} for name, d in runs.items()}
    for name in ("generic", "no_persistent"):
        assert pool[name].keys() == pool["default"].keys()
        for k, v in pool["default"].items():
            assert v.tobytes() == pool[name][k].tobytes(), (name, k)
    assert int(pool["default"]["p_play"][0]) == 6 * 64 and int(pool["default"]["p_temp"][0]) > 0


# ---- never set, and set then cleared -----------------------------------------------------------------------------------------
def test_off_means_off():
    """After setting and then clearing the option, searches and 64 self-play games give the never-set bytes."""
    w = tgf.small_net_weights()
    out = []
    for how in ("never", "cleared", "eights"):
        E = tgf.net_engine(64, w)
        if how == "cleared":
            E.set_policy_temp(4, 4)
            assert E.policy_temp() == (4, 4) and "temp=4/8,4/8" in E.kernel_info() and "tree=k_mcts_pt<2>" in E.kernel_info()
            E.clear_policy_temp()
        elif how == "eights":
            E.set_policy_temp(6, 8)
            E.set_policy_temp(8, 8)
        assert E.policy_temp() == (8, 8)
        info = E.kernel_info()
        assert info.endswith("; temp=off") and "tree=k_mcts<2,generic>" in info
        E.reset()
        E.search()
        tree = {k: np.asarray(v).tobytes() for k, v in E.get_root().items()}
        E.reset()
        rows, st = E.play(1200)
        assert st["games"] >= 64
        played = tgf.sorted_rows(rows, E.play_row_metrics())
        out.append((info, tree, played, {k: v for k, v in st.items() if not k.endswith("seconds")},
                    E.debug_counters().tobytes()))
        assert E.policy_temp_stats() == ZERO
        E.close()
    assert out[0] == out[1] and out[0] == out[2]


# ---- a Match and a three-engine Tournament ---------------------------------------------------------------------------------
def match_engines(w, on, G=32):
    engines = [tgf.net_engine(G, w, seed=(7 + a) << 32, sims=24, bs=6) for a in range(3)]
    if on:
        engines[0].set_policy_temp(6, 4)
    return engines


def test_a_match_takes_an_engine_with_the_option_beside_one_without():
    from azalea_amd import engine as eng
    w = tgf.small_net_weights()
    runs = {}
    for name, on in (("mixed", True), ("again", True), ("off", False)):
        a, b, spare = match_engines(w, on)
        spare.close()
        m = eng.Match(a, b)
        res = m.play(32, moves=True)
        runs[name] = (res, a.policy_temp_stats(), b.policy_temp_stats())
        m.close()
        a.close()
        b.close()
    res, sa, sb = runs["mixed"]
    assert res["stats"]["games"] == 32 and res["stats"]["voided"] == 0
    assert sa["tempered"] > 0 and sa["root_searches"] > 0 and sb == ZERO
    assert runs["off"][1] == ZERO and runs["off"][2] == ZERO
    for k in ("outcome", "length", "moves"):
        assert np.array_equal(res[k], runs["again"][0][k]), k
    assert sa == runs["again"][1]
    assert not np.array_equal(res["moves"], runs["off"][0]["moves"])            # the option acted


def test_a_tournament_takes_one_engine_with_the_option_among_three():
    from azalea_amd import engine as eng
    w = tgf.small_net_weights()
    pairs, rounds = [(0, 1), (0, 2), (1, 2)], 12
    runs = {}
    for name, on in (("mixed", True), ("again", True), ("off", False)):
        engines = match_engines(w, on)
        t = eng.Tournament(engines)
        res = t.play(pairs, rounds, moves=True)
        runs[name] = (res, [e.policy_temp_stats() for e in engines])
        t.close()
        for e in engines:
            e.close()
    res, stats = runs["mixed"]
    assert stats[0]["tempered"] > 0 and stats[1] == ZERO and stats[2] == ZERO
    assert runs["off"][1] == [ZERO] * 3 and stats == runs["again"][1]
    for pair in pairs:
        assert res[pair]["stats"]["games"] == rounds and res[pair]["stats"]["voided"] == 0
        for k in ("outcome", "length", "moves"):
            assert np.array_equal(res[pair][k], runs["again"][0][pair][k]), (pair, k)
    for k in ("outcome", "length", "moves"):                    # the pair of two option-off engines plays the all-off games
        assert np.array_equal(res[(1, 2)][k], runs["off"][0][(1, 2)][k]), k
    assert any(not np.array_equal(res[p]["moves"], runs["off"][0][p]["moves"]) for p in pairs[:2])


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_set_during_a_phase_api_search_is_estate_and_bad_values_are_einval():
    from azalea_amd._lib import AzxError
    cfg = cfg_of(5, 10)
    E = engine_of("skew", cfg, 1)
    L = E.L
    E.set_policy_temp(6, 7)
    for bad in ((0, 8), (9, 8), (6, 0), (6, 9), (-1, 8), (6, 100)):
        assert L.azx_set_policy_temp(E.h, *bad) == -1 and b"policy temperature" in L.azx_last_error(), bad
        assert E.policy_temp() == (6, 7)                        # EINVAL keeps the setting
    assert L.azx_set_policy_temp(None, 6, 8) == -1 and L.azx_policy_temp_stats(E.h, None) == -1
    E.reset(moves=[[]])
    evaluate = ref.host_evaluator("skew")
    n = E.search_begin()
    with pytest.raises(AzxError, match=r"azx error -4.*phase-API search"):
        E.set_policy_temp(4, 8)
    with pytest.raises(AzxError, match=r"azx error -4"):
        E.clear_policy_temp()
    assert E.policy_temp() == (6, 7)
    while True:                                                 # the search goes on, under the setting it began with
        if n:
            b, lm, slot, k = E.get_leaves()
            E.put_evals(*evaluate(b, lm, slot, k))
        n, done = E.search_step()
        if done:
            break
    same_dump(E.tree_dump(0), ref.tree_case(5, 10, cfg.sims, "skew", (6, 7), ())[0], "after the refusals")
    E.set_policy_temp(4, 8)                                     # between searches it is accepted again
    assert E.policy_temp() == (4, 8) and E.policy_temp_stats() == ZERO
    E.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        child(sys.argv[2])
