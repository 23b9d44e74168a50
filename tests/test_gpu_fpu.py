"""First-play urgency (azx_set_fpu; NOT the reference's behaviour, off by default) on the device.  The rule's reference
is tests/fpu_reference.py: the numpy float32 restatement of the oracle's search with `pick` replaced by the definition of
include/azx.h, pinned to the unmodified oracle with the rule off (tests/test_fpu_api.py).  Trees are compared through the
six arrays of azx_tree_dump, bit for bit, on never-compacted arenas (AZX_FLAG_NO_COMPACT), so node ids are the
restatement's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import fpu_reference as ref  # noqa: E402
from fpu_reference import Settings  # noqa: E402

pytestmark = pytest.mark.gpu

ESTATE = -4
SIMS = {5: 100, 11: 60, 13: 40}             # one, two and three mask words of children
BATCHES = (1, 7, 10)
ROW_KEYS = ("board", "color", "nlegal", "moves_prob", "reward", "game_uid")
ZERO_STATS = dict(selects=0, levels_with_unvisited=0, ended_unvisited=0, differs_from_off=0)
REDUCTION = ("reduction", 0.0, 0.25, 0.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cfg_of(n, bs):
    return Settings(n=n, sims=SIMS[n], bs=bs, c_puct=0.5, tree_cap=1 << 17)


def positions(n):
    return ((), ref.prefix_third(n))


def tree_engine(kind, cfg, G, **kw):
    """An engine whose trees can be compared node for node: a never-compacted arena, no noise unless asked for."""
    from azalea_amd import engine as eng
    evaluator = {"uniform": eng.EVAL_UNIFORM, "hash": eng.EVAL_UNIFORM_HASH, "skew": eng.EVAL_EXTERNAL}[kind]
    conf = dict(board_size=cfg.n, n_games=G, simulations=cfg.sims, search_batch_size=cfg.bs, exploration_coef=cfg.c_puct,
                exploration_depth=0, noise_alpha=0.3, noise_scale=0.0, temperature=1.0, seed=4242,
                nodes_per_game=1 << 17, flags=eng.FLAG_NO_COMPACT)
    conf.update(kw)
    E = eng.Engine(evaluator=evaluator, **conf)
    if kind == "hash":
        E.set_prior_table(cfg.table)
    return E


def search(E, kind, noise=None, noise_scale=0.0):
    if kind == "skew":
        E.search_external(ref.skew_host_evaluator(), noise=noise, noise_scale=noise_scale)
    else:
        E.search(noise=noise, noise_scale=noise_scale)


def same_dump(got, want, what):
    assert got["num_nodes"] == want["num_nodes"] and got["root_id"] == want["root_id"], \
        (what, got["num_nodes"], want["num_nodes"], got["root_id"], want["root_id"])
    for name in ("parent", "first_child", "num_children"):
        assert np.array_equal(got[name], want[name]), (what, name)
    for name in ("num_visits", "total_value", "prior_prob"):
        assert np.array_equal(bits(got[name]), bits(want[name])), (what, name)


def add_stats(stats):
    return {k: sum(s[k] for s in stats) for k in ZERO_STATS}


def dumps_of_case(n, bs, kind, modes=ref.MODES):
    """{(mode index, position index): tree_dump} and {mode index: fpu_stats} of one engine with one slot per position."""
    cfg, pos = cfg_of(n, bs), positions(n)
    E = tree_engine(kind, cfg, len(pos))
    dumps, stats = {}, {}
    for mi, mode in enumerate(modes):
        E.set_fpu(*mode)
        got = E.fpu()
        assert (got["mode"], got["value"], got["reduction"], got["root_reduction"]) == mode
        E.reset(moves=[list(p) for p in pos])
        search(E, kind)
        assert (E.get_status() == 0).all()
        for g in range(len(pos)):
            dumps[(mi, g)] = E.tree_dump(g)
        stats[mi] = E.fpu_stats()
    E.close()
    return dumps, stats


# ---- (a) tree parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
@pytest.mark.parametrize("bs", BATCHES)
@pytest.mark.parametrize("n", sorted(SIMS))
def test_trees_are_the_restatements_bit_for_bit(n, bs, kind):
    """Every mode of the issue, on the empty board and on a prefix of a third of the cells: the six arrays and the
    statistics.  "uniform" runs the FAST instantiations, "hash" the generic ones, "skew" -- non-uniform priors, so the
    visited mass is not a multiple of 1/k -- the phase API through Engine.search_external."""
    dumps, stats = dumps_of_case(n, bs, kind)
    pos = positions(n)
    moved = 0
    for mi, mode in enumerate(ref.MODES):
        want_stats = []
        for g, prefix in enumerate(pos):
            want, st = ref.tree_case(n, bs, SIMS[n], kind, mode, prefix)
            same_dump(dumps[(mi, g)], want, (n, bs, kind, mode, prefix))
            want_stats.append(st)
            off, _ = ref.tree_case(n, bs, SIMS[n], kind, ref.OFF, prefix)
            moved += int(off["num_nodes"] != want["num_nodes"] or not np.array_equal(off["num_visits"], want["num_visits"]))
        assert stats[mi] == add_stats(want_stats), (mode, stats[mi], add_stats(want_stats))
        assert stats[mi]["selects"] == len(pos) * (SIMS[n] // bs + 1) * bs
    print(n, bs, kind, "searches that differ from the OFF rule's:", moved, "of", len(ref.MODES) * len(pos))
    assert moved > 0                                            # the cases can tell the rule from the reference's


def test_root_noise_from_an_uploaded_array():
    """The noise mix at the root is untouched, and the mass uses the STORED prior: 11x11, "hash", host Dirichlet rows."""
    n, bs = 11, 10
    cfg, pos = cfg_of(n, bs), positions(n)
    rng = np.random.RandomState(77)
    n_select = (cfg.sims // bs + 1) * bs
    noise = np.zeros((len(pos), n_select, cfg.cells))
    for g, prefix in enumerate(pos):
        k = cfg.cells - len(prefix)
        noise[g, :, :k] = rng.dirichlet([0.3] * k, n_select)
    E = tree_engine("hash", cfg, len(pos))
    for mode in (ref.MODES[3], ref.MODES[1]):
        E.set_fpu(*mode)
        E.reset(moves=[list(p) for p in pos])
        E.search(noise=noise, noise_scale=0.25)
        for g, prefix in enumerate(pos):
            s = ref.Search(prefix, "hash", mode, cfg=cfg, noise=noise[g], noise_scale=0.25)
            same_dump(E.tree_dump(g), s.dump(), (mode, prefix))
            quiet = ref.tree_case(n, bs, cfg.sims, "hash", mode, prefix)[0]
            assert not np.array_equal(quiet["num_visits"][:50], s.dump()["num_visits"][:50])     # the noise acted
    E.close()


@pytest.mark.parametrize("kind,n", [("hash", 5), ("skew", 11)])
def test_three_consecutive_plies_on_a_carried_subtree(kind, n):
    """The root moves to its most-visited child twice: the new root's own Q (Qp at the root) comes from the visits and
    values it collected as a child, and root_reduction holds at the NEW root."""
    bs = 10
    cfg, pos = cfg_of(n, bs), positions(n)
    mode = ref.MODES[3]                                         # reduction 0.5 below the root, 0.5 at it
    E = tree_engine(kind, cfg, len(pos))
    E.set_fpu(*mode)
    E.reset(moves=[list(p) for p in pos])
    refs = [ref.Search(p, kind, mode, cfg=cfg) for p in pos]
    want_stats = ZERO_STATS
    for ply in range(3):
        search(E, kind)
        for g, s in enumerate(refs):
            same_dump(E.tree_dump(g), s.dump(), (kind, n, ply, pos[g]))
        want_stats = add_stats([s.stats() for s in refs])
        if ply < 2:
            children = [ref.most_visited(s) for s in refs]
            E.advance(np.array(children, np.int32))
            for s, c in zip(refs, children):
                s.move_and_search(c)
    assert E.fpu_stats() == want_stats
    E.close()


# ---- (b) the other instantiations, each in a fresh process ---------------------------------------------------------------
CHILD_CASES = [(n, bs, kind) for n in sorted(SIMS) for bs in (7, 10) for kind in ("uniform", "hash")]


def pool_dump(E, plies):
    st = E.play_steps(plies)
    games, root = E.get_games(), E.get_root()
    out = {"game_" + k: v for k, v in games.items()}
    out.update({"root_" + k: v for k, v in root.items()})
    out["counters"] = E.debug_counters()[:10]
    out["play"] = np.array([st[k] for k in ("plies", "selects", "evals", "sum_depth", "positions", "games")], np.int64)
    return out


def child(out):
    """What test_the_generic_and_the_per_move_instantiations_agree compares: the trees of CHILD_CASES and six plies of a
    64-game 5x5 pool under REDUCTION, from whatever instantiations this process's environment selects."""
    from azalea_amd import engine as eng
    dump = {}
    infos = []
    for n, bs, kind in CHILD_CASES:
        dumps, stats = dumps_of_case(n, bs, kind)
        for (mi, g), d in dumps.items():
            for name, v in d.items():
                dump["t_%d_%d_%s_%d_%d_%s" % (n, bs, kind, mi, g, name)] = np.asarray(v)
        for mi, s in stats.items():
            dump["s_%d_%d_%s_%d" % (n, bs, kind, mi)] = np.array([s[k] for k in ZERO_STATS], np.int64)
    for n in (5, 13):
        E = eng.Engine(board_size=n, n_games=64, simulations=40, search_batch_size=8, exploration_coef=0.5,
                       exploration_depth=4, noise_alpha=0.3, noise_scale=0.25, temperature=1.0, seed=99,
                       evaluator=eng.EVAL_UNIFORM)
        E.set_fpu(*REDUCTION)
        infos.append(E.kernel_info())
        for k, v in pool_dump(E, 6).items():
            dump["p%d_%s" % (n, k)] = v
        dump["p%d_fpu" % n] = np.array([E.fpu_stats()[k] for k in ZERO_STATS], np.int64)
        E.close()
    np.savez(out, info=np.array(infos), **dump)


def run_child(tmp_path, name, extra_env):
    out = str(tmp_path / (name + ".npz"))
    env = dict(os.environ, **extra_env)
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "child", out]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=270)
    assert r.returncode == 0, (name, r.returncode, r.stderr.decode()[-2000:])
    return dict(np.load(out))


def test_the_generic_and_the_per_move_instantiations_agree(tmp_path):
    """AZX_MCTS_GENERIC=1 (every tree launch on the generic instantiation) and AZX_NO_PERSISTENT=1 (per-move launches in
    place of the persistent play loop), each in a fresh child process: the same trees as the restatement, and the same
    pool after six plies of self-play under REDUCTION as a third child with neither switch."""
    runs = {name: run_child(tmp_path, name, env) for name, env in
            (("default", {}), ("generic", {"AZX_MCTS_GENERIC": "1"}), ("no_persistent", {"AZX_NO_PERSISTENT": "1"}))}
    infos = {name: [str(x) for x in d.pop("info")] for name, d in runs.items()}
    assert all("k_play<2> (persistent)" in infos["default"][0] and "FAST" in i for i in infos["default"]), infos["default"]
    assert all("generic" in i and "FAST" not in i for i in infos["generic"]), infos["generic"]
    assert all("per move" in i and "(persistent)" not in i for i in infos["no_persistent"]), infos["no_persistent"]
    for name, d in runs.items():
        for n, bs, kind in CHILD_CASES:
            for mi, mode in enumerate(ref.MODES):
                want_stats = []
                for g, prefix in enumerate(positions(n)):
                    want, st = ref.tree_case(n, bs, SIMS[n], kind, mode, prefix)
                    pre = "t_%d_%d_%s_%d_%d_" % (n, bs, kind, mi, g)
                    got = {k[len(pre):]: v for k, v in d.items() if k.startswith(pre)}
                    got["num_nodes"], got["root_id"] = int(got["num_nodes"]), int(got["root_id"])
                    same_dump(got, want, (name, n, bs, kind, mode, prefix))
                    want_stats.append(st)
                want = add_stats(want_stats)
                assert list(d["s_%d_%d_%s_%d" % (n, bs, kind, mi)]) == [want[k] for k in ZERO_STATS], (name, n, bs, kind, mode)
    pool = {name: {k: v for k, v in d.items() if k[0] == "p"} for name, d in runs.items()}
    for name in ("generic", "no_persistent"):
        assert pool[name].keys() == pool["default"].keys()
        for k, v in pool["default"].items():
            assert v.tobytes() == pool[name][k].tobytes(), (name, k)
    for n in (5, 13):
        assert int(pool["default"]["p%d_play" % n][0]) == 6 * 64
        assert int(pool["default"]["p%d_fpu" % n][0]) == int(pool["default"]["p%d_play" % n][1]) > 0     # selects


# ---- (c) never set, and set then cleared -----------------------------------------------------------------------------------
def sorted_rows(rows, m):
    i = np.argsort(rows["game_uid"], kind="stable")       # finished games enter the queue in the order the GPU finished them
    return {k: rows[k][i].tobytes() for k in ROW_KEYS}, m[i].tobytes()


@pytest.mark.parametrize("kind", ("uniform", "hash"))
def test_the_option_never_set_or_cleared_leaves_no_trace(kind):
    from azalea_amd import engine as eng
    out = []
    for how in ("never", "cleared", "off"):
        E = eng.Engine(board_size=5, n_games=64, simulations=40, search_batch_size=4, exploration_coef=0.5,
                       exploration_depth=2, noise_alpha=0.3, noise_scale=0.25, temperature=1.0, seed=11,
                       evaluator=eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH)
        if how == "cleared":
            E.set_fpu(*REDUCTION)
            assert E.fpu()["mode"] == "reduction"
            E.clear_fpu()
        elif how == "off":
            E.set_fpu("absolute", 0.5)
            E.set_fpu("off", 0.7, 3.0, 4.0)                     # OFF stores zeros, whatever came with it
        assert E.fpu() == dict(mode="off", value=0.0, reduction=0.0, root_reduction=0.0)
        info = E.kernel_info()
        E.reset()
        E.search()
        tree = {k: np.asarray(v).tobytes() for k, v in E.tree_dump(3).items()}
        E.reset()
        rows, st = E.play(200)
        played = sorted_rows(rows, E.play_row_metrics())
        steps = E.play_steps(5)
        out.append((info, tree, played, {k: v for k, v in st.items() if not k.endswith("seconds")},
                    {k: v for k, v in steps.items() if not k.endswith("seconds")}, E.debug_counters().tobytes()))
        assert E.fpu_stats() == ZERO_STATS
        E.close()
    assert out[0] == out[1] and out[0] == out[2]


# ---- (d) throughput self-play with REDUCTION ---------------------------------------------------------------------------------
def small_net_weights(n=5, blocks=1, chans=16, seed=3):
    from azalea_amd.network import HexNetwork
    torch.manual_seed(seed)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).eval()
    return {k: v.detach().numpy() for k, v in net.state_dict().items() if v.dtype.is_floating_point}


def net_engine(G, w, seed=2024, sims=30, bs=6, **kw):
    from azalea_amd import engine as eng
    conf = dict(board_size=5, n_games=G, simulations=sims, search_batch_size=bs, exploration_coef=0.5, exploration_depth=3,
                noise_alpha=0.3, noise_scale=0.25, temperature=1.0, seed=seed, num_blocks=1, base_chans=16)
    conf.update(kw)
    E = eng.Engine(evaluator=eng.EVAL_RESNET, **conf)
    E.set_weights(w)
    return E


def test_selfplay_under_reduction_is_deterministic_and_pipeline_independent(monkeypatch):
    """1 024 games (the smallest pool the two half-pools accept) of a 1x16 network on 5x5: two runs from one seed give the
    same rows; AZX_PIPELINE=0 gives them too; fpu_stats counts exactly the run's selects."""
    w = small_net_weights()
    out, infos = [], []
    for run in ("first", "second", "one stream"):
        if run == "one stream":
            monkeypatch.setenv("AZX_PIPELINE", "0")            # (read by azx_create)
        E = net_engine(1024, w)
        E.set_fpu(*REDUCTION)
        infos.append(E.kernel_info())
        rows, st = E.play(3000)
        stats = E.fpu_stats()
        out.append(sorted_rows(rows, E.play_row_metrics()))
        E.close()
        print(run, {k: st[k] for k in ("plies", "selects", "evals", "games")}, stats)
        assert st["games"] > 0 and stats["selects"] == st["selects"] > 0
        assert 0 < stats["ended_unvisited"] <= stats["selects"] and stats["levels_with_unvisited"] > 0
    assert "two half-pools" in infos[0] and "one stream" in infos[2], infos
    assert out[0] == out[1]
    assert out[0] == out[2]


# ---- (e) beside forced playouts, and beside the Gumbel root search -------------------------------------------------------------
@pytest.mark.parametrize("kind", ("uniform", "hash"))
def test_forced_playouts_override_an_argmax_computed_with_fpu(kind):
    import forced_playouts_reference as fp
    import test_gpu_forced_playouts as tgf
    from azalea_amd import engine as eng
    prefixes = fp.prefixes(kind)[:16]
    mode = ref.MODES[3]
    refs = [ref.Search(p, kind, mode, forced_k=fp.K_FORCED) for p in prefixes]
    plain = [fp.Search(p, kind, fp.K_FORCED) for p in prefixes]
    assert any(not np.array_equal(a.n, b.n) for a, b in zip(refs, plain))      # FPU changes what is forced
    E = tgf.make(eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH, len(prefixes))
    if kind == "hash":
        E.set_prior_table(fp.TABLE)
    E.set_train_targets("visits")
    E.set_forced_playouts(fp.K_FORCED, False)
    E.set_fpu(*mode)
    got, stats = tgf.first_rows(E, prefixes)
    fpu_stats = E.fpu_stats()
    E.close()
    for (row, m), r in zip(got, refs):
        k, S = len(r.n), tgf.raw_sum(m)
        assert S == int(r.n.sum()), (r.forced_at, S)
        assert np.array_equal(np.rint(row[:k].astype(np.float64) * S), r.n), (row[:k] * S, r.n)
    assert stats["forced_selects"] == sum(r.forced for r in refs)
    assert fpu_stats["selects"] >= sum(r.stats()["selects"] for r in refs)      # (the games were played on to their ends)


def test_below_a_gumbel_root_fpu_acts_and_the_root_keeps_its_survivors():
    import gumbel_reference as gr
    import test_gpu_gumbel as tgg
    from azalea_amd import engine as eng
    setup = gr.SETUP["m8_200"]
    prefixes = gr.prefixes_of(setup, "hash")[:16]
    G = len(prefixes)
    mode = ref.MODES[2]
    refs = [ref.GumbelSearch(p, "hash", mode, m=setup.m, seed=gr.SEED, uid=G + g, cfg=setup.cfg)
            for g, p in enumerate(prefixes)]
    plain = [gr.Search(p, "hash", setup.m, seed=gr.SEED, uid=G + g, cfg=setup.cfg) for g, p in enumerate(prefixes)]
    assert any(not np.array_equal(a.n, b.n) for a, b in zip(refs, plain))      # FPU acts below the root
    E = tgg.make(eng.EVAL_UNIFORM_HASH, G, setup.cfg)
    E.set_prior_table(setup.cfg.table)
    E.set_train_targets("visits")
    E.set_gumbel(setup.m, setup.c_visit, setup.c_scale, improved_rows=False)
    E.set_fpu(*mode)
    got, state, stats = tgg.first_rows(E, prefixes, setup.cfg)
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


# ---- (f) a Match and a three-engine Tournament -----------------------------------------------------------------------------------
def match_engines(w, fpu_on, G=32):
    """Three engines with the same weights and seeds that differ from run to run in nothing; engine 0 has FPU on."""
    engines = [net_engine(G, w, seed=(7 + a) << 32, sims=24, bs=6) for a in range(3)]
    if fpu_on:
        engines[0].set_fpu(*REDUCTION)
    return engines


def stones(board):
    return (np.asarray(board).reshape(len(board), -1) != 0).sum(1)


def rows_by_game(rows):
    """{game uid: {ply: (moves_prob bytes, reward, nlegal)}}"""
    out = {}
    for r, (u, p) in enumerate(zip(rows["game_uid"], stones(rows["board"]))):
        out.setdefault(int(u), {})[int(p)] = (rows["moves_prob"][r].tobytes(), float(rows["reward"][r]), int(rows["nlegal"][r]),
                                              rows["board"][r].tobytes())
    return out


def check_off_rows(mixed, off, games, on_agent):
    """`games`: (uid, moves of the mixed run, moves of the all-off run, agent index -- 0 or 1 of its pair -- with the
    option on, or None).  Before the first differing move the games coincide, so the rows of the option-off engine
    there are the all-off run's; where the whole game coincides, every row that both runs recorded is."""
    mixed, off = rows_by_game(mixed), rows_by_game(off)
    compared = differing = 0
    for uid, mv_a, mv_b, on in games:
        diff = np.flatnonzero(mv_a != mv_b)
        d = int(diff[0]) if len(diff) else len(mv_a)
        differing += int(len(diff) > 0)
        for p in range(d):
            mover = (uid + p) & 1                               # agent u & 1 moves first in game u
            if on is not None and mover == on:
                continue
            if p in mixed.get(uid, {}) and p in off.get(uid, {}):
                a, b = mixed[uid][p], off[uid][p]
                assert a[0] == b[0] and a[2:] == b[2:], (uid, p)                # the row, its width, its board
                compared += 1
    return compared, differing


def test_a_match_takes_an_engine_with_fpu_beside_one_without():
    from azalea_amd import engine as eng
    w = small_net_weights()
    runs = {}
    for name, fpu_on in (("mixed", True), ("again", True), ("off", False)):
        a, b, spare = match_engines(w, fpu_on)
        spare.close()
        m = eng.Match(a, b)
        res = m.play(32, moves=True, collect=True)
        runs[name] = (res, a.fpu_stats(), b.fpu_stats())
        m.close()
        a.close()
        b.close()
    res, sa, sb = runs["mixed"]
    assert res["stats"]["games"] == 32 and res["stats"]["voided"] == 0
    assert sa["selects"] > 0 and sa["levels_with_unvisited"] > 0 and sb == ZERO_STATS
    assert runs["off"][1] == ZERO_STATS and runs["off"][2] == ZERO_STATS
    for k in ("outcome", "length", "moves"):
        assert np.array_equal(res[k], runs["again"][0][k]), k
    assert sorted_rows(res["rows"], res["row_metrics"]) == sorted_rows(runs["again"][0]["rows"], runs["again"][0]["row_metrics"])
    assert sa == runs["again"][1]
    off = runs["off"][0]
    games = [(u, res["moves"][u], off["moves"][u], 0) for u in range(32)]
    compared, differing = check_off_rows(res["rows"], off["rows"], games, 0)
    print("match: rows of the option-off engine compared", compared, "games that differ", differing, "of 32")
    assert compared > 0 and differing > 0


def test_a_tournament_takes_one_engine_with_fpu_among_three():
    from azalea_amd import engine as eng
    w = small_net_weights()
    pairs, rounds = [(0, 1), (0, 2), (1, 2)], 12
    runs = {}
    for name, fpu_on in (("mixed", True), ("again", True), ("off", False)):
        engines = match_engines(w, fpu_on)
        t = eng.Tournament(engines)
        res = t.play(pairs, rounds, moves=True, collect=True, sink=1)
        runs[name] = (res, [e.fpu_stats() for e in engines])
        t.close()
        for e in engines:
            e.close()
    res, stats = runs["mixed"]
    assert stats[0]["selects"] > 0 and stats[1] == ZERO_STATS and stats[2] == ZERO_STATS
    assert runs["off"][1] == [ZERO_STATS] * 3 and stats == runs["again"][1]
    for pair in pairs:
        assert res[pair]["stats"]["games"] == rounds and res[pair]["stats"]["voided"] == 0
        for k in ("outcome", "length", "moves"):
            assert np.array_equal(res[pair][k], runs["again"][0][pair][k]), (pair, k)
    assert sorted_rows(res["rows"], res["row_metrics"]) == sorted_rows(runs["again"][0]["rows"], runs["again"][0]["row_metrics"])
    off = runs["off"][0]
    games = []
    for s, pair in enumerate(pairs):
        on = 0 if pair[0] == 0 else None                        # engine 0 is agent 0 of its pairs
        games += [(s * rounds + r, res[pair]["moves"][r], off[pair]["moves"][r], on) for r in range(rounds)]
    # the pair of two option-off engines plays the all-off tournament's games
    for k in ("outcome", "length", "moves"):
        assert np.array_equal(res[(1, 2)][k], off[(1, 2)][k]), k
    compared, differing = check_off_rows(res["rows"], off["rows"], games, 0)
    print("tournament: rows of option-off engines compared", compared, "games that differ", differing, "of", 3 * rounds)
    assert compared > 0 and differing > 0


# ---- (g) errors ------------------------------------------------------------------------------------------------------------
def test_set_during_a_phase_api_search_is_estate_and_bad_values_are_einval():
    from azalea_amd import engine as eng
    from azalea_amd._lib import AzxError
    cfg = cfg_of(5, 10)
    E = tree_engine("skew", cfg, 1)
    L = E.L
    E.set_fpu("absolute", 0.25)
    kept = E.fpu()
    for bad in ((3, 0.0, 0.0, 0.0), (-1, 0.0, 0.0, 0.0), (1, 1.5, 0.0, 0.0), (1, -1.5, 0.0, 0.0), (1, float("nan"), 0.0, 0.0),
                (2, 0.0, -0.1, 0.0), (2, 0.0, 0.25, -1.0), (2, 0.0, float("nan"), 0.0), (2, 0.0, 0.25, float("nan")),
                (2, 0.0, float("inf"), 0.0)):
        assert L.azx_set_fpu(E.h, *bad) == -1 and b"fpu" in L.azx_last_error(), bad
        assert E.fpu() == kept
    assert L.azx_set_fpu(None, 2, 0.0, 0.25, 0.0) == -1 and L.azx_fpu_stats(E.h, None) == -1
    E.reset(moves=[[]])
    evaluate = ref.skew_host_evaluator()
    n = E.search_begin()
    with pytest.raises(AzxError, match=r"azx error -4.*phase-API search"):
        E.set_fpu(*REDUCTION)
    with pytest.raises(AzxError, match=r"azx error -4"):
        E.clear_fpu()
    assert E.fpu() == kept
    while True:                                                 # the search goes on, under the setting it began with
        if n:
            b, lm, slot, k = E.get_leaves()
            E.put_evals(*evaluate(b, lm, slot, k))
        n, done = E.search_step()
        if done:
            break
    same_dump(E.tree_dump(0), ref.tree_case(5, 10, cfg.sims, "skew", ("absolute", 0.25, 0.0, 0.0), ())[0], "after the refusals")
    E.set_fpu(*REDUCTION)                                       # between searches it is accepted again
    assert E.fpu()["mode"] == "reduction" and E.fpu_stats() == ZERO_STATS
    E.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        child(sys.argv[2])
