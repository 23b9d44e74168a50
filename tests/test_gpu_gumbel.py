"""Gumbel root search with sequential halving (azx_set_gumbel; NOT the reference's behaviour, off by default) on the
device.  The rule's reference is tests/gumbel_reference.py: the numpy float32 restatement of the oracle's search with the
rule as a parameter (noise from the host function engine.gumbel_variate, keys and softmax in float64), pinned to the
unmodified oracle with the rule off (tests/test_gumbel_api.py).  One slot per reference position: after one reset slot g
plays prefix g as game uid G + g of an engine with seed gumbel_reference.SEED.  A position with a decision inside the
safe margin is left out of the exact comparisons (at most 10 % of a case, a condition the CPU test holds)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gumbel_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
EINVAL = -1
ROW_KEYS = ("board", "color", "nlegal", "moves_prob", "reward", "game_uid")
CTR_SELECTS, CTR_PLIES, CTR_CAP_FULL, CTR_CAP_FAST = 0, 8, 13, 14
STAT_KEYS = ("plies", "halvings", "root_selects", "improved_rows")
ZERO_STATS = dict.fromkeys(STAT_KEYS, 0)
PATHS = ["persistent", "no_persistent", "generic"]
N5, CELLS5 = ref.DEFAULT.n, ref.DEFAULT.cells


def make(evaluator, G, cfg=ref.DEFAULT, seed=ref.SEED, **kw):
    from azalea_amd import engine as eng
    conf = dict(board_size=cfg.n, n_games=G, simulations=cfg.sims, search_batch_size=cfg.bs,
                exploration_coef=cfg.c_puct, exploration_depth=cfg.cells, noise_alpha=0.3, noise_scale=0.0,
                temperature=1.0, seed=seed)
    conf.update(kw)
    return eng.Engine(evaluator=evaluator, **conf)


def stones(board):
    return (np.asarray(board).reshape(len(board), -1) != 0).sum(1)


def engine_on_path(kind, path, monkeypatch, G, cfg, **kw):
    """An engine of `kind` ("uniform": the inline evaluator's three paths; "hash": values leave the wave, so the tree
    kernel is the generic one whatever the switch) created under the diagnostic switch of `path`."""
    from azalea_amd import engine as eng
    if path == "no_persistent":
        monkeypatch.setenv("AZX_NO_PERSISTENT", "1")          # (read by azx_create)
    elif path == "generic":
        monkeypatch.setenv("AZX_MCTS_GENERIC", "1")
    E = make(eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH, G, cfg, **kw)
    if kind == "hash":
        E.set_prior_table(cfg.table)
    else:
        info = E.kernel_info()
        S = 3 if cfg.cells > 128 else 2                       # the instantiation: register slots of 64 children
        assert ("k_play<%d> (persistent)" % S in info) == (path == "persistent"), info
        assert ("k_mcts<%d,FAST" % S in info) == (path != "generic") and ("k_mcts<%d,generic>" % S in info) == (path == "generic"), info
    return E


def first_rows(E, prefixes, cfg):
    """Reset the slots to the prefixes and play: one ply (the option's state and statistics are read there), then every
    slot's game to its end, so that the harvest hands over the row the first ply recorded.  Returns (per slot: that
    row's moves_prob, its metrics and the cell index of the move the game's next row shows, or None where the game ended
    with that ply), gumbel_state and gumbel_stats after the one ply."""
    G = len(prefixes)
    E.reset(moves=[list(p) for p in prefixes])
    never = 4 * G * cfg.cells                                   # more rows than these plies can record: max_plies ends the calls
    parts = []
    rows, _ = E.play(never, max_plies=1)
    parts.append((rows, E.play_row_metrics()))
    state, stats = E.gumbel_state(), E.gumbel_stats()
    rows, _ = E.play(never, max_plies=cfg.cells)
    parts.append((rows, E.play_row_metrics()))
    rows = {k: np.concatenate([p[0][k] for p in parts]) for k in ROW_KEYS}
    m = np.concatenate([p[1] for p in parts])
    assert len(m) == len(rows["reward"])
    out = []
    for g, prefix in enumerate(prefixes):
        mine = np.flatnonzero(rows["game_uid"] == G + g)        # the prefix's game: the slot's second generation
        assert len(mine), (g, prefix)
        order = mine[np.argsort(stones(rows["board"][mine]))]
        r = order[0]
        assert np.array_equal(rows["board"][r], ref.game_at(prefix, cfg).board), (g, prefix)
        assert rows["nlegal"][r] == cfg.cells - len(prefix)
        cell = None
        if len(order) > 1:
            new = np.flatnonzero((rows["board"][order[1]] != rows["board"][r]).ravel())
            assert len(new) == 1
            cell = int(new[0])
        out.append((rows["moves_prob"][r], m[r], cell))
    return out, state, stats


def raw_sum(metrics):
    """The raw visit sum of a row: metric 4 (mean root-child visits) times metric 6 (root children)."""
    return int(np.rint(float(metrics[4]) * float(metrics[6])))


def engine_for(setup, kind, path, monkeypatch, G):
    return engine_on_path(kind, path, monkeypatch, G, setup.cfg,
                          exploration_depth=0 if setup.greedy else setup.cfg.cells)


def check_state_and_stats(refs, state, stats, improved):
    cand, surv = state
    safe = 0
    for g, r in enumerate(refs):
        if not r["safe"]:
            continue
        safe += 1
        assert np.array_equal(cand[g], ref.mask_words(r["candidates"])), (r["prefix"], cand[g], r["candidates"])
        assert np.array_equal(surv[g], ref.mask_words(r["survivors"])), (r["prefix"], surv[g], r["survivors"])
    assert safe >= (1.0 - ref.MAX_UNSAFE_SHARE) * len(refs)
    # plies, halvings and selects depend on no key comparison: over ALL positions
    assert stats == dict(plies=len(refs), halvings=sum(r["halvings"] for r in refs),
                         root_selects=sum(r["root_selects"] for r in refs), improved_rows=len(refs) if improved else 0)


def legal_cells(prefix, cfg):
    return np.asarray(ref.game_at(prefix, cfg).legal_moves()) - 1


# ---- 1. the variates ---------------------------------------------------------------------------------------------------
def test_device_variates_are_the_host_functions():
    """azx_selftest_gumbel against engine.gumbel_variate on 2^16 words: the words of 2^16 - 512 (uid, ply, child)
    triples (tests/gumbel_reference.py restates Philox), where the host function is called itself, and the 256 smallest
    and the 256 largest 24-bit values, where its formula is evaluated in float64.  Within 2e-5 absolute: float32 spacing
    at |g| <= 17.4 is 1.9e-6; two chained logarithms at about 1 ulp each plus the rounding of g stay under ten
    spacings."""
    from azalea_amd import engine as eng
    n = (1 << 16) - 512
    rng = np.random.RandomState(7)
    uid, ply, child = rng.randint(0, 1 << 20, n), rng.randint(0, 169, n), rng.randint(0, 169, n)
    words = np.concatenate([ref.philox_words(ref.SEED, u, p, [c])
                            for u, p, c in zip(uid[:64], ply[:64], child[:64])])       # one by one ...
    per_uid = {}
    for i in range(64, n):
        per_uid.setdefault((int(uid[i]), int(ply[i])), []).append(int(child[i]))
    rest, host = [], [eng.gumbel_variate(ref.SEED, int(u), int(p), int(c)) for u, p, c in zip(uid[:64], ply[:64], child[:64])]
    for (u, p), cs in per_uid.items():                                                  # ... and by arrays
        rest.append(ref.philox_words(ref.SEED, u, p, cs))
        host += [eng.gumbel_variate(ref.SEED, u, p, c) for c in cs]
    lo = (np.arange(256, dtype=np.uint32) << 8) | 0x5A
    hi = ((np.uint32(0xFFFFFF) - np.arange(256, dtype=np.uint32)) << 8) | 0xA5
    words = np.concatenate([words] + rest + [lo, hi]).astype(np.uint32)
    want = np.concatenate([np.array(host), ref.gumbel_of_words(lo), ref.gumbel_of_words(hi)])
    assert len(words) == 1 << 16 == len(want)
    assert np.abs(want[:n] - ref.gumbel_of_words(words[:n])).max() <= 1e-12             # the host function IS the formula
    got = eng.selftest_gumbel(words)
    err = np.abs(got.astype(np.float64) - want)
    print("device g against the host's: max |error| %.3g (at g = %.4f), range of g [%.4f, %.4f]"
          % (err.max(), want[err.argmax()], want.min(), want.max()))
    assert np.isfinite(got).all() and err.max() <= 2e-5


# ---- 2. one ply of every reference position ----------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,kind", ref.CASES)
def test_one_ply_of_every_position_follows_the_restatement(name, kind, path, monkeypatch):
    setup, refs = ref.SETUP[name], ref.positions(name, kind)
    E = engine_for(setup, kind, path, monkeypatch, len(refs))
    assert "gumbel=off" in E.kernel_info()
    E.set_train_targets("visits")
    E.set_gumbel(setup.m, setup.c_visit, setup.c_scale, improved_rows=False)
    assert "gumbel=%d/50/1/norows" % setup.m in E.kernel_info() and E.gumbel() == (setup.m, 50.0, 1.0, False)
    got, state, stats = first_rows(E, [r["prefix"] for r in refs], setup.cfg)
    E.close()
    worst = 0.0
    for (row, m, cell), r in zip(got, refs):
        if not r["safe"]:
            continue
        k, S = r["k"], raw_sum(m)
        assert S == int(r["n"].sum()), (r["prefix"], S)
        assert np.array_equal(np.rint(row[:k].astype(np.float64) * S), r["n"]), (r["prefix"], row[:k] * S, r["n"])
        assert (row[k:] == 0).all()
        if cell is not None:
            assert cell == legal_cells(r["prefix"], setup.cfg)[r["move"]], (r["prefix"], cell, r["move"])
        worst = max(worst, abs(float(m[2]) - float(np.log(r["pi"][r["move"]]))))
    if setup.family in ("9", "13"):                             # more than one live register slot at the root
        assert all(r["k"] > 64 for r in refs) if setup.family == "9" else any(r["k"] > 128 for r in refs)
    print(name, kind, path, "positions", len(refs), "left out", sum(not r["safe"] for r in refs),
          "max |metric 2 - ln pi_chosen| %.3g" % worst)
    assert worst <= 1e-3
    check_state_and_stats(refs, state, stats, improved=False)


# ---- 3. improved rows --------------------------------------------------------------------------------------------------
def pow2_evaluator(n):
    """gumbel_reference's "pow2" stub on the device: value 0, prior w / sum(w), w = 2^-(1 + (i - j) mod 4) of the legal
    cell (i, j); one float64 division, rounded to float32 once."""
    def evaluate(board, legal):
        t = legal.to(torch.int64) - 1
        e = 1 + torch.remainder(torch.div(t, n, rounding_mode="floor") - torch.remainder(t, n), 4)
        one = torch.ones((), dtype=torch.float64, device=DEV)
        w = torch.where(legal != 0, torch.ldexp(one, -e), torch.zeros((), dtype=torch.float64, device=DEV))
        return torch.zeros(len(board), dtype=torch.float32, device=DEV), (w / w.sum(1, keepdim=True)).to(torch.float32)
    return evaluate


def test_improved_rows_under_non_uniform_priors_keep_the_ln_p_term():
    """Both stub evaluators give every child one prior, so ln P cancels in their improved rows.  Here a registered
    external evaluator hands out four different priors: the row, metric 2, the masks and the move against the
    restatement with the same priors, within the same bounds."""
    from azalea_amd import engine as eng
    setup, refs = ref.POW2, ref.positions(ref.POW2.name, "pow2")
    assert all(len(set(r["p"].tolist())) > 1 for r in refs)
    E = make(eng.EVAL_EXTERNAL, len(refs), setup.cfg)
    E.set_external_evaluator(pow2_evaluator(setup.cfg.n))
    E.set_gumbel(setup.m, setup.c_visit, setup.c_scale, improved_rows=True)
    got, state, stats = first_rows(E, [r["prefix"] for r in refs], setup.cfg)
    E.close()
    worst_row = worst_lp = 0.0
    uniform_gap = 0.0
    for (row, m, cell), r in zip(got, refs):
        if not r["safe"]:
            continue
        k = r["k"]
        worst_row = max(worst_row, float(np.abs(row[:k].astype(np.float64) - r["pi"]).max()))
        worst_lp = max(worst_lp, abs(float(m[2]) - float(np.log(r["pi"][r["move"]]))))
        assert abs(float(row[:k].astype(np.float64).sum()) - 1.0) <= 1e-5 and (row[k:] == 0).all()
        assert raw_sum(m) == int(r["n"].sum())
        if cell is not None:
            assert cell == legal_cells(r["prefix"], setup.cfg)[r["move"]]
        x = ref.sigma_of(r["n"], r["w"], r["p"], setup.c_visit, setup.c_scale)          # the row WITHOUT ln P
        e = np.exp(x - x.max())
        uniform_gap = max(uniform_gap, float(np.abs(e / e.sum() - r["pi"]).max()))
    print("pow2 priors: max |row - pi| %.3g, max |metric 2 - ln pi_chosen| %.3g; a row without ln P would be off by %.3g"
          % (worst_row, worst_lp, uniform_gap))
    assert worst_row <= 5e-4 and worst_lp <= 1e-3 and uniform_gap > 1e-2
    check_state_and_stats(refs, state, stats, improved=True)


@pytest.mark.parametrize("setup", ref.POW2Z, ids=[s.name for s in ref.POW2Z])
def test_exact_zeros_among_the_priors(setup):
    """ln P = -inf for a child of prior 0, in the candidates' keys, the halvings and the improved row.  With m = 8 no such
    child may become a candidate; with m = 16 on positions with fewer children of nonzero prior than candidates some
    must, are visited, and are halved away.  One run records the visit shares (the root picks, select by select, decide
    the counts), one the improved rows; both against the restatement: candidates, survivors, counts, the move, the row
    within the bounds of the tests above -- and the row finite, exactly 0 where P = 0, its sum within 1e-5 of 1."""
    from azalea_amd import engine as eng
    refs = ref.positions(setup.name, "pow2z")
    assert all(r["safe"] for r in refs)
    zero = [r["p"] == 0 for r in refs]
    assert all(z.any() and not z.all() for z in zero)
    if setup.family == "few":
        assert all(ref.nonzero_pow2z(r["prefix"]) < r["m0"] for r in refs)
        assert all(z[r["candidates"]].any() and (r["n"][z] > 0).any() and not z[r["survivors"]].any()
                   for r, z in zip(refs, zero))
    else:
        assert not any(z[r["candidates"]].any() for r, z in zip(refs, zero))
    for improved in (False, True):
        E = make(eng.EVAL_EXTERNAL, len(refs), setup.cfg)
        E.set_external_evaluator(ref.pow2z_device_evaluator(setup.cfg.n, DEV))
        if not improved:
            E.set_train_targets("visits")
        E.set_gumbel(setup.m, setup.c_visit, setup.c_scale, improved_rows=improved)
        got, state, stats = first_rows(E, [r["prefix"] for r in refs], setup.cfg)
        E.close()
        worst_row = worst_lp = 0.0
        for (row, m, cell), r, z in zip(got, refs, zero):
            k, S = r["k"], raw_sum(m)
            assert S == int(r["n"].sum()), (r["prefix"], S)
            assert np.isfinite(row).all() and (row >= 0).all() and (row[k:] == 0).all()
            if improved:
                assert (row[:k][z] == 0).all() and (row[:k][~z] > 0).all(), (r["prefix"], row[:k])
                assert abs(float(row[:k].astype(np.float64).sum()) - 1.0) <= 1e-5
                worst_row = max(worst_row, float(np.abs(row[:k].astype(np.float64) - r["pi"]).max()))
            else:
                assert np.array_equal(np.rint(row[:k].astype(np.float64) * S), r["n"]), (r["prefix"], row[:k] * S, r["n"])
            assert np.isfinite(m).all()
            worst_lp = max(worst_lp, abs(float(m[2]) - float(np.log(r["pi"][r["move"]]))))
            if cell is not None:
                assert cell == legal_cells(r["prefix"], setup.cfg)[r["move"]], (r["prefix"], cell, r["move"])
        print(setup.name, "improved rows" if improved else "visit shares", "positions", len(refs),
              "max |row - pi| %.3g, max |metric 2 - ln pi_chosen| %.3g" % (worst_row, worst_lp))
        assert worst_row <= 5e-4 and worst_lp <= 1e-3
        check_state_and_stats(refs, state, stats, improved=improved)


@pytest.mark.parametrize("name,kind", ref.CASES)
def test_improved_rows_are_the_restatements_softmax(name, kind, monkeypatch):
    """The row against the restatement's float64 pi within 5e-4 absolute (an argument error delta of about 1e-4 gives a
    relative error of at most e^(2 delta) - 1), its sum within 1e-5 of 1, zero beyond k; metric 2 within 1e-3."""
    setup, refs = ref.SETUP[name], ref.positions(name, kind)
    E = engine_for(setup, kind, "persistent", monkeypatch, len(refs))
    E.set_gumbel(setup.m, setup.c_visit, setup.c_scale, improved_rows=True)
    assert "gumbel=%d/50/1/rows" % setup.m in E.kernel_info() and E.gumbel() == (setup.m, 50.0, 1.0, True)
    got, state, stats = first_rows(E, [r["prefix"] for r in refs], setup.cfg)
    E.close()
    worst_row = worst_sum = worst_lp = 0.0
    for (row, m, cell), r in zip(got, refs):
        if not r["safe"]:
            continue
        k = r["k"]
        worst_row = max(worst_row, float(np.abs(row[:k].astype(np.float64) - r["pi"]).max()))
        worst_sum = max(worst_sum, abs(float(row[:k].astype(np.float64).sum()) - 1.0))
        worst_lp = max(worst_lp, abs(float(m[2]) - float(np.log(r["pi"][r["move"]]))))
        assert (row[k:] == 0).all() and (row >= 0).all()
        assert raw_sum(m) == int(r["n"].sum()) and m[1] == (r["n"] > 0).sum()      # the other metrics stay on the counts
        if cell is not None:
            assert cell == legal_cells(r["prefix"], setup.cfg)[r["move"]]
    print(name, kind, "max |row - pi| %.3g, max |sum - 1| %.3g, max |metric 2 - ln pi_chosen| %.3g"
          % (worst_row, worst_sum, worst_lp))
    assert worst_row <= 5e-4 and worst_sum <= 1e-5 and worst_lp <= 1e-3
    check_state_and_stats(refs, state, stats, improved=True)


# ---- 4. non-uniform priors ---------------------------------------------------------------------------------------------
def small_net_weights():
    from azalea_amd.network import HexNetwork
    torch.manual_seed(3)
    net = HexNetwork(board_size=N5, num_blocks=1, base_chans=64).eval()
    return {k: v.detach().numpy() for k, v in net.state_dict().items()}


def net_engine(G, w, **kw):
    from azalea_amd import engine as eng
    E = make(eng.EVAL_RESNET, G, ref.SETUP["m16_20"].cfg, num_blocks=1, base_chans=64, **kw)
    E.set_weights(w)
    return E


def test_candidates_under_a_networks_priors_are_the_top_of_g_plus_ln_p():
    from azalea_amd import engine as eng
    import forced_playouts_reference as fp
    prefixes = [list(p) for p in fp.prefixes("hash")][:48]
    G, m = len(prefixes), 8
    E = net_engine(G, small_net_weights())
    E.reset(moves=prefixes)
    E.search()                                                 # (azx_search reads "off": PUCT, and the root's stored priors)
    root = E.get_root()
    E.set_gumbel(m, improved_rows=True)
    E.reset(moves=prefixes)                                    # the second reset: slot g plays uid 2 G + g
    E.play(4 * G * CELLS5, max_plies=1)
    cand, surv = E.gumbel_state()
    E.close()
    compared = 0
    for g, prefix in enumerate(prefixes):
        k = int(root["k"][g])
        P = root["child_prior"][g, :k]
        assert k == CELLS5 - len(prefix) and len(set(P.tolist())) > 1                  # non-uniform
        gv = np.array([eng.gumbel_variate(ref.SEED, 2 * G + g, len(prefix), j) for j in range(k)])
        a = gv + np.log(P.astype(np.float64))
        kept, dropped = ref.top(a, np.arange(k), min(m, k))
        if not ref.safe_cut(a, kept, dropped, [(x,) for x in range(k)]):
            continue
        compared += 1
        assert np.array_equal(cand[g], ref.mask_words(kept)), (prefix, cand[g], kept)
        words = surv[g]
        assert all((int(words[c >> 6]) >> (c & 63)) & 1 == 0 for c in dropped) and int(words.sum()) != 0
    assert compared >= 0.9 * G


def test_no_dirichlet_noise_reaches_the_selects():
    w = small_net_weights()
    out = []
    for scale in (0.0, 0.25):
        E = net_engine(256, w, noise_scale=scale, seed=77)
        E.set_gumbel(16)
        rows, st = E.play(600)
        out.append(sorted_rows(rows, E.play_row_metrics()))
        assert st["games"] > 0
        E.close()
    assert out[0] == out[1]


# ---- 5. whole games ----------------------------------------------------------------------------------------------------
def sorted_rows(rows, m):
    i = np.argsort(rows["game_uid"], kind="stable")       # finished games enter the queue in the order the GPU finished them
    return {k: rows[k][i].tobytes() for k in ROW_KEYS}, m[i].tobytes()


def games_by_uid(rows, m):
    out = {}
    uid = rows["game_uid"]
    for u in np.unique(uid):
        i = np.flatnonzero(uid == u)
        out[int(u)] = tuple(rows[k][i].tobytes() for k in ROW_KEYS) + (m[i].tobytes(),)
    return out


def check_games(rows, cfg=ref.DEFAULT, contiguous=True):
    """Every game's rows replay as a legal, decided game under the oracle's rules: each row's board is the position, its
    row a distribution (non-negative, zero beyond k, sum 1 within 1e-5), the next row's board one legal stone further;
    the last mover's colour gets +1, the other -1.  Returns the number of games."""
    uid, ply = rows["game_uid"], stones(rows["board"])
    starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
    for s, e in zip(starts, np.r_[starts[1:], len(uid)]):
        if contiguous:
            assert np.array_equal(ply[s:e], np.arange(e - s))
        h = ref.game_at([], cfg)
        for r in range(s, e):
            k = int(rows["nlegal"][r])
            p = rows["moves_prob"][r]
            assert (p >= 0).all() and (p[k:] == 0).all() and abs(float(p[:k].astype(np.float64).sum()) - 1.0) <= 1e-5, (r, p)
            if contiguous:
                assert h.result == 0 and np.array_equal(h.board, rows["board"][r])
                assert len(h.legal_moves()) == k and rows["color"][r] == ply[r] % 2
                if r + 1 < e:
                    new = np.flatnonzero((rows["board"][r + 1] != rows["board"][r]).ravel())
                    assert len(new) == 1
                    h.step(int(new[0]) + 1)
        want = np.where(rows["color"][s:e] == rows["color"][e - 1], 1.0, -1.0).astype(np.float32)
        if contiguous:
            assert np.array_equal(rows["reward"][s:e], want)
        else:
            assert (np.abs(rows["reward"][s:e]) == 1).all()
    return len(starts)


def hash_engine(G, sims=40, **kw):
    from azalea_amd import engine as eng
    cfg = ref.Settings(n=5, sims=sims, bs=10, c_puct=0.5)
    E = make(eng.EVAL_UNIFORM_HASH, G, cfg, exploration_depth=4, **kw)
    E.set_prior_table(cfg.table)
    return E


def test_the_pool_size_does_not_change_a_game():
    got = []
    for G in (64, 256):
        E = hash_engine(G, seed=5)
        E.set_gumbel(16)
        rows, st = E.play(1500)
        got.append(games_by_uid(rows, E.play_row_metrics()))
        assert check_games(rows) == st["games"] > 64 and E.gumbel_stats()["improved_rows"] >= len(rows["reward"])
        E.close()
    both = sorted(set(got[0]) & set(got[1]))
    assert len(both) >= 32
    assert all(got[0][u] == got[1][u] for u in both)


def test_the_three_inline_paths_record_the_same_rows(monkeypatch):
    from azalea_amd import engine as eng
    out = []
    for path in PATHS:
        with monkeypatch.context() as mp:
            E = engine_on_path("uniform", path, mp, 64, ref.Settings(n=5, sims=40, bs=10, c_puct=0.5), seed=9,
                               exploration_depth=4)
            E.set_gumbel(16)
            rows, st = E.play(400)
            out.append(games_by_uid(rows, E.play_row_metrics()))      # (the paths differ in how far beyond 400 rows they play)
            assert E.gumbel_stats()["halvings"] > 0 and st["games"] > 0
            E.close()
    both = sorted(set(out[0]) & set(out[1]) & set(out[2]))
    assert len(both) >= 16 and all(out[0][u] == out[1][u] == out[2][u] for u in both)


def test_the_two_half_pools_of_a_network_against_one_stream(monkeypatch):
    w = small_net_weights()
    out = []
    for pipeline in (True, False):
        with monkeypatch.context() as mp:
            if not pipeline:
                mp.setenv("AZX_PIPELINE", "0")
            E = net_engine(1024, w, seed=2024, exploration_depth=4)
            assert ("two half-pools" in E.kernel_info()) == pipeline, E.kernel_info()
            E.set_gumbel(8)
            rows, st = E.play(2000)
            out.append((games_by_uid(rows, E.play_row_metrics())))
            assert check_games(rows) == st["games"] > 0
            E.close()
    both = sorted(set(out[0]) & set(out[1]))
    assert len(both) >= 32 and all(out[0][u] == out[1][u] for u in both)


def test_a_registered_external_evaluator_computing_the_stub_equals_the_inline_stub():
    from azalea_amd import engine as eng
    cfg = ref.Settings(n=5, sims=40, bs=10, c_puct=0.5)
    inv = torch.tensor(cfg.table, device=DEV)

    def evaluate(board, legal):                                   # the "uniform" stub: value 0, prior 1/k
        k = (legal != 0).sum(1)
        prior = torch.where(legal != 0, inv[k][:, None], torch.zeros((), device=DEV))
        return torch.zeros(len(board), dtype=torch.float32, device=DEV), prior

    out = []
    for external in (False, True):
        E = make(eng.EVAL_EXTERNAL if external else eng.EVAL_UNIFORM, 64, cfg, seed=99, exploration_depth=4)
        if external:
            E.set_external_evaluator(evaluate)
        E.set_gumbel(16)
        rows, st = E.play(600)
        out.append(games_by_uid(rows, E.play_row_metrics()))
        assert check_games(rows) == st["games"] > 0
        E.close()
    both = sorted(set(out[0]) & set(out[1]))
    assert len(both) >= 16 and all(out[0][u] == out[1][u] for u in both)


def test_beside_a_playout_cap_fast_plies_search_under_the_option_and_record_nothing():
    from azalea_amd import engine as eng
    G, steps, p, sims, fast, bs = 64, 8, 0.5, 100, 40, 10
    E = hash_engine(G, sims=sims)
    E.set_playout_cap(p, fast)
    E.set_gumbel(16)
    st = E.play_steps(steps)
    raw = E.debug_counters_raw().astype(np.int64)
    stats = E.gumbel_stats()
    E.close()
    full = np.array([[eng.playout_cap_is_full(ref.SEED, g, q, p) for q in range(steps)] for g in range(G)], bool)
    assert st["games"] == 0 and np.array_equal(raw[:, CTR_CAP_FULL], full.sum(1))
    n_full, n_fast = int(full.sum()), int((~full).sum())
    assert stats["plies"] == G * steps and stats["improved_rows"] == n_full      # fast plies record nothing
    # selects per ply are exactly bs * (p_obs * NB_full + (1 - p_obs) * NB_fast)
    assert stats["root_selects"] == bs * (n_full * (sims // bs + 1) + n_fast * (fast // bs + 1))
    assert stats["root_selects"] == raw[:, CTR_SELECTS].sum()


def test_harvested_games_replay_as_legal_decided_games():
    E = hash_engine(128, seed=21)
    E.set_train_targets("visits", 0.0)
    E.set_gumbel(8, improved_rows=False)
    rows, st = E.play(1200)
    assert check_games(rows) == st["games"] >= 64
    E.set_gumbel(8, 30.0, 0.5, improved_rows=True)
    rows, st = E.play(1200)
    m = E.play_row_metrics()
    E.close()
    check_games(rows, contiguous=False)                          # (the first harvest after the switch holds mixed games)
    assert np.isfinite(m[:, 2]).all() and (m[:, 2] <= 1e-6).all()


# ---- 6. off means off --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ref.KINDS)
def test_the_option_never_set_or_cleared_leaves_no_trace(kind):
    from azalea_amd import engine as eng
    evaluator = eng.EVAL_UNIFORM if kind == "uniform" else eng.EVAL_UNIFORM_HASH
    out, infos = [], []
    for cleared in (False, True):
        E = make(evaluator, 64, ref.Settings(n=5, sims=40, bs=4, c_puct=0.5), seed=11, exploration_depth=2,
                 noise_scale=0.25)
        if cleared:
            E.set_gumbel(16)
            assert "gumbel=16/50/1/rows" in E.kernel_info()
            E.clear_gumbel()
        infos.append(E.kernel_info())
        rows, st = E.play(200)
        out.append((sorted_rows(rows, E.play_row_metrics()), {k: v for k, v in st.items() if not k.endswith("seconds")}))
        assert E.gumbel_stats() == ZERO_STATS and E.gumbel() == (0, 0.0, 0.0, False)
        E.close()
    assert out[0][0] == out[1][0]
    assert out[0][1] == out[1][1]
    assert "gumbel=off" in infos[0] and infos[0] == infos[1]


def test_bad_calls_and_the_rules_beside_forced_playouts_and_early_stop():
    import ctypes as C
    from azalea_amd import engine as eng
    E = make(eng.EVAL_UNIFORM, 16, ref.Settings(n=5, sims=40, bs=4, c_puct=0.5))
    L = E.L
    E.set_gumbel(8, 30.0, 2.0, improved_rows=False)
    for bad in ((1, 50.0, 1.0, 1), (65, 50.0, 1.0, 1), (-2, 50.0, 1.0, 1), (8, -1.0, 1.0, 1), (8, 2e4, 1.0, 1),
                (8, float("nan"), 1.0, 1), (8, 50.0, 0.0, 1), (8, 50.0, 101.0, 1), (8, 50.0, float("inf"), 1),
                (8, 50.0, 1.0, 2), (8, 50.0, 1.0, -1)):
        assert L.azx_set_gumbel(E.h, *bad) == EINVAL and b"gumbel" in L.azx_last_error(), bad
        assert "gumbel=8/30/2/norows" in E.kernel_info() and E.gumbel() == (8, 30.0, 2.0, False)
    assert L.azx_set_gumbel(None, 8, 50.0, 1.0, 1) == EINVAL and L.azx_gumbel_stats(E.h, None) == EINVAL
    mm, rr, cv = C.c_int(0), C.c_int(0), C.c_float(0)
    assert L.azx_get_gumbel(E.h, None, C.byref(cv), C.byref(cv), C.byref(rr)) == EINVAL
    assert L.azx_get_gumbel(E.h, C.byref(mm), C.byref(cv), C.byref(cv), None) == EINVAL
    assert L.azx_gumbel_state(E.h, None, None) == EINVAL
    # beside forced playouts and early stop, in both orders: rules about PUCT visit leaders
    assert L.azx_set_forced_playouts(E.h, 2.0, 1) == EINVAL and b"Gumbel" in L.azx_last_error()
    assert L.azx_set_early_stop(E.h, 1) == EINVAL and b"Gumbel" in L.azx_last_error()
    assert L.azx_set_forced_playouts(E.h, 0.0, 0) == 0 and L.azx_set_early_stop(E.h, 0) == 0      # "off" is no conflict
    assert E.gumbel() == (8, 30.0, 2.0, False) and E.forced_playouts() == (0.0, False)
    E.clear_gumbel()
    assert "gumbel=off" in E.kernel_info()
    E.set_forced_playouts(2.0, True)
    assert L.azx_set_gumbel(E.h, 8, 50.0, 1.0, 1) == EINVAL and b"forced playouts" in L.azx_last_error()
    E.clear_forced_playouts()
    E.set_early_stop(True)
    assert L.azx_set_gumbel(E.h, 8, 50.0, 1.0, 1) == EINVAL and b"early stop" in L.azx_last_error()
    assert L.azx_set_gumbel(E.h, 0, 0.0, 0.0, 0) == 0 and E.gumbel() == (0, 0.0, 0.0, False)
    E.set_early_stop(False)
    E.set_gumbel(64, 0.0, 100.0)
    assert "gumbel=64/0/100/rows" in E.kernel_info()
    for bad in ((1,), (65,), (8, -1.0), (8, 50.0, 0.0)):
        with pytest.raises(ValueError, match="gumbel"):
            E.set_gumbel(*bad)
    E.close()


def test_matches_and_tournaments_refuse_the_option_before_touching_any_engine():
    from azalea_amd import engine as eng
    from azalea_amd._lib import AzxError
    cfg = ref.Settings(n=5, sims=16, bs=4, c_puct=0.5)
    a, b = (make(eng.EVAL_UNIFORM_HASH, 64, cfg, seed=s, exploration_depth=4, noise_scale=0.25) for s in (6, 7))
    for e in (a, b):
        e.play(40)                                            # rows in both harvest queues, games under way in the slots
    m, t = eng.Match(a, b), eng.Tournament([a, b])

    def state():
        out = []
        for e in (a, b):
            g = e.get_games()
            out.append((g["board"].tobytes(), g["ply"].tobytes(), e.get_root()["root_visits"].tobytes(),
                        {k: v.tobytes() for k, v in e.rows_read(0, e._last_rows).items()}))
        return out
    before = state()
    for on, name, idx in ((b, "b", 1), (a, "a", 0)):
        on.set_gumbel(16)
        with pytest.raises(AzxError, match=r"azx error -1: engine %s has the Gumbel root search set" % name):
            m.play(4)
        with pytest.raises(AzxError, match=r"azx error -1: engine %d has the Gumbel root search set" % idx):
            t.play([(0, 1)], 4)
        assert state() == before                              # both engines' slots and queues are as they were
        on.clear_gumbel()
    res = m.play(8)                                           # after clearing, it plays
    assert (res["outcome"] != 0).all() and (res["length"] >= 9).all()
    m.close()
    t.close()
    a.close()
    b.close()
