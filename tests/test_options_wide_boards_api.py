"""The inputs of tests/test_gpu_options_wide_boards.py, held on the CPU: the position families of
tests/option_positions.py (9x9 to 13x13, roots of two and three 64-lane words) must make the references do what the
device tests are there to compare -- forced children, pruned children and early-stop leaders in every word of the root
-- and the numpy restatement of the search, rule off, must equal the unmodified oracle bit for bit on every one of
them, as tests/test_forced_playouts_api.py pins it on 5x5.  These are conditions on the inputs, asserted on the
references alone; no expected value is stored.

Two cells of the table cannot be filled by a win-at-rank position and are not asserted (the wide-hash and sweep rows
cover those words): a winning chain takes n - 1 stones of each colour, so such a root has k = n*n - 2n + 2 children --
65 on 9x9, where word 1 is the single lane 64 (the leader when the win lies there, so never pruned), and 122 on 12x12,
where there is no third word."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import early_stop_reference as es  # noqa: E402
import forced_playouts_reference as fp  # noqa: E402
import option_positions as op  # noqa: E402

f32 = np.float32
# words of the root a win-at-rank position can put a pruned child / a stopping leader in (the module docstring)
WIN_PRUNED_WORDS = {9: 1, 11: 2, 12: 2, 13: 3}
WIN_LEADER_WORDS = {9: 2, 11: 2, 12: 2, 13: 3}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_default_settings_are_the_5x5_setup():
    d = es.DEFAULT
    assert (d.n, d.cells, d.sims, d.bs, d.c_puct, d.nb, d.tree_cap) == (5, 25, 200, 10, 0.5, 21, 1 << 16)
    assert (es.N, es.CELLS, es.SIMS, es.BS, es.C_PUCT, es.NB) == (fp.N, fp.CELLS, fp.SIMS, fp.BS, fp.C_PUCT, fp.NB) == (5, 25, 200, 10, 0.5, 21)
    want = (f32(1.0) / np.arange(0, 26).clip(1).astype(f32)).astype(f32)
    assert np.array_equal(bits(es.TABLE), bits(want)) and np.array_equal(bits(fp.TABLE), bits(want))
    s = op.narrow(13)
    assert hash(s) == hash(op.narrow(13)) and s == op.narrow(13) and s != op.wide(13)
    assert len(s.table) == 170 and s.table[169] == f32(1.0) / f32(169) and s.nb == 41


@pytest.mark.parametrize("n", op.BOARDS)
def test_every_prefix_is_a_legal_unfinished_game_of_the_stated_width(n):
    cells = n * n
    families = dict(sweep=op.sweep_prefixes(n), win=tuple(p for p, _ in op.win_prefixes(n)),
                    wide_hash=op.wide_hash_prefixes(n), stop_hash=op.stop_hash_prefixes(n),
                    tied_max=op.tied_max_prefixes(n))
    for name, prefixes in families.items():
        assert 3 <= len(prefixes) <= 128, name
        for p in prefixes:
            h = es.game_at([], op.narrow(n))
            for m in p:                                         # step by step: every move legal, the game unfinished before it
                assert h.result == 0 and m in h.legal_moves(), (name, p)
                h.step(m)
            assert h.result == 0 and len(h.legal_moves()) == cells - len(p), (name, p)
    ks = sorted(cells - len(p) for p in families["sweep"])
    if n == 9:
        assert all(65 <= k <= 81 for k in ks)                    # the smallest two-word case
    if n == 12:
        assert all(129 <= k <= 144 for k in ks)                  # the third word holds 16 lanes or fewer
    if n == 13:                                                 # RS 3, 2 and 1 inside the SLOTS = 3 kernels
        assert ks[-1] > 128 and any(64 < k <= 128 for k in ks) and ks[0] <= 64
    for p, rank in op.win_prefixes(n):                          # the stated rank is the winning child's
        h = es.game_at(p, op.narrow(n))
        assert h.color == 0 and len(p) == 2 * (n - 1)
        h.step(int(h.legal_moves()[rank]))
        assert h.result != 0, (p, rank)
    assert len(op.forced_set(n, "uniform")[1]) <= 128 and len(op.forced_set(n, "hash")[1]) <= 128


PINNED = [(n, f) for n in op.BOARDS for f in ("sweep", "win", "wide_hash", "tied_max")] + [(n, "wider_hash") for n in op.WIDER_BOARDS]


@pytest.mark.parametrize("n,family", PINNED)
def test_the_restatement_with_the_rule_off_is_the_unmodified_oracle_bit_for_bit(n, family):
    kind, cfg = {"wide_hash": ("hash", op.wide(n)), "tied_max": ("hash", op.wide(n)), "wider_hash": ("hash", op.wider(n))}.get(family, ("uniform", op.narrow(n)))
    for r in op.forced_refs(n, family):                         # every position: none may be dropped
        nv, tv, pp = fp.oracle_root(r["prefix"], kind, cfg)
        assert np.array_equal(bits(nv), bits(r["off_n"])), r["prefix"]
        assert np.array_equal(bits(tv), bits(r["off_w"])), r["prefix"]
        assert np.array_equal(bits(pp), bits(r["off_p"])), r["prefix"]
        assert len(nv) == n * n - len(r["prefix"])
        assert 0 < r["off_n"].sum() <= cfg.sims + cfg.bs and 0 < r["n"].sum() <= cfg.sims + cfg.bs
        assert len(r["forced_at"]) == r["forced"] and (r["r"] <= r["n"]).all() and r["r"].max() == r["n"].max()


@pytest.mark.parametrize("n", op.BOARDS)
def test_forced_and_pruned_children_lie_in_every_word(n):
    W = op.words_of(n)
    assert W == (2 if n <= 11 else 3)
    sweep, win, hashed = (op.forced_refs(n, f) for f in ("sweep", "win", "wide_hash"))
    forced = op.by_word([i for r in sweep for i in r["forced_at"]], W)
    pruned_win = op.by_word(op.pruned_children(win), W)
    pruned_hash = op.by_word(op.pruned_children(hashed), W)
    forced_hash = op.by_word([i for r in hashed for i in r["forced_at"]], W)
    print("%dx%d by word: forced selects (sweep) %s, pruned children (win-at-rank) %s, wide-hash forced selects %s and "
          "pruned children %s" % (n, n, forced, pruned_win, forced_hash, pruned_hash))
    assert all(c >= 20 for c in forced), forced
    assert all(c >= 5 for c in pruned_win[:WIN_PRUNED_WORDS[n]]), pruned_win
    assert pruned_hash[0] >= 5 and pruned_hash[1] >= 5, pruned_hash
    assert any(r["overrode"] > 0 for r in sweep) and any(r["overrode"] > 0 for r in hashed)
    if n in op.WIDER_BOARDS:                                    # "hash" at c_puct 12: pruned children in the third word too
        wider = op.forced_refs(n, "wider_hash")
        pruned_wider = op.by_word(op.pruned_children(wider), W)
        print("%dx%d wider-hash by word: forced selects %s, pruned children %s"
              % (n, n, op.by_word([i for r in wider for i in r["forced_at"]], W), pruned_wider))
        assert all(c >= 5 for c in pruned_wider), pruned_wider


@pytest.mark.parametrize("n", op.BOARDS)
def test_some_maxima_are_shared_across_words_and_the_first_one_matters(n):
    """The prune measures against the FIRST most-visited child: at least 3 positions per board would be pruned
    differently against the most-visited child of a later word."""
    cfg = op.wide(n)
    telling = 0
    for r in op.forced_refs(n, "tied_max"):
        b = op.later_maximum(r["n"])
        assert b is not None and b >> 6 > int(np.argmax(r["n"])) >> 6, r["prefix"]
        telling += not np.array_equal(r["r"], fp.prune(r["n"], r["w"], r["p"], op.K_FORCED, cfg.c_puct, b=b))
    assert telling >= 3


@pytest.mark.parametrize("n", op.BOARDS)
def test_early_stop_leaders_lie_in_every_word(n):
    W = op.words_of(n)
    cfg = op.narrow(n)
    (win, _), (hashed, dropped), (sweep, _) = (op.stop_refs(n, f) for f in ("win", "stop_hash", "sweep"))
    assert dropped <= es.MAX_DROPPED_SHARE * (len(hashed) + dropped)
    stopping = [r for r in win + hashed if r["b_star"] < cfg.nb]
    leaders = op.by_word([r["leader"] for r in stopping], W)
    high = [r for r in hashed if r["b_star"] < cfg.nb and not r["ends"] and r["leader"] >= 64]
    never = [r for r in win + hashed + sweep if r["b_star"] == cfg.nb]
    print("%dx%d: stopping leaders by word %s (win-at-rank and stop-hash), of the stop-hash ones non-terminal above "
          "word 0 %d, never stopping %d" % (n, n, leaders, len(high), len(never)))
    assert all(c >= 3 for c in leaders[:WIN_LEADER_WORDS[n]]), leaders
    assert len(high) >= 3 and len(never) >= 3
    assert all(r["ends"] for r in win)                          # the winning move ends the game: read it from the row
    for r in win + hashed:
        assert 1 <= r["b_star"] <= cfg.nb and r["leader"] == r["full_leader"], r["prefix"]
    assert len(op.stop_set(n, "uniform")[1]) <= 128 and len(op.stop_set(n, "hash")[1]) <= 128


def test_the_references_beyond_the_sqrt_table_agree_with_the_oracle():
    """5x5 at 4300 simulations: the root's visit sum passes 4096 (AZX_SQRT_TAB), where the kernel takes sqrtf."""
    for r in op.long_refs():
        nv, tv, pp = fp.oracle_root(r["prefix"], "uniform", op.LONG)
        assert np.array_equal(bits(nv), bits(r["off_n"])) and np.array_equal(bits(tv), bits(r["off_w"]))
        assert r["off_n"].sum() > 4096 + 100 and r["n"].sum() > 4096 + 100 and r["forced"] > 0
