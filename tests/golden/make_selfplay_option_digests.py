"""Writes tests/golden/selfplay_option_digests.json: what one small network-free self-play engine produces under every
self-play option (none, each alone, all the library takes together, the Gumbel root search with the options it goes
with), as exact integers and digests.  tests/test_gpu_selfplay_option_digests.py reads the file, runs the same cases
through `collect` below and compares; it never writes it.

Made ONCE, on the commit BEFORE the options' host plumbing was folded into tables, with that commit's
library and Python: the fixture is what says the tables hand the kernels the values the seven hand-written copies did.
Needs a GPU.  Every case is run twice and nothing is written when the two runs differ.

    python tests/golden/make_selfplay_option_digests.py

A case is: a fresh engine, the options set in the order Player applies them, one play of PLIES plies per slot.  Per case
the fixture holds the seven stats dicts, the option fields of azx_kernel_info and a SHA-256 over the harvested rows and
their row metrics, whole games ordered by game_uid (the order games reach the harvest queue comes from an atomic and is
not fixed).  Where the library refuses a setting the case holds the refusal's text instead.
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "selfplay_option_digests.json")

N, G, SEED = 5, 64, 20261020
PLIES = 30                  # per slot and play: every slot finishes at least one 5x5 game (25 cells)
SHORT_PLIES = 3             # ... and no game can end in these (5 stones in a row at the least; RESIGN's min_ply)

BOOK = ([[13], [7, 19], []], [2.0, 1.0, 1.0])
CAP = (0.5, 8)
RESIGN = (-0.3, 8, 0.25)
TARGETS = ("visits", 0.5)
FORCED = (3.0, True)
GUMBEL = (4, 30.0, 0.5, True)

# (Engine setter, arguments) in the order Player applies the options
SETTERS = dict(selfplay_openings=("set_selfplay_openings", BOOK), playout_cap=("set_playout_cap", CAP),
               resign=("set_resign", RESIGN), early_stop=("set_early_stop", (True,)),
               train_targets=("set_train_targets", TARGETS), forced_playouts=("set_forced_playouts", FORCED),
               gumbel=("set_gumbel", GUMBEL))
ORDER = tuple(SETTERS)
CASES = dict([("none", ())] + [(name, (name,)) for name in ORDER] +
             [("all_but_gumbel", tuple(o for o in ORDER if o != "gumbel")),
              ("gumbel_with", ("selfplay_openings", "playout_cap", "resign", "train_targets", "gumbel"))])

CLEARERS = ("clear_selfplay_openings", "clear_playout_cap", "clear_resign", "clear_train_targets",
            "clear_forced_playouts", "clear_gumbel")

# mid-game positions for the search() of reset slots: slot g gets PREFIXES[g % len(PREFIXES)]
PREFIXES = ([], [13], [13, 7], [1, 25, 13, 12], [7, 19, 8, 18, 12], [3, 23, 9, 17, 11, 15])

ROW_KEYS = ("board", "color", "nlegal", "moves_prob", "reward", "game_uid")
ROOT_KEYS = ("k", "legal_moves", "child_visits", "child_value", "child_prior", "root_visits", "root_value",
             "num_nodes", "search_value")


def make_engine():
    from azalea_amd import engine as eng
    return eng.Engine(board_size=N, n_games=G, simulations=20, search_batch_size=4, exploration_coef=0.5,
                      exploration_depth=3, noise_alpha=0.3, noise_scale=0.25, temperature=1.0,
                      evaluator=eng.EVAL_UNIFORM_HASH, seed=SEED)


def apply_options(E, names):
    """The setters of `names`, in ORDER; the text of the first refusal, or None."""
    for name in ORDER:
        if name in names:
            setter, args = SETTERS[name]
            try:
                getattr(E, setter)(*args)
            except (ValueError, RuntimeError) as exc:
                return "%s: %s" % (name, exc)
    return None


def clear_options(E):
    for name in CLEARERS:
        getattr(E, name)()
    E.set_early_stop(False)


def play(E, plies=PLIES):
    """One play of `plies` plies per slot: (rows, row metrics, play stats).  More rows are asked for than the plies can
    record, so max_plies ends the call and the set of finished games does not depend on timing."""
    rows, st = E.play(4 * G * N * N, max_plies=plies)
    return rows, E.play_row_metrics(), st


def rows_digest(rows, metrics):
    """SHA-256 over the rows and their metrics with whole games ordered by game_uid (a game's rows keep their order)."""
    order = np.argsort(rows["game_uid"], kind="stable")
    h = hashlib.sha256()
    for k in ROW_KEYS:
        h.update(np.ascontiguousarray(rows[k][order]).tobytes())
    h.update(np.ascontiguousarray(metrics[order]).tobytes())
    return h.hexdigest()


def root_digest(root):
    h = hashlib.sha256()
    for k in ROOT_KEYS:
        h.update(np.ascontiguousarray(root[k]).tobytes())
    return h.hexdigest()


def option_fields(info):
    """The option fields of an azx_kernel_info line, as a dict."""
    return dict(re.findall(r" (cap|resign|estop|targets|forced|gumbel|book)=([^ ;]+)", info))


def all_stats(E):
    book = {k: [int(x) for x in v] for k, v in E.selfplay_openings_stats().items()}
    return dict(playout_cap=E.playout_cap_stats(), resign=E.resign_stats(), early_stop=E.early_stop_stats(),
                train_targets=E.train_targets_stats(), forced_playouts=E.forced_playouts_stats(),
                gumbel=E.gumbel_stats(), selfplay_openings=book)


def searched_roots(E):
    """search() (no noise) on every slot reset to its PREFIXES position: the digest of the root arrays."""
    E.reset(moves=[list(PREFIXES[g % len(PREFIXES)]) for g in range(G)])
    E.search()
    return root_digest(E.get_root())


def run_case(names):
    E = make_engine()
    try:
        refused = apply_options(E, names)
        if refused is not None:
            return dict(refused=refused)
        info = option_fields(E.kernel_info())
        rows, metrics, st = play(E)
        return dict(info=info, stats=all_stats(E), games=int(st["games"]), rows=int(len(rows["reward"])),
                    digest=rows_digest(rows, metrics))
    finally:
        E.close()


def run_cleared():
    """An engine that played SHORT_PLIES plies under every option the library takes together (no game ends in them, so
    no slot has used up a uid), then had every option cleared and was reset(): its play, beside that of a fresh engine
    after the same reset()."""
    out = {}
    for label, names in (("fresh", ()), ("cleared", CASES["all_but_gumbel"])):
        E = make_engine()
        try:
            if names:
                assert apply_options(E, names) is None
                _, _, st = play(E, SHORT_PLIES)
                assert st["games"] == 0, "a game ended inside the short play: the uids would differ"
                clear_options(E)
            E.reset()
            info = option_fields(E.kernel_info())
            rows, metrics, st = play(E)
            out[label] = dict(info=info, games=int(st["games"]), digest=rows_digest(rows, metrics))
        finally:
            E.close()
    return out


def run_search_after_options():
    """search() after a whole play under every option the library takes together, the options still set: the root
    arrays' digest, beside a fresh engine's."""
    out = {}
    for label, names in (("fresh", ()), ("after_all_options", CASES["all_but_gumbel"])):
        E = make_engine()
        try:
            if names:
                assert apply_options(E, names) is None
                play(E)
            out[label] = searched_roots(E)
        finally:
            E.close()
    return out


def collect():
    return dict(engine=dict(board_size=N, n_games=G, seed=SEED, plies=PLIES),
                cases={name: run_case(names) for name, names in CASES.items()},
                cleared=run_cleared(), search=run_search_after_options())


def main():
    sys.path.insert(0, ROOT)
    first, second = collect(), collect()
    if first != second:
        for name in first["cases"]:
            if first["cases"][name] != second["cases"][name]:
                print("case %s differs between two runs:\n  %r\n  %r" % (name, first["cases"][name], second["cases"][name]))
        raise SystemExit("two runs differ: nothing written")
    with open(FIXTURE, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (FIXTURE, len(first["cases"])))


if __name__ == "__main__":
    main()
