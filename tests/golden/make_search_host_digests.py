"""Writes tests/golden/search_host_digests.json: a SHA-256 per case over what small searches and self-play calls leave
behind.  tests/test_gpu_search_host_digests.py reads the file, replays the same cases through `run_case` below and
compares; it never writes it.

Made ONCE, on the commit BEFORE the host code that issues a search's launches was folded into one phase sequence
(DESIGN 7.21), with that commit's library and Python: the fixture is what says the one sequence enqueues what the five
hand-written ones did, under every driver -- azx_search per evaluator, the phase API, azx_play_steps by persistent
launches, per-move launches and the two half-pools, and azx_play.  Needs a GPU.  Every case is run twice and nothing is
written when the two runs differ.

    python tests/golden/make_search_host_digests.py [--out FILE]
    python tests/golden/make_search_host_digests.py --case NAME      (prints that case's digest and writes nothing)

The engines, seeds, agent settings and the seeded 1x16 network are those of make_match_host_digests.py (imported, with
single settings overridden): a 5x5 board, 8 slots, 20 simulations in batches of 5, so a search's phases are 0..5; the
pipelined cases take 1024 slots, the smallest pool the half-pools are used for.  Rows are hashed as that script hashes
them: whole games by game_uid, a game's rows in queue order (its docstring says why).

A search digest covers get_root() and tree_dump() of slots 0 and 7, after a search from a reset and after a second one
on the root kept by an advance.  A phase API digest adds every n_pending that begin and the steps return, the last
included (the count after the final APPLY).  A self-play value is "<sha>|mcts_launches,mcts_kernel_launches,
net_launches": the SHA-256 covers the other integer fields of the stats, get_games(), the engine's counters and, where
the call returns rows, the rows and their metrics; the launch counts of each call stand beside it, and for azx_play_steps
the way the engine says it plays its moves (azx_kernel_info's "play="), so that the pipelined modes, which play the same
games by different launches, can be held to each other.  (azx_play_steps leaves its rows in a queue no
call reads back: its cases are pinned by the games and the counters, the rows by the azx_play cases.)
"""
import argparse
import functools
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "search_host_digests.json")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mm = _load("make_match_host_digests")

N, AGENT, BIG = 5, 1, 1024
# The bounded queue of the parked cases.  A finished game's wave reserves its rows with an atomicAdd on the queue's row
# count and gives them back when they do not fit (advance_body in azalea_amd/csrc/mcts_kernels.hip), so under a bound
# that SOME games fit, which of the games that finish in one launch get in depends on the order their waves arrive in --
# and a game that would fit can meet another's reservation not yet given back.  That is not fixed from run to run (a
# 16-row queue gave two different second calls in two runs), so the digests take a bound below the shortest game,
# 2N - 1 rows: every game parks whatever the order.  tests/test_gpu_search_host_digests.py runs the 16-row queue too
# and asserts what holds in every order.
PARK_CAP = 2 * N - 2
FPU = ("reduction", 0.0, 0.25, 0.0)
INT_STATS = ("positions", "games", "game_errors", "plies", "selects", "evals", "sum_depth", "sum_k_interior", "sum_k_leaf")
LAUNCHES = ("mcts_launches", "mcts_kernel_launches", "net_launches")
TREE_KEYS = ("parent", "first_child", "num_children", "num_visits", "total_value", "prior_prob")


class _Override:
    """The engine module as make_match_host_digests.engine takes it, with single Engine settings overridden."""

    def __init__(self, eng, **over):
        self.eng, self.over = eng, over

    def __getattr__(self, name):
        return getattr(self.eng, name)

    def Engine(self, **kw):
        kw.update(self.over)
        return self.eng.Engine(**kw)


def engine(eng, kind, slots=mm.SLOTS, **over):
    """kind 'hash', 'ext', 'net': the match script's engines; 'uniform': the uniform evaluator with the default prior
    (the fast instantiation, and k_play in self-play); 'rollout': the rollout evaluator with 4 rollouts; 'external': an
    EVAL_EXTERNAL engine with nothing registered (the phase API's)."""
    if kind == "uniform":
        return mm.engine(_Override(eng, evaluator=eng.EVAL_UNIFORM, **over), N, AGENT, "hash", slots)
    if kind in ("rollout", "external"):
        E = mm.engine(_Override(eng, evaluator=eng.EVAL_EXTERNAL, **over), N, AGENT, "hash", slots)
        if kind == "rollout":
            E.set_rollout_evaluator(4, seed=77)
        return E
    return mm.engine(_Override(eng, **over), N, AGENT, kind, slots)


def stub():
    if mm.TESTS not in sys.path:
        sys.path.insert(0, mm.TESTS)
    from test_gpu_external_eval import uniform_hash_evaluator
    return uniform_hash_evaluator(N * N)


def add_trees(h, E):
    root = E.get_root()
    for k in sorted(root):
        h.update(np.ascontiguousarray(root[k]).tobytes())
    for slot in (0, E.G - 1):
        t = E.tree_dump(slot)
        for k in TREE_KEYS:
            h.update(np.ascontiguousarray(t[k]).tobytes())
        h.update(np.asarray([t["num_nodes"], t["root_id"]], np.int64).tobytes())
    return root


def host_noise(E):
    return np.random.RandomState(5).dirichlet([0.3] * E.cells, size=(E.G, E.selects_per_search)).astype(np.float64)


def two_searches(E, h, search):
    """`search()` from a reset and again on the root an advance kept (phase 0 then finds the root evaluated)."""
    E.reset()
    search()
    root = add_trees(h, E)
    E.advance(np.argmax(root["child_visits"], axis=1).astype(np.int32))
    search()
    add_trees(h, E)


def search_case(eng, kind, noise=False, **over):
    E = engine(eng, kind, **over)
    h = hashlib.sha256()
    try:
        kw = dict(noise=host_noise(E), noise_scale=0.25) if noise else {}
        two_searches(E, h, lambda: E.search(**kw))
    finally:
        E.close()
    return h.hexdigest()


def record_pending(E, seen):
    """Every n_pending that E.search_begin and E.search_step return from here on, appended to `seen`."""
    begin, step = E.search_begin, E.search_step

    def search_begin(*a, **kw):
        n = begin(*a, **kw)
        seen.append(n)
        return n

    def search_step():
        n, done = step()
        seen.append(n)
        return n, done
    E.search_begin, E.search_step = search_begin, search_step


def phase_case(eng, kind):
    import torch
    E = engine(eng, kind)
    h = hashlib.sha256()
    seen = []
    record_pending(E, seen)
    try:
        if kind == "net":
            def search():
                for slot, k, v, p in E.search_recorded():
                    h.update(np.asarray([slot, k], np.int64).tobytes())
                    h.update(np.float32(v).tobytes())
                    h.update(np.ascontiguousarray(p).tobytes())
        else:
            fn = stub()

            def evaluate(b, lm, slot, k):
                kmax = int(k.max())
                v, p = fn(torch.tensor(b, device="cuda:0"), torch.tensor(lm[:, :kmax], device="cuda:0"))
                return v.cpu().numpy(), p.cpu().numpy()

            def search():
                E.search_external(evaluate)
        two_searches(E, h, search)
    finally:
        E.close()
    assert len(seen) == 2 * (E.num_batches + 2), seen        # begin and num_batches + 1 steps per search
    h.update(np.asarray(seen, np.int64).tobytes())
    return h.hexdigest()


def play_value(h, stats_list):
    for st in stats_list:
        h.update(np.asarray([st[k] for k in INT_STATS], np.int64).tobytes())
    return h.hexdigest() + "|" + ";".join(",".join(str(st[k]) for k in LAUNCHES) for st in stats_list)


def add_state(h, E):
    games = E.get_games()
    for k in sorted(games):
        h.update(np.ascontiguousarray(games[k]).tobytes())
    h.update(np.ascontiguousarray(E.debug_counters()).tobytes())


def steps_case(eng, kind, plies=6, slots=mm.SLOTS, fpu=None):
    """play_steps(plies) twice on one engine: the second call starts from the trees and counters the first left."""
    E = engine(eng, kind, slots)
    h = hashlib.sha256()
    try:
        if fpu:
            E.set_fpu(*fpu)
        stats = [E.play_steps(plies), E.play_steps(plies)]
        add_state(h, E)
        how = E.kernel_info().split("play=")[1].split(";")[0]
    finally:
        E.close()
    return play_value(h, stats) + "|" + how


def play_case(eng, kind, queue_cap=0, **kw):
    """play(40) twice on one engine; under a queue of `queue_cap` rows every slot parks, the call ends at the check for
    that, and the second call begins with the parked slots' rejoin."""
    E = engine(eng, kind)
    h = hashlib.sha256()
    stats = []
    try:
        if queue_cap:
            E.debug_set_queue_cap(queue_cap)
        for _ in range(2):
            rows, st = E.play(40, **kw)
            if st["positions"]:                               # (none under PARK_CAP)
                mm.add_rows(h, dict(rows=rows, row_metrics=E.play_row_metrics(), n_rows=st["positions"]))
            stats.append(st)
        add_state(h, E)
    finally:
        E.close()
    return play_value(h, stats)


CASES = {
    "search_hash": lambda eng: search_case(eng, "hash"),
    "search_uniform": lambda eng: search_case(eng, "uniform"),
    "search_net": lambda eng: search_case(eng, "net"),
    "search_ext": lambda eng: search_case(eng, "ext"),
    "search_rollout": lambda eng: search_case(eng, "rollout"),
    "search_hash_noise": lambda eng: search_case(eng, "hash", noise=True),
    "search_net_noise": lambda eng: search_case(eng, "net", noise=True),
    "search_net_one_batch": lambda eng: search_case(eng, "net", simulations=5),
    "phase_recorded_net": lambda eng: phase_case(eng, "net"),
    "phase_external": lambda eng: phase_case(eng, "external"),
    "steps_uniform": lambda eng: steps_case(eng, "uniform"),
    "steps_net": lambda eng: steps_case(eng, "net"),
    "steps_ext": lambda eng: steps_case(eng, "ext"),
    "steps_rollout": lambda eng: steps_case(eng, "rollout"),
    "steps_net_fpu": lambda eng: steps_case(eng, "net", fpu=FPU),
    "steps_net_big": lambda eng: steps_case(eng, "net", plies=3, slots=BIG),
    "play_uniform": lambda eng: play_case(eng, "uniform"),
    "play_net": lambda eng: play_case(eng, "net"),
    "play_uniform_parked": lambda eng: play_case(eng, "uniform", queue_cap=PARK_CAP),
    "play_net_parked": lambda eng: play_case(eng, "net", queue_cap=PARK_CAP),
    "play_net_ply_cap": lambda eng: play_case(eng, "net", max_plies=3),
}
# cases made in a child process, under switches that azx_create reads from the environment: name -> (case, environment)
CHILDREN = {
    "steps_uniform_per_move": ("steps_uniform", {"AZX_NO_PERSISTENT": "1"}),
    "steps_net_big_pipelined": ("steps_net_big", {}),
    "steps_net_big_no_stagger": ("steps_net_big", {"AZX_PIPELINE_STAGGER": "0"}),
    "steps_net_big_one_stream": ("steps_net_big", {"AZX_PIPELINE": "0"}),
}
IN_CHILD_ONLY = ("steps_net_big",)                 # no fixture entry of its own: its three modes are, and play the same games
SAME_GAMES = ("steps_net_big_pipelined", "steps_net_big_no_stagger", "steps_net_big_one_stream")
SAME_TREES = ("search_hash", "search_ext")         # the registered stub computes what the inline evaluator does


def games_of(value):
    """The part of a self-play value that the games decide (everything but the launch counts)."""
    return value.split("|")[0]


def fresh_case(name):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from azalea_amd import engine as eng
    return CASES[name](eng)


run_case = functools.lru_cache(maxsize=None)(fresh_case)     # the tests share a case's digest


def child_case(name):
    """The case CHILDREN[name] in a fresh process under its environment."""
    case, env = CHILDREN[name]
    clean = {k: v for k, v in os.environ.items() if k not in ("AZX_NO_PERSISTENT", "AZX_PIPELINE", "AZX_PIPELINE_STAGGER")}
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], env=dict(clean, **env), check=True,
                         stdout=subprocess.PIPE, timeout=300).stdout.decode()
    return out.strip().splitlines()[-1]


def collect():
    out = {name: fresh_case(name) for name in CASES if name not in IN_CHILD_ONLY}
    out.update({name: child_case(name) for name in CHILDREN})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--case", default=None)
    args = ap.parse_args()
    if args.case is not None:
        print(fresh_case(args.case))
        return
    first, second = collect(), collect()
    if first != second:
        for name in first:
            if first[name] != second[name]:
                print("case %s differs between two runs:\n  %s\n  %s" % (name, first[name], second[name]))
        raise SystemExit("two runs differ: nothing written")
    if len({games_of(first[name]) for name in SAME_GAMES}) != 1 or first[SAME_TREES[0]] != first[SAME_TREES[1]]:
        raise SystemExit("cases that must agree differ: nothing written\n%s" % json.dumps(first, indent=1))
    with open(args.out, "w") as f:
        json.dump(first, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (args.out, len(first)))


if __name__ == "__main__":
    main()
