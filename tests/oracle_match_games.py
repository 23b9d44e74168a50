"""Two-agent evaluation games by the CPU oracle under numpy's RandomState: the reference side of
tests/test_gpu_match.py.

TEST INFRASTRUCTURE (imports oracle/).  A game is evaluation.worker + play_game + Policy.choose_action
(evaluation.py:60-80, play_game.py:27-52, policy.py:132-176) built from the oracle's existing pieces only: one `Hex`,
one `Tree` and one `RandomState` PER AGENT; the mover's agent searches with its own settings (simulations, batch,
c_puct, noise, depth, temperature: `rng.dirichlet` once per select_leaf, mcts.py:126-131), draws
`argmax(rng.multinomial(1, as_distribution(visits, T)))` (policy.py:160) and BOTH trees move to that child
(search_tree.py:115-132).  The evaluator is the stub network of the golden games (uniform priors, board-hash value).
Game u is first moved by agent u & 1 (the engine's alternation; the reference flips a coin per game), and its two
RandomStates are seeded seed0 + 2u + a + 1.

Run as a script in its own process (the GPU tests start it with subprocess so that the fork pool never inherits an
initialised HIP runtime):

    python tests/oracle_match_games.py --n 7 --games 4096 --seed0 0 --out /tmp/a.npz \\
        --agents '[{"sims": 60, "batch": 10, "c": 0.5, "depth": 6, "eps": 0.0, "alpha": 0.3, "temp": 1.0}, {...}]'
"""
import argparse
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MAX_PROCS = 16


def prior_table(n):
    """f32(1/k): the uniform prior the reference's stub network hands a position with k legal moves."""
    return (np.float32(1.0) / np.arange(0, n * n + 1).clip(1).astype(np.float32)).astype(np.float32)


def _one(args):
    n, cfgs, u, seed0 = args
    from oracle import oracle as orc
    ev = orc.UniformEval(hash_value=True, prior_by_k=prior_table(n))
    game = orc.Hex(n)
    trees = [orc.Tree(1 << 18), orc.Tree(1 << 18)]
    rngs = [np.random.RandomState(seed0 + 2 * u + a + 1) for a in range(2)]
    first = u & 1
    ply = 0
    while not game.result:
        a = (first + ply) & 1
        c = cfgs[a]
        temp = c["temp"] if ply < c["depth"] else 0.0            # policy.py:142-149: T is gated by depth, noise is not
        lm = game.legal_moves()
        noise = None
        if c["eps"]:
            sel = (c["sims"] // c["batch"] + 1) * c["batch"]     # mcts.py:268
            noise = np.array([rngs[a].dirichlet(np.full(len(lm), c["alpha"])) for _ in range(sel)])
        st = orc.search(trees[a], game, ev, c["sims"], c["batch"], c["c"], c["eps"], noise)
        assert not st.status
        probs = orc.as_distribution(trees[a].root_stats()[0], temp)
        mid = int(np.argmax(rngs[a].multinomial(1, probs)))
        for t in trees:                                          # every agent follows the move (policy.py:170-176)
            t.move(mid)
        game.step(int(lm[mid]))
        ply += 1
    winner_color = 1 if game.result == 3 else 2                  # result 3: the first player (X) won
    winner_agent = first if winner_color == 1 else 1 - first
    return ply, winner_agent, int(winner_color == 1), first


def sample(n, cfgs, games, seed0, procs=None):
    from oracle import oracle as orc
    orc.lib()                                  # built and loaded once, before the workers fork
    procs = max(1, min(MAX_PROCS, procs or (os.cpu_count() or 2) - 1))
    work = [(n, cfgs, u, seed0) for u in range(games)]
    if procs == 1:
        r = [_one(w) for w in work]
    else:
        with mp.get_context("fork").Pool(procs) as pool:
            r = pool.map(_one, work, chunksize=16)
    r = np.array(r)
    return dict(length=r[:, 0].astype(np.int32), agent0_wins=(r[:, 1] == 0).astype(np.int8),
                first_wins=r[:, 2].astype(np.int8), agent0_first=(r[:, 3] == 0).astype(np.int8))


def compare(a, b):
    """Two-sample p-values (tests/game_stats.py) of two match samples: game-length histogram, agent-0 wins,
    first-player wins, and agent-0 wins among the games it moved first in and among those it moved second in."""
    import game_stats as gs

    def prop(x, y, key, sel=None):
        xs = x[key] if sel is None else x[key][x["agent0_first"] == sel]
        ys = y[key] if sel is None else y[key][y["agent0_first"] == sel]
        return gs.proportion_test(int(xs.sum()), len(xs), int(ys.sum()), len(ys))

    return {"length": gs.chi2_two_sample(a["length"], b["length"]),
            "agent0_wins": prop(a, b, "agent0_wins"),
            "first_player_wins": prop(a, b, "first_wins"),
            "agent0_wins_when_first": prop(a, b, "agent0_wins", 1),
            "agent0_wins_when_second": prop(a, b, "agent0_wins", 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--agents", required=True, help="JSON list of the two agents' settings")
    ap.add_argument("--games", type=int, required=True)
    ap.add_argument("--seed0", type=int, default=0)
    ap.add_argument("--procs", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    cfgs = json.loads(a.agents)
    assert len(cfgs) == 2
    np.savez_compressed(a.out, **sample(a.n, cfgs, a.games, a.seed0, a.procs or None))


if __name__ == "__main__":
    main()
