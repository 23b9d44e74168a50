"""Round-robin tournament between policies (azalea/evaluation.py:17-80), SURVEY 8(f).3.

`evaluate` keeps the reference's schedule: pairs (i, j), i < j in `gen_pairs` order, one game per
pair and round, task seed `10000 * round + index`, first player by a coin flip of
`RandomState(seed)`, both agents re-seeded from the same stream, outcome = order * (result - 2)
(+1: the pair's first agent won).  Games run in this process, one after the other, through
`play_game` -- every agent's search runs on its own engine.

`evaluate_batched` plays all games of a round concurrently on the GPU when every agent is a
`Policy` with a device network: per agent one engine holds a slot for each of its games, a ply
searches only the slots whose turn it is (`azx_set_active`), and every game keeps the private
RandomStates the sequential schedule would give it, so the outcomes are the same games, move for
move.

`evaluate_throughput` is the throughput form of the same round robin: a pair's games are played by two
engines against each other entirely on the device (`engine.Match`, azx_match_*), the move draws come from
the device RNG, and the first mover alternates instead of following a coin flip -- the reference's
algorithm as a distribution, not game for game.
"""
import logging
import os
from collections import defaultdict
from typing import Dict, List, Tuple

import numpy as np

from . import fpu as _fpu
from . import policy_temp as _ptemp
from .play_game import play_game

Pair = Tuple[int, int]
OutcomeCounts = List[int]


def gen_pairs(num_players: int) -> List[Pair]:
    """Round-robin pair ordering (evaluation.py:39-44)."""
    return [(i, j) for j in range(num_players) for i in range(j)]


def _tally(outcomes, pair, res, game, num_games):
    outcomes[pair][0] += (res > 0)    # first player of the pair wins
    outcomes[pair][1] += (res == 0)   # draws
    outcomes[pair][2] += (res < 0)    # second player wins
    winrate = outcomes[pair][0] / sum(outcomes[pair])
    logging.info("game %d/%d: pair %s: outcomes %s (wins %.2f)", game, num_games, pair, outcomes[pair], winrate)


def worker(pair: Pair, agents, seed: int) -> Tuple[Pair, int]:
    """One game of a pair (evaluation.py:60-80)."""
    rng = np.random.RandomState(seed)
    order = rng.choice([-1, 1])
    for a in agents:
        a.seed(rng.randint(1 << 32))
    result, _, _ = play_game(agents[::order])
    return pair, order * (result - 2)


def evaluate(agents, num_rounds: int, num_workers=None) -> Dict[Pair, OutcomeCounts]:
    """Round robin, `num_rounds` games per pair (evaluation.py:17-36).  `num_workers` is accepted
    for signature compatibility; there is no process pool."""
    outcomes: Dict[Pair, OutcomeCounts] = defaultdict(lambda: [0, 0, 0])
    pairs = gen_pairs(len(agents))
    num_games = num_rounds * len(pairs)
    game = 1
    for r in range(num_rounds):
        for s, pair in enumerate(pairs):
            _, res = worker(pair, (agents[pair[0]], agents[pair[1]]), 10000 * r + s)
            _tally(outcomes, pair, res, game, num_games)
            game += 1
    return outcomes


# ---------------------------------------------------------------------------------------------
# all games of the tournament at once, on the GPU
# ---------------------------------------------------------------------------------------------
def _device_policy(agent):
    from .policy import Policy
    pol = getattr(agent, "policy", None)
    if not isinstance(pol, Policy) or not pol._uses_device_net():
        raise TypeError("evaluate_batched needs agents whose Policy holds a HexNetwork")
    return pol


def evaluate_batched(agents, num_rounds: int, *, game_max_length: int = 300) -> Dict[Pair, OutcomeCounts]:
    """Same tournament as `evaluate` (same seeds, coin flips, per-game RandomStates, so the same
    games and tallies), with every game resident on the GPU at once: agent a's engine holds one
    slot per game a plays in and searches, each ply, the slots whose turn it is."""
    import torch
    from . import engine as _eng
    from .policy import SearchTreeFull, as_distribution

    pols = [_device_policy(a) for a in agents]
    n = agents[0].game.board_size
    pairs = gen_pairs(len(agents))
    # ---- the schedule of evaluation.py:24-57, with the worker's RNG draws (evaluation.py:69-75) ----
    games = []
    for r in range(num_rounds):
        for s, pair in enumerate(pairs):
            rng = np.random.RandomState(10000 * r + s)
            order = rng.choice([-1, 1])
            rngs = {}
            for a in pair:
                g_rng = np.random.RandomState()
                g_rng.seed(rng.randint(1 << 32) + 1)          # AzaleaAgent.seed -> policy.seed(s + 1)
                rngs[a] = g_rng
            first, second = (pair if order == 1 else pair[::-1])
            games.append(dict(pair=pair, order=order, rngs=rngs, players=(first, second),
                              game=agents[0].game.__class__(n), result=0, ply=0, slot={}))
    # ---- one engine per agent, one slot per game it plays in ----
    engines = []
    for a, pol in enumerate(pols):
        mine = [g for g in games if a in g["pair"]]
        for i, g in enumerate(mine):
            g["slot"][a] = i
        dev = pol.net.device
        eng = _eng.Engine(board_size=n, n_games=max(1, len(mine)), simulations=pol.simulations,
                          search_batch_size=pol.search_batch_size, exploration_coef=pol.exploration_coef,
                          exploration_depth=pol.exploration_depth, noise_alpha=pol.exploration_noise_alpha,
                          noise_scale=pol.exploration_noise_scale, temperature=pol.exploration_temperature,
                          evaluator=_eng.EVAL_RESNET, num_blocks=pol.num_blocks, base_chans=pol.base_chans,
                          device=(dev.index or 0) if dev.type == "cuda" else 0)
        _fpu.apply(eng, _fpu.policy_fpu(pol))                  # first-play urgency, if the policy carries it
        _ptemp.apply(eng, _ptemp.policy_policy_temp(pol))      # and its policy temperature
        pol.net.eval()
        sd = {k: v for k, v in pol.net.state_dict().items() if v.dtype == torch.float32}
        if dev.type == "cuda":
            eng.set_weights({k: (v.contiguous().data_ptr(), v.numel()) for k, v in sd.items()}, on_device=True)
        else:
            eng.set_weights({k: v.detach().cpu().numpy() for k, v in sd.items()})
        engines.append((eng, mine))
    try:
        for ply in range(game_max_length):
            alive = [g for g in games if not g["result"]]
            if not alive:
                break
            chosen = {}                                    # id(game) -> (move, move_id)
            for a, (eng, mine) in enumerate(engines):
                todo = [g for g in mine if not g["result"] and g["players"][g["ply"] % 2] == a]
                if not todo:
                    continue
                pol = pols[a]
                # Policy.choose_action's schedule (policy.py:132-149)
                temperature = noise_scale = 0.0
                if pol.settings["move_sampling"]:
                    temperature = pol.exploration_temperature
                    if pol.settings["move_exploration"]:
                        noise_scale = pol.exploration_noise_scale
                mask = np.zeros(eng.G, np.int32)
                noise = None
                if noise_scale:
                    noise = np.zeros((eng.G, eng.selects_per_search, n * n), np.float64)
                for g in todo:
                    slot = g["slot"][a]
                    mask[slot] = 1
                    if noise_scale:
                        k = len(g["game"].state.legal_moves)
                        alpha = np.full(k, pol.exploration_noise_alpha)
                        for j in range(eng.selects_per_search):
                            noise[slot, j, :k] = g["rngs"][a].dirichlet(alpha)
                eng.set_active(mask)
                eng.search(noise=noise, noise_scale=noise_scale)
                status = eng.get_status()
                root = eng.get_root()
                for g in todo:
                    slot = g["slot"][a]
                    if status[slot]:
                        raise SearchTreeFull("too many nodes")
                    legal = g["game"].state.legal_moves
                    k = len(legal)
                    assert int(root["k"][slot]) == k
                    t = 0.0 if g["ply"] >= pol.exploration_depth else temperature
                    probs = as_distribution(root["child_visits"][slot, :k], t)
                    move_id = int(np.argmax(g["rngs"][a].multinomial(1, probs)))
                    chosen[id(g)] = (int(legal[move_id]), move_id)
            # every agent follows every move of its games (Policy.execute_action, policy.py:170-176)
            for a, (eng, mine) in enumerate(engines):
                ids = np.full(eng.G, -1, np.int32)
                mask = np.zeros(eng.G, np.int32)
                for g in mine:
                    if not g["result"]:
                        ids[g["slot"][a]] = chosen[id(g)][1]
                        mask[g["slot"][a]] = 1
                if mask.any():
                    eng.set_active(mask)
                    eng.advance(ids)
            for g in alive:
                g["game"].step(chosen[id(g)][0])
                g["ply"] += 1
                g["result"] = int(g["game"].state.result)
        outcomes: Dict[Pair, OutcomeCounts] = defaultdict(lambda: [0, 0, 0])
        for i, g in enumerate(games):
            result = g["result"]
            if not result:
                logging.warning("game didn't terminate in %d moves", game_max_length)
                result = 2
            _tally(outcomes, g["pair"], g["order"] * (result - 2), i + 1, len(games))
        return outcomes
    finally:
        for eng, _ in engines:
            eng.close()


# ---------------------------------------------------------------------------------------------
# the tournament in throughput mode: every pair's games played on the device, no host in the ply loop
# ---------------------------------------------------------------------------------------------
def _throughput_policy(agent, external_batch=False):
    from .policy import Policy
    pol = getattr(agent, "policy", None)
    if not isinstance(pol, Policy):
        raise TypeError("evaluate_throughput needs agents whose policy is an azalea_amd Policy")
    if pol._uses_device_net():
        return pol
    from .rollout import is_rollout_net
    if is_rollout_net(pol.net):         # the rollout kernel is its evaluator: no torch in the loop, nothing to place
        return pol
    if not external_batch:
        raise TypeError("evaluate_throughput needs agents whose Policy holds a HexNetwork "
                        "(external_batch=True takes other networks)")
    from .parallel_player import _net_device
    dev = _net_device(pol.net)
    if dev.type != "cuda":
        raise ValueError("external_batch needs the network on a CUDA (ROCm) device, it is on %s" % dev)
    return pol


def evaluate_throughput(agents, num_rounds: int, *, n_slots=None, seed: int = 0,
                        games=None, external_batch: bool = False, pooled: bool = False,
                        collect=None, info=None, openings=None, gumbel=None) -> Dict[Pair, OutcomeCounts]:
    """Round robin of `evaluate` -- pairs in `gen_pairs` order, `num_rounds` games per pair -- with each
    pair's games played by the two agents' engines against each other on the device (azx_match_play):
    returns {(i, j): [wins of i, 0, wins of j]}.  One engine per agent, `n_slots` games resident at a time
    (default min(num_rounds, AZX_GAMES or 4096), rounded up to even); agent a's engine seed is derived from
    `seed` and a, and every pair plays its own range of game indices, so no two games of a call share a
    random stream.  The policies' `settings` are honoured as Policy.choose_action does (policy.py:132-149).
    `games`: optional dict that receives per pair dict(outcome, length, moves).  A game voided by a full
    search tree raises policy.SearchTreeFull (a policy attribute `nodes_per_game`, if set, sizes its engine's
    per-game arena; the engine's default otherwise).
    `external_batch`: an agent whose Policy holds a network other than HexNetwork, on a CUDA (ROCm) device, plays
    through an EVAL_EXTERNAL engine with policy.external_evaluator(net) registered: its net gets the leaf batches
    of all the slots in which it is the mover, on the device, at every evaluation point (ValueError when the
    network is not on such a device).  Agents with a HexNetwork keep the device tower, so fields may be mixed.
    An agent whose Policy holds a rollout.RolloutNet needs no `external_batch`: its engine gets the rollout kernel
    (Engine.set_rollout_evaluator; NOT the reference's behaviour) and `info` names it as eval=rollout(R).
    `pooled`: play all pairs in ONE ply loop (engine.Tournament, azx_tournament_play) instead of one match per pair
    after the other: the same games, tallies and `games` records, bit for bit.  `n_slots` stays "slots per engine"
    (default min((K - 1) * num_rounds, AZX_GAMES or 4096), rounded up to even): every engine's pool is shared out
    among its K - 1 opponents, max(1, n_slots // (K - 1)) tables per pair.
    `collect`: optional dict that receives, per pair, the replay rows of that pair's games -- evaluation games that
    double as training data: dict(rows=..., row_metrics=...) as engine.Match.play(collect=True) returns them (row p of
    a game from the agent that moved at ply p; game_uid = the game's index, pair s owning [s * num_rounds,
    (s + 1) * num_rounds); games in the order they settled).  The games and tallies are the same with or without.
    A policy attribute `tower_precision` ("f16": the plain-f16 tower, one MFMA per product, of the 6x64-class fused
    tower or of the wide 128 / 256-channel tower; opt-in and OUTSIDE every parity claim, policy.tower_flags) is honoured per agent, pooled or not: a match between the same weights at the
    two precisions is two agents that differ in that attribute.  `info`: optional dict that receives, per agent
    index, its engine's kernel_info() (which tower and heads kernels played).
    `openings`: an opening book, a list of move lists (tile + 1 in play order, colour 1 first; engine.all_openings
    makes the usual ones), handed to every match or to the one tournament: game u -- pair s plays u = s * num_rounds
    .. (s + 1) * num_rounds - 1 -- starts from opening (u >> 1) % len(openings), so rounds 2j and 2j + 1 of a pair are
    one opening with the colours swapped.  Use an EVEN num_rounds: with an odd one a pair's last opening is played
    one way round only and the following pairs' openings fall out of step with their colours.  Pooled or not, the
    games are the same; `games[pair]` gains "opening", the opening index of each game.  NOT the reference's
    behaviour, whose evaluation games all start from the empty board; off by default.  A ValueError with the
    library's message, before any engine is made, for a book the rules refuse (engine.openings_check).
    A policy attribute `fpu` (Policy.set_fpu, config["fpu"]; first-play urgency, Engine.set_fpu: NOT the reference's
    behaviour, off by default, OUTSIDE every parity claim) is honoured per agent, pooled or not: it is a property of an
    engine's search, not a self-play option, so a match between the same weights with and without it is two agents that
    differ in that attribute.  A policy attribute `policy_temp` (Policy.set_policy_temp, config["policy_temp"]; the
    policy temperature of the search's priors, Engine.set_policy_temp: NOT the reference's behaviour, off by default,
    OUTSIDE every parity claim) is honoured per agent in the same way.
    `gumbel`: refused.  The Gumbel root search (Engine.set_gumbel, Player(gumbel=...)) is a self-play option; device
    matches and tournaments search and draw every ply as the reference does.  Anything but None / False / 0 is a
    ValueError, before any engine is made."""
    import torch
    from .parallel_player import normalize_gumbel
    if normalize_gumbel(gumbel) is not None:
        raise ValueError("evaluate_throughput: gumbel is a self-play option: device matches and tournaments search and "
                         "draw every ply as the reference does (engine.Match refuses an engine with it set)")
    from . import engine as _eng
    from .policy import SearchTreeFull, tower_flags
    from .rollout import register_evaluator

    pols = [_throughput_policy(a, external_batch) for a in agents]
    flags = [tower_flags(pol) for pol in pols]           # a ValueError before any engine is made
    num_rounds = int(num_rounds)
    if num_rounds < 1:
        raise ValueError("num_rounds must be >= 1")
    pairs = gen_pairs(len(agents))
    if len(agents) > 256 or len(pairs) * num_rounds >= 1 << 32 or not 0 <= int(seed) < 1 << 24:
        raise ValueError("evaluate_throughput: at most 256 agents, 2^32 games and a seed below 2^24")
    n = agents[0].game.board_size
    openings = [[int(m) for m in o] for o in ([] if openings is None else openings)]
    _eng.openings_check(n, openings)
    opponents = max(1, len(agents) - 1)
    if n_slots is None:
        n_slots = min((opponents if pooled else 1) * num_rounds, int(os.environ.get("AZX_GAMES", "4096")))
    n_slots = max(2, int(n_slots) + (int(n_slots) & 1))
    if pooled:
        tables_per_pair = max(1, n_slots // opponents)
        n_slots = max(n_slots, tables_per_pair * opponents)      # (fewer slots than opponents: one table per pair)
    engines = []
    try:
        for a, pol in enumerate(pols):
            # Policy.choose_action's schedule (policy.py:132-149); the depth gate is the engine's
            temperature = noise_scale = 0.0
            if pol.settings["move_sampling"]:
                temperature = pol.exploration_temperature
                if pol.settings["move_exploration"]:
                    noise_scale = pol.exploration_noise_scale
            external = not pol._uses_device_net()
            if external:
                from .parallel_player import _net_device
                dev = _net_device(pol.net)
            else:
                dev = pol.net.device
            # game_rng keys on seed + uid: agent a's streams are [base_a, base_a + 2^32), disjoint between agents
            eng = _eng.Engine(board_size=n, n_games=n_slots, simulations=pol.simulations,
                              search_batch_size=pol.search_batch_size, exploration_coef=pol.exploration_coef,
                              exploration_depth=pol.exploration_depth, noise_alpha=pol.exploration_noise_alpha,
                              noise_scale=noise_scale, temperature=temperature,
                              evaluator=_eng.EVAL_EXTERNAL if external else _eng.EVAL_RESNET,
                              num_blocks=getattr(pol, "num_blocks", 0) if external else pol.num_blocks,
                              base_chans=getattr(pol, "base_chans", 0) if external else pol.base_chans,
                              device=(dev.index or 0) if dev.type == "cuda" else 0,
                              nodes_per_game=int(getattr(pol, "nodes_per_game", 0) or 0),   # 0: the engine's default
                              flags=flags[a], seed=((int(seed) << 8) + a) << 32)
            engines.append(eng)
            _fpu.apply(eng, _fpu.policy_fpu(pol))              # first-play urgency, per agent, if its policy carries it
            _ptemp.apply(eng, _ptemp.policy_policy_temp(pol))  # and its policy temperature
            if hasattr(pol.net, "eval"):
                pol.net.eval()
            if external:
                # (a net's forward passes run on the engine's stream: after whatever torch queued last on its device)
                register_evaluator(eng, pol.net)
            if info is not None:
                info[a] = eng.kernel_info()
            if external:
                continue
            sd = {k: v for k, v in pol.net.state_dict().items() if v.dtype == torch.float32}
            if dev.type == "cuda":
                eng.set_weights({k: (v.contiguous().data_ptr(), v.numel()) for k, v in sd.items()}, on_device=True)
            else:
                eng.set_weights({k: v.detach().cpu().numpy() for k, v in sd.items()})
        outcomes: Dict[Pair, OutcomeCounts] = defaultdict(lambda: [0, 0, 0])
        results = {}
        if pooled:
            tour = _eng.Tournament(engines)
            try:
                results = tour.play(pairs, num_rounds, tables_per_pair=tables_per_pair, moves=games is not None,
                                    collect=collect is not None, openings=openings)
            finally:
                tour.close()
        for s, (i, j) in enumerate(pairs):
            if not pooled:
                match = _eng.Match(engines[i], engines[j])
                try:
                    results[(i, j)] = match.play(num_rounds, first_game=s * num_rounds, moves=games is not None,
                                                 collect=collect is not None, openings=openings)
                finally:
                    match.close()
            res = results[(i, j)]
            st = res["stats"]
            if st["voided"]:
                raise SearchTreeFull("too many nodes")
            outcomes[(i, j)] = [int(st["wins"][0]), 0, int(st["wins"][1])]
            if games is not None:
                games[(i, j)] = {k: res[k] for k in ("outcome", "length", "moves", "opening") if k in res}
            if collect is not None:
                if pooled:                               # one queue for all pairs: pair s owns a range of uids
                    uid = results["rows"]["game_uid"]
                    mine = (uid >= s * num_rounds) & (uid < (s + 1) * num_rounds)
                    collect[(i, j)] = dict(rows={k: v[mine] for k, v in results["rows"].items()},
                                           row_metrics=results["row_metrics"][mine])
                else:
                    collect[(i, j)] = dict(rows=res["rows"], row_metrics=res["row_metrics"])
            logging.info("pair %s: outcomes %s (%.1f games/s on the device)", (i, j), outcomes[(i, j)],
                         (len(pairs) if pooled else 1) * num_rounds / max(st["seconds"], 1e-9))
        return outcomes
    finally:
        for eng in engines:
            eng.close()
