"""Player: endless stream of self-play games, read in whole games (azalea/parallel_player.py:17-76).

The reference runs one game per worker process and ships pickled frames back through pipes.
Here a Policy with the device network plays `n_games` games concurrently inside one engine
(throughput mode: device RNG, device move draw); finished games are harvested in whole, buffered
on the host and handed out by `read(size)` exactly as batch_examples does -- whole games until
`len >= size`, metrics summed over the games returned.  With torch.distributed initialised each
rank plays its share and the rows are all-gathered (azalea_amd/distributed.py).

The `pool` argument is accepted for signature compatibility (policy_trainer.py:75) and unused:
there are no worker processes.  Random movers and two-agent setups go through the host play_game
loop (one game at a time), like the reference's in-process pool (num_workers=0) -- unless a two-agent
Player is created with `device_match=True`: then each agent gets an engine of `n_games` slots, the two
play each other entirely on the device (engine.Match, agent 0 moving first in every game as in
play_game) and every game's replay rows, each from the agent that moved, are harvested on the device
and handed out by `read` like self-play's.  So do duck-typed
networks (config["network"] naming another class, policy.py:11-18) by default; with
`external_batch=True` such a net on a CUDA (ROCm) device plays `n_games` games in one engine instead,
the engine handing it the whole pool's leaf batch on the device at every evaluation point
(Engine.set_external_evaluator, policy.external_evaluator).
"""
import logging
import os
from collections import defaultdict, deque
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import distributed as azdist
from . import engine as _eng
from .game.hex import HexGameState
from .play_game import play_game
from .policy import Policy, SearchTreeFull, external_evaluator, tower_flags  # noqa: F401
from .rollout import is_rollout_net, register_evaluator
from .replay_buffer import ReplayDataFrame

Metrics = Dict[str, float]


def rows_to_frame(rows) -> ReplayDataFrame:
    """Engine rows -> the reference's struct-of-lists frame (replay_buffer.py:11-38).  The per-row
    arrays are cut out of whole-table numpy passes (one nonzero for every row's legal moves, one
    astype per table); only the GameState constructors run per row."""
    frame = ReplayDataFrame()
    P = len(rows["reward"])
    if P == 0:
        return frame
    n = rows["board"].shape[-1]
    boards = np.ascontiguousarray(rows["board"], np.int32).reshape(P, n, n)
    flat = boards.reshape(P, n * n)
    ri, ci = np.nonzero(flat == 0)                                   # row-major: ascending tiles per row
    counts = np.bincount(ri, minlength=P)
    k = np.asarray(rows["nlegal"], np.int64)
    if not np.array_equal(counts, k):
        raise AssertionError("replay rows: legal-move counts do not match the boards")
    ends = np.cumsum(counts)
    legal_all = (ci + 1).astype(np.int32)
    probs = np.ascontiguousarray(rows["moves_prob"], np.float32)
    color = np.asarray(rows["color"]).tolist()
    reward = np.asarray(rows["reward"], np.float32)
    state, mp = frame.state, frame.moves_prob
    s = 0
    for i in range(P):
        e = int(ends[i])
        state.append(HexGameState(color[i], legal_all[s:e], 0, boards[i]))
        mp.append(probs[i, :e - s])
        s = e
    frame.reward.extend(reward)       # np.float32 scalars, like play_game.py:64-65
    return frame


class Player:
    MAX_BARREN_PRODUCTIONS = 1000     # consecutive productions without a finished game before read() gives up

    MATCH_CHUNK = 2                   # device_match: games per Match.play call, in units of n_games

    def __init__(self, pool, agents: Sequence, *, n_games: int = None, gather: bool = True, role: str = None,
                 external_batch: bool = False, device_match: bool = False, random_reflect: bool = False,
                 openings=None, playout_cap=None, resign=None, early_stop=False, train_targets=None,
                 forced_playouts=None, gumbel=None, selfplay_openings=None, selfplay_opening_weights=None):
        """`gather`: under torch.distributed every rank plays its share of a read and all ranks get all rows.
        `role`: None -- every rank calls read() itself, in lock-step (symmetric); "leader" / "follower" -- the
        training-time topology (azalea_amd/distributed.py: rank 0 announces each shared production and broadcasts
        the trainer's weights first; the followers are driven by policy_trainer.serve_selfplay).
        `external_batch`: a single agent whose Policy holds a network other than HexNetwork, on a CUDA device,
        plays `n_games` games in one engine that hands the net every leaf batch of the pool on the device
        (instead of the host loop); a ValueError when that does not hold.
        `device_match`: exactly two agents, each with a Policy whose network is on a CUDA (ROCm) device, play each
        other in two engines of `n_games` slots on the device (agents[0] moves first in every game), and the games'
        replay rows are harvested there.  HexNetwork agents use the device tower; other networks need
        external_batch=True as well.  A ValueError when any of that does not hold, or under torch.distributed with
        gather=True: there is no silent fall-back to the host loop.
        `random_reflect` (NOT the reference's behaviour for Hex, whose random_reflect is the identity; off by
        default): the engines this Player builds -- device self-play, external_batch, both engines of device_match
        -- hand the network about half of all evaluation requests turned by 180 degrees
        (engine.FLAG_RANDOM_REFLECT, include/azx.h).  A ValueError when the games would run through the host loop
        instead.
        A policy attribute `tower_precision` (None / "f16x3" = the split-f16 tower as always, "f16"; opt-in and
        OUTSIDE every parity claim, policy.tower_flags) is honoured per agent by the device engines of the one-agent
        throughput mode and of device_match (engine.FLAG_TOWER_F16: the plain-f16 tower, one MFMA per product).  A
        ValueError -- here, before any engine is made -- when "f16" is asked for but the games would run through
        the host loop or an external evaluator, or the network's shape has no plain-f16 tower (the 6x64-class fused
        tower's shapes and the wide tower's -- 128 / 256 channels, up to 13x13 -- have one, given at least one block).
        `openings` (NOT in the reference, whose games all start from the empty board; off by default): an opening
        book for device_match, a list of move lists as engine.Match.set_openings takes it -- with agents[0] always
        first, game u starts from opening u % len(openings) and its rows begin at that position.  A ValueError
        -- here, before any engine is made -- in any other mode, or for a book the rules refuse.
        `playout_cap` (NOT the reference's behaviour, which searches and records every ply alike; off by default):
        (full_prob, fast_simulations) -- playout cap randomisation (Engine.set_playout_cap, include/azx.h) for the
        self-play engine this Player builds, device self-play or external_batch: every ply is with probability
        full_prob a full search that records a row and otherwise a fast search of fast_simulations, without noise,
        that records nothing.  A ValueError -- here, before any engine is made -- with device_match=True (a match
        records one row per moved ply), when the games would run through the host loop, or for values outside
        (0, 1] x [1, simulations].
        `resign` (NOT the reference's behaviour, which plays every game to the end; off by default):
        (threshold, min_ply, keep_prob), or a dict with exactly these keys -- resignation (Engine.set_resign,
        include/azx.h) for the self-play engine this Player builds, device self-play or external_batch: the mover of a
        game gives up at a ply >= min_ply whose root value is below threshold, except in the share keep_prob of the
        games that is exempt and measures the false positives (resign_stats()).  It is applied again whenever the
        engine is made again.  A ValueError -- here, before any engine is made -- with device_match=True (resign is a
        self-play option), when the games would run through the host loop, or for values outside
        [-1, 1] x [0, ...) x [0, 1].
        `early_stop` (NOT the reference's behaviour, which runs every search to its last simulation; off by default):
        True sets Engine.set_early_stop (include/azx.h has the rule) on the self-play engine this Player builds, device
        self-play or external_batch: the search of a ply drawn at temperature 0 stops once the most-visited root child
        leads by more than the selects still to come.  It is applied again whenever the engine is made again.  A
        ValueError -- here, before any engine is made -- with device_match=True (a match searches every ply in full),
        when the games would run through the host loop, or for a value that is not a bool.  Its effect on playing
        strength and training efficiency is not measured.
        `train_targets` (NOT the reference's behaviour, whose rows are one-hot from exploration_depth on and carry the
        game's outcome alone; off by default): "visits", a (policy_rows, value_mix) pair or a {"policy_rows": ...,
        "value_mix": ...} dict sets Engine.set_train_targets (include/azx.h has the definition) on the self-play engine
        this Player builds, device self-play or external_batch: the recorded rows are the root's visit shares at every
        ply, and / or the reward is (1 - value_mix) * z + value_mix * v.  The games themselves are untouched.  It is
        applied again whenever the engine is made again.  A ValueError -- here, before any engine is made -- with
        device_match=True (a match's harvest records the reference's rows and the outcome), when the games would run
        through the host loop, or for anything normalize_train_targets refuses.  DESIGN 7.12 has what is measured.
        `forced_playouts` (NOT the reference's behaviour, which selects by PUCT alone and records every visit; off by
        default): True (= (2.0, True)), a (k, prune) pair or a {"k": ..., "prune": ...} dict sets
        Engine.set_forced_playouts (include/azx.h states the rules) on the self-play engine this Player builds, device
        self-play or external_batch: a full search's root selects force sqrt(k * P * S) visits on every visited child,
        and with prune the move draw and the recorded row are made from the pruned counts.  It is applied again
        whenever the engine is made again.  A ValueError -- here, before any engine is made -- with device_match=True
        (a match searches and draws as the reference does), when the games would run through the host loop, or for
        anything normalize_forced_playouts refuses.  Its effect on playing strength and training efficiency is not
        measured.
        `gumbel` (NOT the reference's behaviour, which draws and records from PUCT visit counts under Dirichlet noise;
        off by default): True (= m 16), an int m, an (m, c_visit, c_scale) triple or a dict with those keys plus
        "improved_rows" sets Engine.set_gumbel (include/azx.h has the definition) on the self-play engine this Player
        builds, device self-play or external_batch: a Gumbel root search with sequential halving at every ply, the
        final survivor played, the recorded row the policy improved by the completed Q-values -- a search whose move
        and row are sound at 32-100 simulations.  The defaults c_visit = 50 and c_scale = 1.0 are the author's
        recollection of the paper's board-game values and are not checked here.  It is applied again whenever the
        engine is made again.  A ValueError -- here, before any engine is made -- with device_match=True (a match
        searches and draws as the reference does), when the games would run through the host loop, together with
        forced_playouts or early_stop (rules about PUCT visit leaders), or for anything normalize_gumbel refuses.  Its
        effect on playing strength and training efficiency is NOT measured.
        `selfplay_openings` (NOT the reference's behaviour, whose games all start from the empty board; off by default):
        a weighted opening book for SELF-PLAY -- a list of move lists, or any form normalize_selfplay_openings takes,
        with `selfplay_opening_weights` (None: uniform) -- sets Engine.set_selfplay_openings (include/azx.h has the
        definition) on the self-play engine this Player builds, device self-play or external_batch, right after the
        engine is created and before any play: every game the engine starts begins from the opening its uid draws, on
        the device.  It is applied again whenever the engine is made again.  (`openings` keeps its meaning: the book of
        a device match.)  A ValueError -- here, before any engine is made -- with device_match=True (a match has its
        own book: use openings=), with two agents, when the games would run through the host loop, or for anything
        normalize_selfplay_openings or the rules refuse.  opening_stats() has the per-opening tallies.  Its effect on
        playing strength and training efficiency is NOT measured."""
        if role not in (None, "leader", "follower"):
            raise ValueError("Player role must be None, 'leader' or 'follower'")
        self.openings = [[int(m) for m in o] for o in ([] if openings is None else openings)]
        if self.openings and not device_match:
            raise ValueError("openings are a device_match option: only the device match starts its games from an "
                             "opening book (self-play and the host loop start from the empty board)")
        self.agents = agents
        self.running = True
        self.gather = gather
        self.external_batch = bool(external_batch)
        self.device_match = bool(device_match)
        if self.device_match:
            self._match_policies()
            if self.openings:
                _eng.openings_check(self.agents[0].game.board_size, self.openings)
        elif self.external_batch:
            self._external_policy()
        self.random_reflect = bool(random_reflect)
        if self.random_reflect and not (self.device_match or self.external_batch) and self._device_policy() is None:
            raise ValueError("random_reflect needs the games to run in a device engine (a single agent whose Policy "
                             "holds a HexNetwork, external_batch=True or device_match=True): these agents play "
                             "through the host loop, which does not reflect")
        self._engine_flags = _eng.FLAG_RANDOM_REFLECT if self.random_reflect else 0
        self._check_tower_precision()
        self.playout_cap = self._check_playout_cap(playout_cap)
        self.resign = self._check_resign(resign)
        self.early_stop = self._check_early_stop(early_stop)
        self.train_targets = self._check_train_targets(train_targets)
        self.forced_playouts = self._check_forced_playouts(forced_playouts)
        self.gumbel = self._check_gumbel(gumbel)
        self.selfplay_openings = self._check_selfplay_openings(selfplay_openings, selfplay_opening_weights)
        self._match = None             # device_match: (engine a, engine b, engine.Match)
        self._match_next = 0           # ... the first game index of the next chunk: no game index repeats
        self.role = role if (gather and azdist.is_distributed()) else None
        self.learner = None            # actor_learner.Learner: read() pulls the actors' backlogs instead of playing
        self.weight_syncs = 0          # broadcasts of the trainer's weights this player took part in
        self.n_games = n_games or int(os.environ.get("AZX_GAMES", "4096"))
        self._games = deque()          # finished games waiting to be read: (rows dict, metrics)
        self._engine = None
        self._engine_key = None
        self._seed_base = None
        self._skipped = 0              # games dropped because of SearchTreeFull since the last read

    # ---- reference surface -------------------------------------------------------------------
    def read(self, size) -> Tuple[ReplayDataFrame, Metrics]:
        """Whole games until at least `size` positions (parallel_player.py:41-52).  A game that
        overflowed its tree (SearchTreeFull) is skipped like the reference's worker does
        (parallel_player.py:73-76) and counted in metrics['game_error']."""
        if self.learner is not None:
            return self._read_pulled(size)
        shared = self.gather and azdist.is_distributed()
        self.announce(azdist.OP_READ, int(np.ceil(size)))
        self._agree_seed_base()       # a collective when shared: every rank passes here, whatever its quota
        quota = azdist.shard_quota(size) if shared else size
        rows_list, metrics = [], defaultdict(float)
        have, barren = 0, 0
        failure = None
        try:
            while have < quota:
                if not self._games:
                    self._produce(quota - have)
                    if not self._games:
                        barren += 1
                        if barren > self.MAX_BARREN_PRODUCTIONS:
                            raise RuntimeError("self-play produced no finished game in %d attempts" % barren)
                        continue
                rows, gm = self._games.popleft()
                rows_list.append(rows)
                have += len(rows["reward"])
                for name, v in gm.items():
                    metrics[name] += v
        except Exception as exc:
            if not shared:
                raise
            # the other ranks are on their way into this read's record collectives: join the first one with the
            # failure mark so that every rank leaves it (distributed.PeerFailed), then raise what happened here
            failure = exc
            rows_list = []
        if self._skipped:
            metrics["game_error"] += self._skipped
            self._skipped = 0
        n = self.agents[0].game.board_size
        if rows_list:
            rows = {k: np.concatenate([r[k] for r in rows_list]) for k in rows_list[0]}
        else:
            rows = azdist.empty_rows(n)       # quota 0 (size < world): still join the collectives
        if shared:
            try:
                rows = azdist.all_gather_rows(rows, n, failed=failure is not None)
            except azdist.PeerFailed:
                if failure is not None:
                    raise failure
                raise
            metrics = azdist.all_reduce_metrics(dict(metrics))
        return rows_to_frame(rows), dict(metrics)

    def _read_pulled(self, size) -> Tuple[ReplayDataFrame, Metrics]:
        """read() of the learner in actor / learner mode (azalea_amd/actor_learner.py): whole games out of the other
        ranks' backlogs, as a host frame; metrics in play_game's keys, summed over the games returned."""
        n = self.agents[0].game.board_size
        dev = azdist._comm_device()
        parts, counts, st = self.learner.pull(size, dev, azdist.record_bytes(n * n))
        rec = torch.cat(parts).cpu().numpy() if sum(counts) else np.zeros((0, azdist.record_bytes(n * n)), np.uint8)
        rows = azdist.unpack_rows(rec, n)
        metrics = {"games": st.get("games", 0.0), "reward": st.get("sum_reward_last", 0.0),
                   "moves_per_game": float(len(rows["reward"])), "seconds_per_game": st.get("seconds", 0.0),
                   "game_error": st.get("game_errors", 0.0)}
        metrics.update({k[5:]: v for k, v in st.items() if k.startswith("game_") and k != "game_errors"})
        return rows_to_frame(rows), metrics

    def announce(self, op: int, arg: int) -> None:
        """Leader / follower topology only: rank 0 says what all ranks produce next, then its network --
        the trainer's live weights and BatchNorm statistics -- is broadcast, so every rank searches with what
        the trainer holds right now (parallel_player.py:36-38).  Collectives: called by every rank, in the
        same place (the leader from read() / DeviceReplayBuffer.consume, the followers from serve_selfplay
        through the same two methods)."""
        if self.role is None:
            return
        if self.role == "leader":
            azdist.lead(op, arg)
        pol = self._device_policy()
        if pol is not None:
            azdist.broadcast_weights(pol.net, src=0)
            # in-place copies into the parameters do move their version counters, graph replays do not:
            pol.net.weight_updates_outside_autograd = getattr(pol.net, "weight_updates_outside_autograd", 0) + 1
            self.weight_syncs += 1

    def stop(self) -> None:
        self.running = False
        self._games.clear()
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        self._close_match()

    # ---- device-resident replay (azalea_amd/device_replay.py) ---------------------------------
    def device_engine(self):
        """The engine self-play runs in (created on first use); DeviceReplayBuffer keeps its ring there."""
        pol = self._device_policy()
        if pol is None:
            raise RuntimeError("device-resident replay needs a single agent whose Policy holds a HexNetwork")
        self._agree_seed_base()
        return self._get_engine(pol)

    def prepare_device_engine(self, engine) -> None:
        """Refresh the engine's packed weights from the trainer's live module (SURVEY 8(b) ownership)."""
        pol = self._device_policy()
        if pol is not None and engine is self._engine:
            self._push_weights(engine, pol)

    # ---- production --------------------------------------------------------------------------
    def _device_policy(self):
        pol = getattr(self.agents[0], "policy", None)
        return pol if isinstance(pol, Policy) and pol._uses_device_net() and len(self.agents) == 1 else None

    def _check_tower_precision(self) -> None:
        """Every agent's `tower_precision` is one this Player's engines can honour (policy.tower_flags, which refuses
        policies without a HexNetwork itself); no GPU needed."""
        on_device = self.device_match or self._device_policy() is not None
        for i, agent in enumerate(self.agents):
            pol = getattr(agent, "policy", None)
            if pol is not None and tower_flags(pol) and not on_device:
                raise ValueError("agent %d asks for tower_precision='f16', but these games run through the host loop, "
                                 "which does not launch the device tower" % i)

    def _check_playout_cap(self, cap):
        """`playout_cap` as (full_prob, fast_simulations), or None; a ValueError naming what does not hold."""
        if cap is None:
            return None
        full_prob, fast = normalize_playout_cap(cap)
        if self.device_match:
            raise ValueError("playout_cap is a self-play option: a device match records one row per moved ply "
                             "(engine.Match refuses an engine with a cap)")
        pol = self._external_policy() if self.external_batch else self._device_policy()
        if pol is None:
            raise ValueError("playout_cap needs the games to run in a device engine (a single agent whose Policy "
                             "holds a HexNetwork, or external_batch=True): these agents play through the host loop, "
                             "which searches every ply in full")
        if fast > pol.simulations:
            raise ValueError("playout_cap: fast_simulations %d above the policy's simulations %d" % (fast, pol.simulations))
        return full_prob, fast

    def _check_resign(self, resign):
        """`resign` as (threshold, min_ply, keep_prob), or None; a ValueError naming what does not hold."""
        if resign is None:
            return None
        resign = normalize_resign(resign)
        if self.device_match:
            raise ValueError("resign is a self-play option: a device match plays every game to the end "
                             "(engine.Match refuses an engine with resignation set)")
        pol = self._external_policy() if self.external_batch else self._device_policy()
        if pol is None:
            raise ValueError("resign needs the games to run in a device engine (a single agent whose Policy holds a "
                             "HexNetwork, or external_batch=True): these agents play through the host loop, which "
                             "plays every game to the end")
        return resign

    def _check_early_stop(self, early_stop):
        """`early_stop` as a bool; a ValueError naming what does not hold."""
        early_stop = normalize_early_stop(early_stop)
        if not early_stop:
            return False
        if self.device_match:
            raise ValueError("early_stop is a self-play option: a device match searches every ply in full "
                             "(engine.Match refuses an engine with early stop set)")
        pol = self._external_policy() if self.external_batch else self._device_policy()
        if pol is None:
            raise ValueError("early_stop needs the games to run in a device engine (a single agent whose Policy holds "
                             "a HexNetwork, or external_batch=True): these agents play through the host loop, which "
                             "runs every search to its last simulation")
        return True

    def _check_train_targets(self, train_targets):
        """`train_targets` as a (policy_rows, value_mix) pair, or None for off; a ValueError naming what does not hold."""
        train_targets = normalize_train_targets(train_targets)
        if train_targets is None:
            return None
        if self.device_match:
            raise ValueError("train_targets is a self-play option: a device match's harvest records the reference's "
                             "rows and the outcome (engine.Match refuses an engine with training targets set)")
        pol = self._external_policy() if self.external_batch else self._device_policy()
        if pol is None:
            raise ValueError("train_targets needs the games to run in a device engine (a single agent whose Policy "
                             "holds a HexNetwork, or external_batch=True): these agents play through the host loop, "
                             "which records the reference's rows and the outcome")
        return train_targets

    def _check_forced_playouts(self, forced_playouts):
        """`forced_playouts` as a (k, prune) pair, or None for off; a ValueError naming what does not hold."""
        forced_playouts = normalize_forced_playouts(forced_playouts)
        if forced_playouts is None:
            return None
        if self.device_match:
            raise ValueError("forced_playouts is a self-play option: a device match searches and draws every ply as "
                             "the reference does (engine.Match refuses an engine with forced playouts set)")
        pol = self._external_policy() if self.external_batch else self._device_policy()
        if pol is None:
            raise ValueError("forced_playouts needs the games to run in a device engine (a single agent whose Policy "
                             "holds a HexNetwork, or external_batch=True): these agents play through the host loop, "
                             "which selects by PUCT alone and records every visit")
        return forced_playouts

    def _check_gumbel(self, gumbel):
        """`gumbel` as an (m, c_visit, c_scale, improved_rows) tuple, or None for off; a ValueError naming what does not
        hold."""
        gumbel = normalize_gumbel(gumbel)
        if gumbel is None:
            return None
        if self.device_match:
            raise ValueError("gumbel is a self-play option: a device match searches and draws every ply as the "
                             "reference does (engine.Match refuses an engine with the Gumbel root search set)")
        if self.forced_playouts is not None or self.early_stop:
            raise ValueError("gumbel cannot be set together with %s: that option is a rule about PUCT visit leaders, "
                             "which a Gumbel root search does not play"
                             % ("forced_playouts" if self.forced_playouts is not None else "early_stop"))
        pol = self._external_policy() if self.external_batch else self._device_policy()
        if pol is None:
            raise ValueError("gumbel needs the games to run in a device engine (a single agent whose Policy holds a "
                             "HexNetwork, or external_batch=True): these agents play through the host loop, which "
                             "selects by PUCT and draws from the visit counts")
        return gumbel

    def _check_selfplay_openings(self, openings, weights):
        """`selfplay_openings` as a (book, weights or None) pair, or None for off; a ValueError naming what does not
        hold."""
        if openings is None:
            if weights is not None:
                raise ValueError("selfplay_opening_weights given without selfplay_openings")
            return None
        if self.device_match:
            raise ValueError("selfplay_openings is a self-play option: a device match starts its games from its own "
                             "book (use openings=; engine.Match refuses an engine with a self-play book)")
        if len(self.agents) != 1:
            raise ValueError("selfplay_openings is a self-play option: it needs a single agent, got %d (two agents play "
                             "through the host loop or, with device_match=True, a device match)" % len(self.agents))
        pol = self._external_policy() if self.external_batch else self._device_policy()
        if pol is None:
            raise ValueError("selfplay_openings needs the games to run in a device engine (a single agent whose Policy "
                             "holds a HexNetwork, or external_batch=True): these agents play through the host loop, "
                             "which starts every game from the empty board")
        n = self.agents[0].game.board_size
        book, w = normalize_selfplay_openings(openings, n)
        if weights is not None:
            if w is not None:
                raise ValueError("selfplay_openings: weights given twice (in the book's dict and as selfplay_opening_weights)")
            book, w = normalize_selfplay_openings({"book": book, "weights": weights}, n)
        _eng.openings_check(n, book)
        return book, w

    def opening_stats(self):
        """Engine.selfplay_openings_stats() of the self-play engine, or None while there is none or selfplay_openings
        is not set."""
        if self.selfplay_openings is None or self._engine is None:
            return None
        return self._engine.selfplay_openings_stats()

    def gumbel_stats(self):
        """Engine.gumbel_stats() of the self-play engine, or None while there is none or gumbel is not set."""
        if self.gumbel is None or self._engine is None:
            return None
        return self._engine.gumbel_stats()

    def forced_playouts_stats(self):
        """Engine.forced_playouts_stats() of the self-play engine, or None while there is none or forced_playouts is
        not set."""
        if self.forced_playouts is None or self._engine is None:
            return None
        return self._engine.forced_playouts_stats()

    def train_targets_stats(self):
        """Engine.train_targets_stats() of the self-play engine, or None while there is none or train_targets is not set."""
        if self.train_targets is None or self._engine is None:
            return None
        return self._engine.train_targets_stats()

    def early_stop_stats(self):
        """Engine.early_stop_stats() of the self-play engine, or None while there is none or early_stop is not set."""
        if not self.early_stop or self._engine is None:
            return None
        return self._engine.early_stop_stats()

    def resign_stats(self):
        """Engine.resign_stats() of the self-play engine, or None while there is none or resign is not set."""
        if self.resign is None or self._engine is None:
            return None
        return self._engine.resign_stats()

    def _external_policy(self) -> Policy:
        """The Policy whose duck-typed net evaluates the pool's leaf batches (external_batch=True); a ValueError
        naming what does not hold otherwise -- there is no silent fall-back to the host loop."""
        if len(self.agents) != 1:
            raise ValueError("external_batch needs a single agent (self-play), got %d" % len(self.agents))
        pol = getattr(self.agents[0], "policy", None)
        if not isinstance(pol, Policy):
            raise ValueError("external_batch needs an agent whose policy is an azalea_amd Policy")
        if pol._uses_device_net():
            raise ValueError("external_batch is for networks other than HexNetwork: a HexNetwork takes the "
                             "native device path without it")
        dev = _net_device(pol.net)
        if dev.type != "cuda" and not is_rollout_net(pol.net):      # (a RolloutNet's evaluator is a kernel of the engine)
            raise ValueError("external_batch needs the network on a CUDA (ROCm) device, it is on %s" % dev)
        if self.gather and azdist.is_distributed():
            raise ValueError("external_batch does not share reads across ranks: pass gather=False under "
                             "torch.distributed")
        return pol

    def _match_policies(self):
        """The two agents' Policies of a device_match Player; a ValueError naming what does not hold otherwise."""
        from .evaluation import _throughput_policy
        if len(self.agents) != 2:
            raise ValueError("device_match needs exactly two agents, got %d" % len(self.agents))
        pols = []
        for i, agent in enumerate(self.agents):
            try:
                pol = _throughput_policy(agent, self.external_batch)
            except TypeError as exc:
                raise ValueError("device_match: agent %d: %s" % (i, str(exc).replace("evaluate_throughput", "it"))) from exc
            pols.append(pol)
        for i, pol in enumerate(pols):
            dev = _net_device(pol.net)
            if dev.type != "cuda" and not is_rollout_net(pol.net):
                raise ValueError("device_match needs every network on a CUDA (ROCm) device, agent %d's is on %s" % (i, dev))
        if self.gather and azdist.is_distributed():
            raise ValueError("device_match does not share reads across ranks: pass gather=False under "
                             "torch.distributed")
        return pols

    def _engine_policy(self):
        """The Policy whose searches run in this Player's engine (None: the host loop plays)."""
        if self.device_match:
            return self._match_policies()[0]      # (its rng seeds both engines' streams)
        return self._external_policy() if self.external_batch else self._device_policy()

    def _agree_seed_base(self) -> None:
        """Each game draws from its own stream: seed base + GLOBAL game index.  Ranks that share
        their reads use rank 0's base (rank r of W plays the games r, r+W, ...: the set of games does not depend
        on W).  The broadcast is a collective, so it happens where every rank is guaranteed to arrive -- at the
        top of read() / device_engine() -- never inside the production path, which a rank with quota 0 or with
        games still queued skips.  A Player that does not gather derives its base locally."""
        if self._seed_base is not None:
            return
        pol = self._engine_policy()
        if pol is None:
            return
        local = int(pol.rng.randint(0, 2 ** 31 - 1))
        if self.gather and azdist.is_distributed():
            self._seed_base = azdist.broadcast_int(local)
        else:
            # no shared index space: the engine counts its own games 0, 1, ... (stride 1, offset 0 in _get_engine);
            # ranks whose policies were seeded alike must still not replay each other's games
            self._seed_base = (local ^ (azdist.rank() * 0x9E3779B1)) & 0x7FFFFFFF

    def _produce(self, want: int) -> None:
        if self.device_match:
            self._produce_match(self._match_policies())
            return
        if self.external_batch:
            self._produce_external(self._external_policy(), want)
            return
        pol = self._device_policy()
        if pol is None:
            self._produce_on_host()
        else:
            self._produce_on_device(pol, want)

    def _produce_on_host(self) -> None:
        """One game through the generic loop (random mover / duck-typed nets / two agents)."""
        for a in self.agents:
            net = getattr(getattr(a, "policy", None), "_net", None)
            if hasattr(net, "eval"):
                net.eval()
        try:
            _, frame, gm = play_game(self.agents, collect_data=True)
        except SearchTreeFull:
            logging.warning("game failed because of SearchTreeFull (skipped)")
            self._skipped += 1
            return
        n = self.agents[0].game.board_size
        P = len(frame)
        rows = dict(board=np.stack([s.board for s in frame.state]).astype(np.int32),
                    color=np.array([s.color for s in frame.state], np.int32),
                    nlegal=np.array([len(s.legal_moves) for s in frame.state], np.int32),
                    moves_prob=np.zeros((P, n * n), np.float32),
                    reward=np.array(frame.reward, np.float32),
                    game_uid=np.full(P, -1, np.int64))
        for i, p in enumerate(frame.moves_prob):
            rows["moves_prob"][i, :len(p)] = p
        self._games.append((rows, dict(gm)))

    def _get_engine(self, pol: Policy, external: bool = False):
        n = self.agents[0].game.board_size
        rank, world = ((torch.distributed.get_rank(), torch.distributed.get_world_size())
                       if (self.gather and azdist.is_distributed()) else (0, 1))
        net_dev = _net_device(pol.net)
        device = (net_dev.index or 0) if net_dev.type == "cuda" else 0
        key = (n, device, pol.simulations, pol.search_batch_size, float(pol.exploration_coef),
               pol.exploration_depth, pol.exploration_noise_alpha, pol.exploration_noise_scale,
               pol.exploration_temperature, pol.num_blocks, pol.base_chans,
               bool(pol.settings.get("move_sampling")), bool(pol.settings.get("move_exploration")), external, tower_flags(pol))
        if self._engine is None or key != self._engine_key:
            if self._engine is not None:
                self._engine.close()
            sampling = pol.settings.get("move_sampling", False)
            explore = sampling and pol.settings.get("move_exploration", False)
            if self._seed_base is None:      # read() / device_engine() agree on it before any production
                raise RuntimeError("Player: the seed base must be agreed before the engine is created")
            self._engine = _eng.Engine(
                board_size=n, n_games=self.n_games, simulations=pol.simulations,
                search_batch_size=pol.search_batch_size, exploration_coef=pol.exploration_coef,
                exploration_depth=pol.exploration_depth if sampling else 0,
                noise_alpha=pol.exploration_noise_alpha,
                noise_scale=pol.exploration_noise_scale if explore else 0.0,
                temperature=pol.exploration_temperature if sampling else 0.0,
                evaluator=_eng.EVAL_EXTERNAL if external else _eng.EVAL_RESNET,
                num_blocks=pol.num_blocks, base_chans=pol.base_chans,
                flags=self._engine_flags | tower_flags(pol),
                device=device, seed=self._seed_base, game_index_stride=world, game_index_offset=rank)
            if self.selfplay_openings is not None:      # before any play: generation 0 follows the book too
                self._engine.set_selfplay_openings(*self.selfplay_openings)
            if self.playout_cap is not None:
                self._engine.set_playout_cap(*self.playout_cap)
            if self.resign is not None:
                self._engine.set_resign(*self.resign)
            if self.early_stop:
                self._engine.set_early_stop(True)
            if self.train_targets is not None:
                self._engine.set_train_targets(*self.train_targets)
            if self.forced_playouts is not None:
                self._engine.set_forced_playouts(*self.forced_playouts)
            if self.gumbel is not None:
                self._engine.set_gumbel(*self.gumbel)
            self._engine_key = key
        return self._engine

    def _produce_on_device(self, pol: Policy, want: int) -> None:
        eng = self._get_engine(pol)
        self._push_weights(eng, pol)
        rows, st = eng.play(max(1, int(want)))
        self._harvest(eng, rows, st)

    def _produce_external(self, pol: Policy, want: int) -> None:
        """_produce_on_device with the policy's own (duck-typed) net as the evaluator of the whole pool."""
        eng = self._get_engine(pol, external=True)
        net = pol.net
        if hasattr(net, "eval"):
            net.eval()                          # parallel_player.py:64-69
        # a net's forward passes run on the engine's stream: after whatever torch queued last (the trainer's step);
        # a RolloutNet gets the rollout kernel instead
        register_evaluator(eng, net)
        rows, st = eng.play(max(1, int(want)))
        self._harvest(eng, rows, st)

    def _close_match(self) -> None:
        if self._match is not None:
            a, b, match = self._match
            if match is not None:
                match.close()
            a.close()
            b.close()
            self._match = None

    def _match_engine(self, pol: Policy, which: int):
        """Agent `which`'s engine, configured as evaluation.evaluate_throughput configures a pair's engines."""
        n = self.agents[0].game.board_size
        temperature = noise_scale = 0.0            # Policy.choose_action's schedule (policy.py:132-149)
        if pol.settings["move_sampling"]:
            temperature = pol.exploration_temperature
            if pol.settings["move_exploration"]:
                noise_scale = pol.exploration_noise_scale
        external = not pol._uses_device_net()
        dev = _net_device(pol.net)
        # game_rng keys on seed + uid: the two agents' streams are disjoint ranges of 2^32 games
        return _eng.Engine(board_size=n, n_games=self.n_games, simulations=pol.simulations,
                           search_batch_size=pol.search_batch_size, exploration_coef=pol.exploration_coef,
                           exploration_depth=pol.exploration_depth, noise_alpha=pol.exploration_noise_alpha,
                           noise_scale=noise_scale, temperature=temperature,
                           evaluator=_eng.EVAL_EXTERNAL if external else _eng.EVAL_RESNET,
                           num_blocks=getattr(pol, "num_blocks", 0) if external else pol.num_blocks,
                           base_chans=getattr(pol, "base_chans", 0) if external else pol.base_chans,
                           device=(dev.index or 0) if dev.type == "cuda" else 0, nodes_per_game=int(getattr(pol, "nodes_per_game", 0) or 0),
                           flags=self._engine_flags | tower_flags(pol),
                           seed=(2 * (int(self._seed_base) & 0x3FFFFFFF) + which) << 32)

    def _produce_match(self, pols) -> None:
        """One chunk of MATCH_CHUNK * n_games games between the two agents' engines, harvested on the device."""
        if self._seed_base is None:
            raise RuntimeError("Player: the seed base must be agreed before the engines are created")
        if self._match is None:
            a = self._match_engine(pols[0], 0)
            try:
                b = self._match_engine(pols[1], 1)
            except Exception:
                a.close()
                raise
            self._match = (a, b, None)
        a, b, match = self._match
        for eng, pol in ((a, pols[0]), (b, pols[1])):         # the live weights, before every chunk
            net = pol.net
            if hasattr(net, "eval"):
                net.eval()
            if pol._uses_device_net():
                self._push_weights(eng, pol)
            else:
                register_evaluator(eng, net)
        if match is None:                                     # (a match wants its engines ready: weights / evaluator)
            match = _eng.Match(a, b)
            if self.openings:
                match.set_openings(self.openings)
            self._match = (a, b, match)
        chunk = self.MATCH_CHUNK * self.n_games
        res = match.play(chunk, first_game=self._match_next, collect=True, first_mover=0)
        self._match_next += chunk
        st = res["stats"]
        self._harvest(a, res["rows"], dict(game_errors=st["voided"], seconds=st["seconds"],
                                           games=st["games"] - st["voided"]), meta=res["row_metrics"])

    def _harvest(self, eng, rows, st, meta=None) -> None:
        """Whole games of one engine play call -> the read queue, with play_game's per-game metrics."""
        uid = rows["game_uid"]
        self._skipped += int(st["game_errors"])
        if len(uid) == 0:
            return
        # play_game's per-game metrics are means over the game's own plies (play_game.py:73-76)
        if meta is None:
            meta = eng.play_row_metrics()
        starts = np.flatnonzero(np.r_[True, uid[1:] != uid[:-1]])
        ends = np.r_[starts[1:], len(uid)]
        names = [k for k, _ in eng.ROW_METRIC_COLUMNS]
        cols = [c for _, c in eng.ROW_METRIC_COLUMNS]
        for s, e in zip(starts, ends):
            game = {k: v[s:e] for k, v in rows.items()}
            mean = meta[s:e][:, cols].astype(np.float64).mean(0)
            # the key set of play_game.py:69-76 over search_tree.py:109-112 / mcts.py:291 / policy.py:164
            gm = dict(games=1, reward=float(game["reward"][-1]), moves_per_game=int(e - s),
                      seconds_per_game=st["seconds"] / max(1, st["games"]), game_error=0)
            gm.update(zip(names, (float(x) for x in mean)))
            self._games.append((game, gm))

    @staticmethod
    def _push_weights(eng, pol: Policy) -> None:
        net = pol.net
        sd = {k: v for k, v in net.state_dict().items() if v.dtype == torch.float32}
        if net.device.type == "cuda":
            eng.set_weights({k: (v.contiguous().data_ptr(), v.numel()) for k, v in sd.items()}, on_device=True)
        else:
            eng.set_weights({k: v.detach().cpu().numpy() for k, v in sd.items()})


def normalize_playout_cap(cap):
    """(full_prob, fast_simulations) of a pair or of a {"full_prob": ..., "fast_simulations": ...} mapping; a
    ValueError unless full_prob is in (0, 1] and fast_simulations a whole number >= 1."""
    try:
        if isinstance(cap, dict):
            if set(cap) != {"full_prob", "fast_simulations"}:
                raise ValueError
            full_prob, fast = cap["full_prob"], cap["fast_simulations"]
        else:
            full_prob, fast = cap
        full_prob = float(full_prob)
        if isinstance(fast, bool) or int(fast) != fast:
            raise ValueError
        fast = int(fast)
    except (TypeError, ValueError, KeyError):
        raise ValueError("playout_cap must be (full_prob, fast_simulations) or a dict with exactly these two keys, "
                         "got %r" % (cap,)) from None
    if not 0.0 < full_prob <= 1.0:
        raise ValueError("playout_cap: full_prob %r outside (0, 1]" % full_prob)
    if fast < 1:
        raise ValueError("playout_cap: fast_simulations %d below 1" % fast)
    return full_prob, fast


def normalize_selfplay_openings(spec, board_size=None):
    """(book, weights) of a self-play opening book -- book a list of move lists (tile + 1 in play order), weights a list
    of floats or None for uniform -- or None for None.  Accepted: a list of move lists; {"book": [...]} with an optional
    "weights": [...]; {"all": 1 | 2} for engine.all_openings(board_size, plies) (needs `board_size`); and in a dict an
    optional "empty_share": s in [0, 1], which puts the empty opening first with weight s and gives the others 1 - s in
    equal parts (not together with "weights").  A ValueError for anything else: unknown keys, both or neither of "book"
    and "all", an empty book, moves that are not whole numbers, weights of another length, or negative, non-finite or
    all zero.  The rules themselves (moves on the board, no tile twice, undecided) are engine.openings_check's."""
    if spec is None:
        return None
    what = "selfplay_openings"
    weights, share = None, None
    if isinstance(spec, dict):
        extra = set(spec) - {"book", "weights", "all", "empty_share"}
        if extra:
            raise ValueError("%s as a dict takes the keys 'book', 'weights', 'all' and 'empty_share', got %r"
                             % (what, sorted(map(str, spec))))
        if ("book" in spec) == ("all" in spec):
            raise ValueError("%s as a dict needs exactly one of 'book' and 'all'" % what)
        if "all" in spec:
            plies = spec["all"]
            if isinstance(plies, bool) or plies not in (1, 2):
                raise ValueError("%s: 'all' must be 1 or 2 (plies), got %r" % (what, plies))
            if board_size is None:
                raise ValueError("%s: 'all' needs the board size" % what)
            book = _eng.all_openings(int(board_size), int(plies))
        else:
            book = spec["book"]
        weights, share = spec.get("weights"), spec.get("empty_share")
    else:
        book = spec
    try:
        if isinstance(book, (str, bytes, dict)):
            raise TypeError
        book = [list(o) for o in book]
        for o in book:
            for m in o:
                if isinstance(m, bool) or int(m) != m:
                    raise ValueError
        book = [[int(m) for m in o] for o in book]
    except (TypeError, ValueError):
        raise ValueError("%s: the book must be a list of move lists (whole numbers, tile + 1 in play order), got %r"
                         % (what, spec)) from None
    if not book:
        raise ValueError("%s: the book is empty (leave the option out to play from the empty board)" % what)
    if share is not None:
        if weights is not None:
            raise ValueError("%s: 'empty_share' and 'weights' cannot be given together" % what)
        if isinstance(share, bool) or not isinstance(share, (int, float, np.integer, np.floating)) \
                or not 0.0 <= float(share) <= 1.0:
            raise ValueError("%s: empty_share must be a number in [0, 1], got %r" % (what, share))
        share = float(share)
        weights = [share] + [(1.0 - share) / len(book)] * len(book)
        book = [[]] + book
    if weights is not None:
        try:
            if isinstance(weights, (str, bytes, dict)):
                raise TypeError
            weights = [float(w) for w in weights]
        except (TypeError, ValueError):
            raise ValueError("%s: weights must be a list of numbers, got %r" % (what, weights)) from None
        if len(weights) != len(book):
            raise ValueError("%s: %d weights for %d openings" % (what, len(weights), len(book)))
        if any(not np.isfinite(w) or w < 0.0 for w in weights):
            raise ValueError("%s: weights must be finite and >= 0, got %r" % (what, weights))
        if not sum(weights) > 0.0:
            raise ValueError("%s: the weights are all zero" % what)
    return book, weights


def normalize_train_targets(train_targets):
    """(policy_rows, value_mix) of "visits" (= ("visits", 0.0)), of a pair or of a {"policy_rows": ..., "value_mix": ...}
    mapping; None for None / False and for the pair that is "off", ("reference", 0.0).  A ValueError unless policy_rows
    is "reference" or "visits" and value_mix a number in [0, 1]."""
    if train_targets is None or train_targets is False:
        return None
    if isinstance(train_targets, str):
        if train_targets != "visits":
            raise ValueError("train_targets must be 'visits', a (policy_rows, value_mix) pair or a dict with those "
                             "keys, got %r" % (train_targets,))
        return "visits", 0.0
    if isinstance(train_targets, dict):
        if set(train_targets) != {"policy_rows", "value_mix"}:
            raise ValueError("train_targets as a dict needs exactly the keys 'policy_rows' and 'value_mix', got %r"
                             % (sorted(map(str, train_targets)),))
        rows, mix = train_targets["policy_rows"], train_targets["value_mix"]
    elif isinstance(train_targets, (tuple, list)) and len(train_targets) == 2:
        rows, mix = train_targets
    else:
        raise ValueError("train_targets must be 'visits', a (policy_rows, value_mix) pair or a dict with those keys, "
                         "got %r" % (train_targets,))
    if rows not in ("reference", "visits"):
        raise ValueError("train_targets: policy_rows must be 'reference' or 'visits', got %r" % (rows,))
    if isinstance(mix, (bool, np.bool_)) or not isinstance(mix, (int, float, np.integer, np.floating)):
        raise ValueError("train_targets: value_mix must be a number in [0, 1], got %r" % (mix,))
    mix = float(mix)
    if not 0.0 <= mix <= 1.0:                  # (NaN fails both comparisons)
        raise ValueError("train_targets: value_mix must be in [0, 1], got %r" % (mix,))
    if rows == "reference" and mix == 0.0:
        return None
    return rows, mix


def normalize_forced_playouts(forced_playouts):
    """(k, prune) of True (= (2.0, True)), a pair or a {"k": ..., "prune": ...} mapping, or None for off (None, False,
    (0, False)); a ValueError unless k is a number in [0, 64], prune a bool, and k > 0 where prune is set."""
    if forced_playouts is None or forced_playouts is False:
        return None
    if forced_playouts is True:
        return 2.0, True
    if isinstance(forced_playouts, dict):
        if set(forced_playouts) != {"k", "prune"}:
            raise ValueError("forced_playouts as a dict needs exactly the keys 'k' and 'prune', got %r"
                             % (sorted(map(str, forced_playouts)),))
        k, prune = forced_playouts["k"], forced_playouts["prune"]
    elif isinstance(forced_playouts, (tuple, list)) and len(forced_playouts) == 2:
        k, prune = forced_playouts
    else:
        raise ValueError("forced_playouts must be True, a (k, prune) pair or a dict with those keys, got %r"
                         % (forced_playouts,))
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, float, np.integer, np.floating)):
        raise ValueError("forced_playouts: k must be a number in [0, 64], got %r" % (k,))
    k = float(k)
    if not 0.0 <= k <= 64.0:                        # NaN fails both comparisons
        raise ValueError("forced_playouts: k must be in [0, 64], got %r" % (k,))
    if not isinstance(prune, (bool, np.bool_)):
        raise ValueError("forced_playouts: prune must be True or False, got %r" % (prune,))
    if k == 0.0:
        if prune:
            raise ValueError("forced_playouts: pruning needs forcing (k > 0), got k = 0 with prune = True")
        return None
    return k, bool(prune)


GUMBEL_DEFAULT = (16, 50.0, 1.0, True)


def normalize_gumbel(gumbel):
    """(m, c_visit, c_scale, improved_rows) of True (= (16, 50.0, 1.0, True)), an int m, an (m, c_visit, c_scale)
    triple or a mapping with the keys "m", "c_visit", "c_scale", "improved_rows" (any subset: the rest default), or None
    for off (None, False, m = 0); a ValueError unless m is an int in [2, 64], c_visit a number in [0, 1e4], c_scale a
    number in (0, 100] and improved_rows a bool.  The defaults 50 and 1.0 are the author's recollection of the paper's
    board-game values and are not checked here."""
    if gumbel is None or gumbel is False:
        return None
    m, c_visit, c_scale, rows = GUMBEL_DEFAULT
    if gumbel is True:
        pass
    elif isinstance(gumbel, dict):
        extra = set(gumbel) - {"m", "c_visit", "c_scale", "improved_rows"}
        if extra:
            raise ValueError("gumbel as a dict takes the keys 'm', 'c_visit', 'c_scale' and 'improved_rows', got %r"
                             % (sorted(map(str, gumbel)),))
        m, c_visit = gumbel.get("m", m), gumbel.get("c_visit", c_visit)
        c_scale, rows = gumbel.get("c_scale", c_scale), gumbel.get("improved_rows", rows)
    elif isinstance(gumbel, (tuple, list)) and len(gumbel) == 3:
        m, c_visit, c_scale = gumbel
    elif isinstance(gumbel, (int, np.integer)):
        m = gumbel
    else:
        raise ValueError("gumbel must be True, an int m, an (m, c_visit, c_scale) triple or a dict with those keys, "
                         "got %r" % (gumbel,))
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)):
        raise ValueError("gumbel: m must be an int in [2, 64] (0 is off), got %r" % (m,))
    m = int(m)
    if m == 0:
        return None
    if not 2 <= m <= 64:
        raise ValueError("gumbel: m must be in [2, 64] (0 is off), got %r" % (m,))
    for name, v in (("c_visit", c_visit), ("c_scale", c_scale)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError("gumbel: %s must be a number, got %r" % (name, v))
    c_visit, c_scale = float(c_visit), float(c_scale)
    if not 0.0 <= c_visit <= 1.0e4:                  # NaN fails both comparisons
        raise ValueError("gumbel: c_visit must be in [0, 1e4], got %r" % (c_visit,))
    if not 0.0 < c_scale <= 100.0:
        raise ValueError("gumbel: c_scale must be in (0, 100], got %r" % (c_scale,))
    if not isinstance(rows, (bool, np.bool_)):
        raise ValueError("gumbel: improved_rows must be True or False, got %r" % (rows,))
    return m, c_visit, c_scale, bool(rows)


def normalize_early_stop(early_stop):
    """`early_stop` as a bool; a ValueError for anything but True / False (None counts as False)."""
    if early_stop is None:
        return False
    if not isinstance(early_stop, (bool, np.bool_)):
        raise ValueError("early_stop must be True or False, got %r" % (early_stop,))
    return bool(early_stop)


def normalize_resign(resign):
    """(threshold, min_ply, keep_prob) of a triple or of a {"threshold": ..., "min_ply": ..., "keep_prob": ...}
    mapping; a ValueError unless threshold is in [-1, 1], min_ply a whole number >= 0 and keep_prob in [0, 1]."""
    try:
        if isinstance(resign, dict):
            if set(resign) != {"threshold", "min_ply", "keep_prob"}:
                raise ValueError
            thr, min_ply, keep = resign["threshold"], resign["min_ply"], resign["keep_prob"]
        else:
            thr, min_ply, keep = resign
        thr, keep = float(thr), float(keep)
        if isinstance(min_ply, bool) or int(min_ply) != min_ply:
            raise ValueError
        min_ply = int(min_ply)
    except (TypeError, ValueError, KeyError):
        raise ValueError("resign must be (threshold, min_ply, keep_prob) or a dict with exactly these three keys, "
                         "got %r" % (resign,)) from None
    if not -1.0 <= thr <= 1.0:              # (false for NaN)
        raise ValueError("resign: threshold %r outside [-1, 1]" % thr)
    if min_ply < 0:
        raise ValueError("resign: min_ply %d is negative" % min_ply)
    if not 0.0 <= keep <= 1.0:
        raise ValueError("resign: keep_prob %r outside [0, 1]" % keep)
    return thr, min_ply, keep


def _net_device(net) -> torch.device:
    """Where a duck-typed net lives: its `device` attribute (HexNetwork, the reference's Network), else its first
    parameter's device."""
    dev = getattr(net, "device", None)
    if dev is not None:
        return torch.device(dev)
    for p in net.parameters() if hasattr(net, "parameters") else ():
        return p.device
    return torch.device("cpu")
