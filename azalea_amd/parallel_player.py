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
from . import fpu as _fpu
from . import policy_temp as _ptemp
from .game.hex import HexGameState
from .play_game import play_game
from .policy import Policy, SearchTreeFull, external_evaluator, tower_flags  # noqa: F401
from .rollout import is_rollout_net, register_evaluator
from .replay_buffer import ReplayDataFrame
from .selfplay_options import (BY_NAME, GUMBEL_DEFAULT, OPTIONS, normalize_early_stop,  # noqa: F401 (re-exported)
                               normalize_forced_playouts, normalize_gumbel, normalize_playout_cap, normalize_resign,
                               normalize_selfplay_openings, normalize_train_targets)

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
                 forced_playouts=None, gumbel=None, selfplay_openings=None, selfplay_opening_weights=None, fpu=None,
                 policy_temp=None):
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
        playing strength and training efficiency is NOT measured.
        `fpu` (NOT the reference's behaviour, which scores an unvisited child with Q = 0; off by default): first-play
        urgency, anything azalea_amd.fpu.normalize_fpu takes -- True (reduction 0.25 below the root, 0 at it; lc0's /
        KataGo's customary values as the author recalls them, not checked here), "absolute" / "reduction", a (mode,
        value, reduction, root_reduction) tuple or a dict with those keys.  Unlike the options above it is a property
        of the SEARCH, not a self-play option: it is put on every agent's Policy (Policy.set_fpu) and from there on every
        engine built for it -- device self-play, external_batch, BOTH engines of device_match, and the host loop's
        single-game engines.  None leaves each policy's own setting (config["fpu"], Policy.set_fpu) as it is.  A
        ValueError for anything normalize_fpu refuses.  DESIGN 7.20 has what was and was not measured.
        `policy_temp` (NOT the reference's behaviour, which searches with the evaluator's prior rows as delivered; off
        by default): a policy temperature for the search's priors, anything
        azalea_amd.policy_temp.normalize_policy_temp takes -- an int m (the rows a search expands from at temperature
        8 / m), an (eighths, root_eighths) tuple or a dict with those keys.  Like `fpu` it is a property of the SEARCH,
        not a self-play option: it is put on every agent's Policy (Policy.set_policy_temp) and from there on every
        engine built for it.  None leaves each policy's own setting as it is.  A ValueError for anything
        normalize_policy_temp refuses.  DESIGN 7.22 has what was and was not measured."""
        self.fpu = _fpu.normalize_fpu(fpu)
        self.policy_temp = _ptemp.normalize_policy_temp(policy_temp)
        if role not in (None, "leader", "follower"):
            raise ValueError("Player role must be None, 'leader' or 'follower'")
        self.openings = [[int(m) for m in o] for o in ([] if openings is None else openings)]
        if self.openings and not device_match:
            raise ValueError("openings are a device_match option: only the device match starts its games from an "
                             "opening book (self-play and the host loop start from the empty board)")
        self.agents = agents
        if self.fpu is not None:
            for a in agents:
                if hasattr(getattr(a, "policy", None), "set_fpu"):
                    a.policy.set_fpu(self.fpu)
        if self.policy_temp is not None:
            for a in agents:
                if hasattr(getattr(a, "policy", None), "set_policy_temp"):
                    a.policy.set_policy_temp(self.policy_temp)
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
        given = dict(selfplay_openings=selfplay_openings, selfplay_opening_weights=selfplay_opening_weights,
                     playout_cap=playout_cap, resign=resign, early_stop=early_stop, train_targets=train_targets,
                     forced_playouts=forced_playouts, gumbel=gumbel)
        for opt in OPTIONS:             # self.playout_cap ... self.selfplay_openings: normalised, or off
            setattr(self, opt.name, self._check_option(opt, *(given[k] for k in opt.keywords)))
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

    def _check_option(self, opt, *given):
        """One entry of selfplay_options.OPTIONS as this Player keeps it -- normalised, or opt.off -- or a ValueError
        naming what does not hold: the normaliser's, "a self-play option" under device_match, an option it excludes,
        "needs a device engine" where the host loop plays, and what the entry's own hooks hold.  No GPU needed."""
        if opt.given is not None:
            value = opt.given(*given)
        else:
            value = opt.off if given[0] is None else opt.normalize(given[0])
        if not opt.is_on(value):
            return opt.off
        if self.device_match:
            raise ValueError("%s is a self-play option: %s" % (opt.name, opt.match_reason))
        other = opt.excluded_by(value, vars(self))
        if other is not None:
            raise ValueError(opt.exclusion_text(other))
        if opt.requires is not None:
            opt.requires(self)
        pol = self._external_policy() if self.external_batch else self._device_policy()
        if pol is None:
            raise ValueError("%s needs the games to run in a device engine (a single agent whose Policy holds a "
                             "HexNetwork, or external_batch=True): these agents play through the host loop, which %s"
                             % (opt.name, opt.host_reason))
        return value if opt.fits is None else opt.fits(self, value, pol)

    def _option_stats(self, name):
        """The option's Engine stats of the self-play engine, or None while there is none or the option is not set."""
        opt = BY_NAME[name]
        if not opt.is_on(getattr(self, name)) or self._engine is None:
            return None
        return getattr(self._engine, opt.stats)()

    def opening_stats(self):
        """Engine.selfplay_openings_stats() of the self-play engine, or None while there is none or selfplay_openings
        is not set."""
        return self._option_stats("selfplay_openings")

    def gumbel_stats(self):
        """Engine.gumbel_stats() of the self-play engine, or None while there is none or gumbel is not set."""
        return self._option_stats("gumbel")

    def forced_playouts_stats(self):
        """Engine.forced_playouts_stats() of the self-play engine, or None while there is none or forced_playouts is
        not set."""
        return self._option_stats("forced_playouts")

    def train_targets_stats(self):
        """Engine.train_targets_stats() of the self-play engine, or None while there is none or train_targets is not set."""
        return self._option_stats("train_targets")

    def early_stop_stats(self):
        """Engine.early_stop_stats() of the self-play engine, or None while there is none or early_stop is not set."""
        return self._option_stats("early_stop")

    def resign_stats(self):
        """Engine.resign_stats() of the self-play engine, or None while there is none or resign is not set."""
        return self._option_stats("resign")

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
            for opt in OPTIONS:          # (the book first, before any play: generation 0 follows it too)
                opt.apply(self._engine, getattr(self, opt.name))
            self._engine_key = key
        _fpu.apply(self._engine, _fpu.policy_fpu(pol))          # a property of the search, not one of OPTIONS
        _ptemp.apply(self._engine, _ptemp.policy_policy_temp(pol))   # likewise
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
        eng = _eng.Engine(board_size=n, n_games=self.n_games, simulations=pol.simulations,
                           search_batch_size=pol.search_batch_size, exploration_coef=pol.exploration_coef,
                           exploration_depth=pol.exploration_depth, noise_alpha=pol.exploration_noise_alpha,
                           noise_scale=noise_scale, temperature=temperature,
                           evaluator=_eng.EVAL_EXTERNAL if external else _eng.EVAL_RESNET,
                           num_blocks=getattr(pol, "num_blocks", 0) if external else pol.num_blocks,
                           base_chans=getattr(pol, "base_chans", 0) if external else pol.base_chans,
                           device=(dev.index or 0) if dev.type == "cuda" else 0, nodes_per_game=int(getattr(pol, "nodes_per_game", 0) or 0),
                           flags=self._engine_flags | tower_flags(pol),
                           seed=(2 * (int(self._seed_base) & 0x3FFFFFFF) + which) << 32)
        _fpu.apply(eng, _fpu.policy_fpu(pol))
        _ptemp.apply(eng, _ptemp.policy_policy_temp(pol))
        return eng

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


def _net_device(net) -> torch.device:
    """Where a duck-typed net lives: its `device` attribute (HexNetwork, the reference's Network), else its first
    parameter's device."""
    dev = getattr(net, "device", None)
    if dev is not None:
        return torch.device(dev)
    for p in net.parameters() if hasattr(net, "parameters") else ():
        return p.device
    return torch.device("cpu")
