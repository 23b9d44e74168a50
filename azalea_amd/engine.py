"""Thin numpy front-end over the C ABI (include/azx.h): one Engine = one azx_engine handle.

Everything here is plumbing: arrays in, arrays out.  The search, the rules and the network
forward all run in libazx_hip.so on the GPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (EVAL_EXTERNAL, EVAL_RESNET, EVAL_UNIFORM, EVAL_UNIFORM_HASH,  # noqa: F401
                   FLAG_NO_COMPACT, FLAG_RANDOM_REFLECT, FLAG_TOWER_F16, AzxError, Config, MatchStats, PlayStats, check)


def _p(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


class _DeviceArray:
    """A device buffer of the engine seen through the CUDA array interface: torch.as_tensor aliases it."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class Engine:
    def __init__(self, board_size=11, n_games=1, simulations=400, search_batch_size=10,
                 exploration_coef=0.5, exploration_depth=15, noise_alpha=0.03, noise_scale=0.25,
                 temperature=1.0, evaluator=EVAL_UNIFORM, num_blocks=6, base_chans=64,
                 nodes_per_game=0, flags=0, device=0, seed=0xBAD5EED5,
                 game_index_stride=1, game_index_offset=0):
        self.L = _lib.lib()
        self.cfg = Config(board_size, n_games, simulations, search_batch_size,
                          float(np.float32(exploration_coef)), exploration_depth, noise_alpha,
                          noise_scale, temperature, evaluator, num_blocks, base_chans,
                          nodes_per_game, flags, device, seed, game_index_stride, game_index_offset)
        self.h = C.c_void_p()
        check(self.L.azx_create(C.byref(self.cfg), C.byref(self.h)))
        self.n = board_size
        self.cells = board_size * board_size
        self.G = n_games
        self.bs = search_batch_size
        self.num_batches = simulations // search_batch_size + 1          # mcts.py:268
        self.selects_per_search = self.num_batches * search_batch_size
        self._last_rows = 0
        self._ext_cb = None            # the registered azx_eval_fn trampoline, kept alive with the engine
        self._ext_exc = None           # what the user's evaluator raised inside the current call

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.azx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        """check() for the calls that may run a registered external evaluator: an exception it raised inside the
        call surfaces itself, chained to the engine's AzxError."""
        exc, self._ext_exc = self._ext_exc, None
        if rc != 0 and exc is not None:
            try:
                check(rc)
            except AzxError as err:
                raise exc from err
        check(rc)

    @property
    def stream(self):
        """The engine's hipStream_t (an int): every kernel of this engine runs on it."""
        return self.L.azx_stream(self.h) or 0

    # ---- set-up -------------------------------------------------------------------------
    def set_external_evaluator(self, fn):
        """azx_set_external_evaluator (EVAL_EXTERNAL engines): fn(board, legal_moves) -> (value, prior) over torch
        tensors on the engine's device -- board int32 [n, N, N] in the first player's view, legal_moves int32
        [n, kmax] (tile + 1, 0-padded), value float32 [n], prior float32 [n, kmax] (entry j = legal move j) -- for
        the whole pool's leaf batch at once.  play / play_device / replay_fill / play_steps / search then call it
        at every evaluation point, and so does Match.play for the slots in which this engine is the mover.  The inputs alias the engine's buffers and are valid during the call only; fn
        runs under torch.no_grad() on the engine's stream, so it needs no synchronisation.  An exception it raises
        fails the engine call and is re-raised from it.  None unregisters."""
        if fn is None:
            check(self.L.azx_set_external_evaluator(self.h, None, None))
            self._ext_cb = None
            return
        import torch
        dev = torch.device("cuda", self.cfg.device)
        N, cells = self.n, self.cells

        def view(ptr, shape, typestr):
            return torch.as_tensor(_DeviceArray(ptr, shape, typestr), device=dev)

        def trampoline(user, n, kmax, board_p, legal_p, value_p, prior_p, stream_p):
            try:
                board = view(board_p, (n, N, N), "<i4")
                legal = view(legal_p, (n, cells), "<i4")[:, :kmax]
                value_out = view(value_p, (n,), "<f4")
                prior_out = view(prior_p, (n, cells), "<f4")
                with torch.no_grad(), torch.cuda.device(dev), \
                        torch.cuda.stream(torch.cuda.ExternalStream(stream_p, device=dev)):
                    value, prior = fn(board, legal)
                    value_out.copy_(torch.as_tensor(value, device=dev).reshape(n))
                    prior_out[:, :kmax].copy_(torch.as_tensor(prior, device=dev).reshape(n, kmax))
                return 0
            except BaseException as exc:       # (an exception must not unwind through the C frames)
                self._ext_exc = exc
                return 1

        cb = _lib.EVAL_FN(trampoline)
        check(self.L.azx_set_external_evaluator(self.h, C.cast(cb, C.c_void_p), None))
        self._ext_cb = cb

    # ---- rollout evaluator (azx_set_rollout_evaluator; NOT the reference's behaviour) ----
    def set_rollout_evaluator(self, rollouts, seed=0):
        """azx_set_rollout_evaluator (EVAL_EXTERNAL engines): every pending position's value is the share of `rollouts`
        (1..4096) uniformly random playouts its mover wins, by the definition in include/azx.h; the priors are uniform.
        The rollout kernel runs where a registered external evaluator would be called -- search / play / play_device /
        replay_fill / play_steps, Match and Tournament -- with no torch tensor and no Python callback in the loop.  It
        replaces a registered external evaluator and is replaced by one; 0 unregisters.  Zeroes rollout_stats().
        Refused on an engine with FLAG_RANDOM_REFLECT."""
        rollouts = int(rollouts)
        if rollouts < 0 or rollouts > 4096:
            raise ValueError("rollouts must be 0 (unregister) or in [1, 4096], got %r" % (rollouts,))
        check(self.L.azx_set_rollout_evaluator(self.h, rollouts, int(seed) & 0xFFFFFFFFFFFFFFFF))
        if rollouts:
            self._ext_cb = None

    def rollout_stats(self):
        """azx_rollout_stats since the evaluator was last registered: dict(handovers, rows, rollouts, rollouts_won)."""
        out = np.zeros(4, np.int64)
        check(self.L.azx_rollout_stats(self.h, _p(out, C.c_int64)))
        return dict(handovers=int(out[0]), rows=int(out[1]), rollouts=int(out[2]), rollouts_won=int(out[3]))

    def set_prior_table(self, table):
        t = np.ascontiguousarray(table, np.float32)
        check(self.L.azx_set_prior_table(self.h, _p(t, C.c_float), t.size))

    def set_weights(self, tensors, on_device=False, sync=True):
        """tensors: {state_dict name: contiguous fp32 numpy array} or {name: (ptr, count)}.
        `on_device`: the pointers are device memory of this GPU (torch tensors).  The engine copies them through its
        own HIP runtime, which knows nothing of torch's streams, so whatever last wrote them -- an optimizer step
        still in flight, a graph replay -- is waited for here (`sync=False`: the caller has already waited for the
        writer, e.g. on an event; play_ahead.PlayAhead)."""
        if on_device and sync:
            import torch
            torch.cuda.synchronize(self.cfg.device)
        names, ptrs, counts, keep = [], [], [], []
        for name, t in tensors.items():
            if name.endswith("num_batches_tracked"):
                continue
            if isinstance(t, tuple):
                ptr, cnt = t
            else:
                a = np.ascontiguousarray(t, np.float32)
                keep.append(a)
                ptr, cnt = a.ctypes.data, a.size
            names.append(name.encode())
            ptrs.append(ptr)
            counts.append(cnt)
        n = len(names)
        c_names = (C.c_char_p * n)(*names)
        c_ptrs = (C.c_void_p * n)(*ptrs)
        c_counts = (C.c_int64 * n)(*counts)
        check(self.L.azx_set_weights(self.h, n, c_names, c_ptrs, c_counts, 1 if on_device else 0))

    def packed_weights(self):
        """{operand name: bytes} -- the packed weight buffers exactly as the kernels read them (azx_debug_weights)."""
        out, which = {}, 0
        while True:
            nbytes = C.c_int64(0)
            name = C.create_string_buffer(64)
            check(self.L.azx_debug_weights(self.h, which, None, 0, C.byref(nbytes), name, 64))
            if nbytes.value < 0:
                return out
            buf = np.empty(nbytes.value, np.uint8)
            check(self.L.azx_debug_weights(self.h, which, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(nbytes), name, 64))
            out[name.value.decode()] = buf
            which += 1

    def weights_digest(self):
        """sha256 over the packed operands: two engines search with the same network iff their digests agree."""
        import hashlib
        h = hashlib.sha256()
        for name, buf in sorted(self.packed_weights().items()):
            h.update(name.encode())
            h.update(buf.tobytes())
        return h.hexdigest()

    def reset(self, slots=None, moves=None):
        """Reset slots (all by default); `moves` = list of move lists replayed per slot."""
        s = None if slots is None else np.ascontiguousarray(slots, np.int32)
        ns = self.G if s is None else len(s)
        if moves is None:
            check(self.L.azx_reset(self.h, _p(s, C.c_int32), ns, None, None, 0))
            return
        stride = max(1, max(len(m) for m in moves))
        mv = np.zeros((ns, stride), np.int32)
        nm = np.zeros(ns, np.int32)
        for i, m in enumerate(moves):
            mv[i, :len(m)] = m
            nm[i] = len(m)
        check(self.L.azx_reset(self.h, _p(s, C.c_int32), ns, _p(mv, C.c_int32), _p(nm, C.c_int32), stride))

    # ---- search -------------------------------------------------------------------------
    def set_active(self, mask):
        m = np.ascontiguousarray(mask, np.int32)
        assert m.shape == (self.G,)
        check(self.L.azx_set_active(self.h, _p(m, C.c_int32)))

    def _noise_args(self, noise):
        """(rows pointer, n_select, stride) of azx_search / azx_search_begin for float64 [G, n_select, stride] host
        Dirichlet rows, or for None; the array is returned with them to be kept alive over the call."""
        if noise is None:
            return (None, 0, 0), None
        nz = np.ascontiguousarray(noise, np.float64)
        assert nz.ndim == 3 and nz.shape[0] == self.G
        return (_p(nz, C.c_double), nz.shape[1], nz.shape[2]), nz

    def search(self, noise=None, noise_scale=0.0):
        """noise: float64 [G, n_select, stride] host Dirichlet rows, or None."""
        args, _keep = self._noise_args(noise)
        self._check(self.L.azx_search(self.h, *args, noise_scale))

    def search_begin(self, noise=None, noise_scale=0.0):
        n = C.c_int(0)
        args, _keep = self._noise_args(noise)
        check(self.L.azx_search_begin(self.h, *args, noise_scale, C.byref(n)))
        return n.value

    def search_step(self):
        n, done = C.c_int(0), C.c_int(0)
        check(self.L.azx_search_step(self.h, C.byref(n), C.byref(done)))
        return n.value, bool(done.value)

    def get_leaves(self):
        cap = self.G * self.bs
        boards = np.zeros((cap, self.n, self.n), np.int32)
        lm = np.zeros((cap, self.cells), np.int32)
        slot = np.zeros(cap, np.int32)
        k = np.zeros(cap, np.int32)
        n = C.c_int(0)
        check(self.L.azx_get_leaves(self.h, cap, _p(boards, C.c_int32), _p(lm, C.c_int32),
                                    _p(slot, C.c_int32), _p(k, C.c_int32), C.byref(n)))
        n = n.value
        return boards[:n], lm[:n], slot[:n], k[:n]

    def put_evals(self, value, prior):
        v = np.ascontiguousarray(value, np.float32)
        p = np.zeros((len(v), self.cells), np.float32)
        pr = np.asarray(prior, np.float32)
        if len(v):
            p[:, :pr.shape[1]] = pr
        check(self.L.azx_put_evals(self.h, len(v), _p(v, C.c_float), _p(p, C.c_float)))

    def get_evals(self):
        """Device-network results for the pending leaves (EVAL_RESNET + phase API)."""
        cap = self.G * self.bs
        v = np.zeros(cap, np.float32)
        p = np.zeros((cap, self.cells), np.float32)
        n = C.c_int(0)
        check(self.L.azx_get_evals(self.h, cap, _p(v, C.c_float), _p(p, C.c_float), C.byref(n)))
        return v[:n.value], p[:n.value]

    def _search_phases(self, on_leaves, noise, noise_scale):
        """One search driven phase by phase: on_leaves(boards, legal_moves, slot, k) after every phase that left
        leaves pending, in mcts.sample_paths' call order."""
        n = self.search_begin(noise, noise_scale)
        done = False
        while not done:
            if n:
                on_leaves(*self.get_leaves())
            n, done = self.search_step()

    def search_recorded(self, noise=None, noise_scale=0.0):
        """EVAL_RESNET search driven phase by phase, returning the evaluation tape
        [(slot, k, value, prior[:k])] in mcts.evaluate_batch order."""
        tape = []

        def record(b, lm, slot, k):
            v, p = self.get_evals()
            tape.extend((int(slot[i]), int(k[i]), np.float32(v[i]), p[i, :k[i]].copy()) for i in range(len(k)))
        self._search_phases(record, noise, noise_scale)
        return tape

    def search_external(self, evaluate, noise=None, noise_scale=0.0):
        """Drive one search with a host evaluator: evaluate(boards, legal_moves, slot, k) ->
        (value[n], prior[n, >=max k]).  Mirrors mcts.sample_paths' call order."""
        self._search_phases(lambda *leaves: self.put_evals(*evaluate(*leaves)), noise, noise_scale)

    # ---- results ------------------------------------------------------------------------
    def get_root(self):
        G, Cn = self.G, self.cells
        out = dict(k=np.zeros(G, np.int32), legal_moves=np.zeros((G, Cn), np.int32),
                   child_visits=np.zeros((G, Cn), np.float32),
                   child_value=np.zeros((G, Cn), np.float32),
                   child_prior=np.zeros((G, Cn), np.float32), root_visits=np.zeros(G, np.float32),
                   root_value=np.zeros(G, np.float32), num_nodes=np.zeros(G, np.int32),
                   search_value=np.zeros(G, np.float32))
        check(self.L.azx_get_root(
            self.h, _p(out["k"], C.c_int32), _p(out["legal_moves"], C.c_int32),
            _p(out["child_visits"], C.c_float), _p(out["child_value"], C.c_float),
            _p(out["child_prior"], C.c_float), _p(out["root_visits"], C.c_float),
            _p(out["root_value"], C.c_float), _p(out["num_nodes"], C.c_int32),
            _p(out["search_value"], C.c_float)))
        return out

    def get_status(self):
        st = np.zeros(self.G, np.int32)
        check(self.L.azx_get_status(self.h, _p(st, C.c_int32)))
        return st

    def get_tree_nodes(self):
        """SearchTree.num_nodes as the reference counts it (never reclaimed; search_tree.py:112)."""
        nn = np.zeros(self.G, np.int32)
        check(self.L.azx_get_tree_nodes(self.h, _p(nn, C.c_int32)))
        return nn

    def get_games(self):
        G = self.G
        board = np.zeros((G, self.n, self.n), np.int32)
        color, result, ply = (np.zeros(G, np.int32) for _ in range(3))
        check(self.L.azx_get_games(self.h, _p(board, C.c_int32), _p(color, C.c_int32),
                                   _p(result, C.c_int32), _p(ply, C.c_int32)))
        return dict(board=board, color=color, result=result, ply=ply)

    def advance(self, move_ids):
        m = np.ascontiguousarray(move_ids, np.int32)
        assert m.shape == (self.G,)
        check(self.L.azx_advance(self.h, _p(m, C.c_int32)))

    def tree_dump(self, slot=0, cap=None):
        if cap is None:
            cap = int(self.get_root()["num_nodes"][slot]) + 8
        arrs = dict(parent=np.zeros(cap, np.int32), first_child=np.zeros(cap, np.int32),
                    num_children=np.zeros(cap, np.int32), num_visits=np.zeros(cap, np.float32),
                    total_value=np.zeros(cap, np.float32), prior_prob=np.zeros(cap, np.float32))
        nn, rid = C.c_int32(0), C.c_int32(0)
        check(self.L.azx_tree_dump(
            self.h, slot, cap, _p(arrs["parent"], C.c_int32), _p(arrs["first_child"], C.c_int32),
            _p(arrs["num_children"], C.c_int32), _p(arrs["num_visits"], C.c_float),
            _p(arrs["total_value"], C.c_float), _p(arrs["prior_prob"], C.c_float),
            C.byref(nn), C.byref(rid)))
        out = {k: v[:nn.value].copy() for k, v in arrs.items()}
        out["num_nodes"], out["root_id"] = nn.value, rid.value
        return out

    def forward(self, boards, legal_moves):
        b = np.ascontiguousarray(boards, np.int32)
        lm = np.ascontiguousarray(legal_moves, np.int32)
        B, K = lm.shape
        value = np.zeros(B, np.float32)
        logprob = np.zeros((B, K), np.float32)
        check(self.L.azx_forward(self.h, B, K, _p(b, C.c_int32), _p(lm, C.c_int32),
                                 _p(value, C.c_float), _p(logprob, C.c_float)))
        return value, logprob

    # ---- throughput mode ------------------------------------------------------------------
    def play(self, min_positions, max_plies=0):
        cap = int(min_positions) + self.G * self.cells
        board = np.zeros((cap, self.n, self.n), np.int32)
        color = np.zeros(cap, np.int32)
        nlegal = np.zeros(cap, np.int32)
        prob = np.zeros((cap, self.cells), np.float32)
        reward = np.zeros(cap, np.float32)
        uid = np.zeros(cap, np.int64)
        st = PlayStats()
        self._check(self.L.azx_play(self.h, int(min_positions), int(max_plies), cap,
                              _p(board, C.c_int32), _p(color, C.c_int32), _p(nlegal, C.c_int32),
                              _p(prob, C.c_float), _p(reward, C.c_float), _p(uid, C.c_int64),
                              C.byref(st)))
        n = st.positions
        self._last_rows = int(n)
        return dict(board=board[:n], color=color[:n], nlegal=nlegal[:n], moves_prob=prob[:n],
                    reward=reward[:n], game_uid=uid[:n]), st.as_dict()

    # azx_play_row_metrics columns -> the reference's per-ply metric names (search_tree.py:109-112, mcts.py:291,
    # policy.py:164); column 3 flags the first row of a game
    ROW_METRIC_COLUMNS = (("search_value", 0), ("search_root_width", 1), ("action_logprob", 2),
                          ("search_root_visits", 4), ("search_tree_nodes", 5), ("search_root_children", 6))

    def game_metric_sums(self, rows=None):
        """Sums over the games of the last play()/play_device()/replay_fill() call of each game's per-ply MEANS
        of the search metrics, by the reference's key names: what Player.read's metrics add up
        (play_game.py:73-76, parallel_player.py:50-51)."""
        m = self.play_row_metrics(rows)
        names = [k for k, _ in self.ROW_METRIC_COLUMNS]
        if len(m) == 0:
            return dict.fromkeys(names, 0.0)
        starts = np.flatnonzero(m[:, 3] > 0.5)
        if len(starts) == 0 or starts[0] != 0:
            starts = np.r_[0, starts]
        cols = [c for _, c in self.ROW_METRIC_COLUMNS]
        sums = np.add.reduceat(m[:, cols].astype(np.float64), starts, axis=0)
        lens = np.diff(np.r_[starts, len(m)])
        return dict(zip(names, (sums / lens[:, None]).sum(0).tolist()))

    def play_row_metrics(self, rows=None):
        """azx_play_row_metrics: [rows, AZX_ROW_METRICS] for the rows of the last play() / play_device() call
        (`rows`: how many that call returned, if known); columns: ROW_METRIC_COLUMNS, 3 = first row of a game."""
        cap = int(rows) if rows is not None else self._last_rows
        m = np.zeros((max(1, cap), _lib.ROW_METRICS), np.float32)
        n = C.c_int64(0)
        check(self.L.azx_play_row_metrics(self.h, max(1, cap), _p(m, C.c_float), C.byref(n)))
        return m[:n.value]

    def kernel_info(self):
        """azx_kernel_info: which kernels this engine launches (and the diagnostic switches it was created under)."""
        buf = C.create_string_buffer(2048)
        n = self.L.azx_kernel_info(self.h, buf, len(buf))
        if n < 0:
            check(n)
        return buf.value.decode()

    def debug_set_queue_cap(self, rows):
        """tests: bound the harvest queue of the following play calls (0 = no bound)."""
        check(self.L.azx_debug_set_queue_cap(self.h, int(rows)))

    def debug_stagger(self):
        """azx_debug_stagger: the pipelined play loop's staggered starts since creation, as a dict (rows_behind: rows the
        last second sub-launch evaluated, rows_queued: rows queued for that evaluation, starts, empty: starts whose
        second sub-launch found nothing to do)."""
        out = np.zeros(4, np.int32)
        check(self.L.azx_debug_stagger(self.h, _p(out, C.c_int32)))
        return dict(zip(("rows_behind", "rows_queued", "starts", "empty"), out.tolist()))

    def play_device(self, min_positions, max_plies=0):
        """azx_play_device: whole games until >= min_positions rows sit in the harvest queue (in HBM)."""
        st = PlayStats()
        rows = C.c_int64(0)
        self._check(self.L.azx_play_device(self.h, int(min_positions), int(max_plies), C.byref(rows), C.byref(st)))
        self._last_rows = int(rows.value)
        return rows.value, st.as_dict()

    def rows_read(self, first, n):
        """azx_rows_read: rows [first, first + n) of the harvest queue as the dict play() returns -- whatever filled
        the queue last: play() / play_device(), or a collecting Match / Tournament that has this engine as its sink."""
        first, n = int(first), int(n)
        board = np.zeros((n, self.n, self.n), np.int32)
        color = np.zeros(n, np.int32)
        nlegal = np.zeros(n, np.int32)
        prob = np.zeros((n, self.cells), np.float32)
        reward = np.zeros(n, np.float32)
        uid = np.zeros(n, np.int64)
        check(self.L.azx_rows_read(self.h, first, n, _p(board, C.c_int32), _p(color, C.c_int32), _p(nlegal, C.c_int32),
                                   _p(prob, C.c_float), _p(reward, C.c_float), _p(uid, C.c_int64)))
        return dict(board=board, color=color, nlegal=nlegal, moves_prob=prob, reward=reward, game_uid=uid)

    def rows_pack(self, first, n, records_ptr):
        """queue rows [first, first+n) -> fixed-size records in the device buffer at records_ptr."""
        check(self.L.azx_rows_pack(self.h, int(first), int(n), C.c_void_p(int(records_ptr))))

    def replay_put_records(self, n, records_ptr):
        """n records from a device buffer into the replay ring (FIFO)."""
        check(self.L.azx_replay_put_records(self.h, int(n), C.c_void_p(int(records_ptr))))

    def replay_put_records_async(self, n, records_ptr, stream):
        """The same put enqueued on `stream` (a hipStream_t value) and not synchronised: the one engine call that may
        run on another host thread than a play in progress (include/azx.h)."""
        check(self.L.azx_replay_put_records_async(self.h, int(n), C.c_void_p(int(records_ptr)), C.c_void_p(int(stream))))

    def reserve_cus(self, cus_per_xcd):
        """Keep `cus_per_xcd` CUs of every XCD (rounded up to 4: one per shader engine) free of this engine's kernels;
        0 = use all.  Returns the CUs left free on the whole device."""
        out = C.c_int(0)
        check(self.L.azx_reserve_cus(self.h, int(cus_per_xcd), C.byref(out)))
        return out.value

    @property
    def record_bytes(self):
        return _lib.record_bytes(self.cells)

    def debug_counters(self):
        out = np.zeros(16, np.uint64)
        check(self.L.azx_debug_counters(self.h, _p(out, C.c_uint64)))
        return out

    # ---- device-resident replay ring (azx_replay_*) -------------------------------------------
    def replay_create(self, capacity):
        check(self.L.azx_replay_create(self.h, int(capacity)))

    def replay_state(self):
        v = [C.c_int64(0) for _ in range(3)]
        check(self.L.azx_replay_state(self.h, *(C.byref(x) for x in v)))
        return dict(capacity=v[0].value, size=v[1].value, write_idx=v[2].value)

    def replay_set_state(self, size, write_idx):
        check(self.L.azx_replay_set_state(self.h, int(size), int(write_idx)))

    def replay_put(self, board, color, nlegal, moves_prob, reward):
        """Host rows (azx_play layout: board i32[P,cells], moves_prob f32[P,cells] dense by child
        index) into the ring, FIFO."""
        P = len(reward)
        cells = self.n * self.n
        board = np.ascontiguousarray(board, np.int32).reshape(P, cells)
        prob = np.ascontiguousarray(moves_prob, np.float32).reshape(P, cells)
        color = np.ascontiguousarray(color, np.int32)
        nlegal = np.ascontiguousarray(nlegal, np.int32)
        reward = np.ascontiguousarray(reward, np.float32)
        check(self.L.azx_replay_put(self.h, P, _p(board, C.c_int32), _p(color, C.c_int32),
                                    _p(nlegal, C.c_int32), _p(prob, C.c_float), _p(reward, C.c_float)))

    def replay_fill(self, min_positions, max_plies=0):
        st = PlayStats()
        rows = C.c_int64(0)
        self._check(self.L.azx_replay_fill(self.h, int(min_positions), int(max_plies), C.byref(rows), C.byref(st)))
        self._last_rows = int(rows.value)
        return rows.value, st.as_dict()

    def replay_collate(self, indices, out):
        """indices: int64 host array; out: dict of device pointers (ints) color, legal_moves,
        result, board, moves_prob, reward.  Returns the batch's largest legal-move count."""
        idx = np.ascontiguousarray(indices, np.int64)
        mk = C.c_int32(0)
        check(self.L.azx_replay_collate(self.h, len(idx), _p(idx, C.c_int64),
                                        *(C.c_void_p(int(out[k])) for k in
                                          ("color", "legal_moves", "result", "board", "moves_prob", "reward")),
                                        C.byref(mk)))
        return mk.value

    def replay_set_mover_view(self, on: bool):
        """azx_replay_set_mover_view: the collates hand out the second player's rows as the search sees them."""
        check(self.L.azx_replay_set_mover_view(self.h, 1 if on else 0))

    def replay_set_reflect(self, on: bool, seed: int = 0):
        """azx_replay_set_reflect: the collates hand out about half their rows turned by 180 degrees, the bit of
        output row b a function of (seed, collates since this call, b).  Every call restarts the collate count."""
        check(self.L.azx_replay_set_reflect(self.h, 1 if on else 0, int(seed) & 0xFFFFFFFFFFFFFFFF))

    def replay_collate_async(self, indices, out, stream):
        """replay_collate enqueued on `stream` (a hipStream_t as int) without synchronising and without max_k."""
        idx = np.ascontiguousarray(indices, np.int64)
        check(self.L.azx_replay_collate_async(self.h, len(idx), _p(idx, C.c_int64),
                                              *(C.c_void_p(int(out[k])) for k in
                                                ("color", "legal_moves", "result", "board", "moves_prob", "reward")),
                                              C.c_void_p(int(stream))))

    def debug_choose(self):
        """azx_debug_choose: (move_id[G], moves_prob[G, cells]) of the device move draw on the current roots."""
        mid = np.zeros(self.G, np.int32)
        prob = np.zeros((self.G, self.cells), np.float32)
        check(self.L.azx_debug_choose(self.h, _p(mid, C.c_int32), _p(prob, C.c_float)))
        return mid, prob

    def debug_counters_raw(self):
        out = np.zeros((self.G, 16), np.uint64)
        check(self.L.azx_debug_counters_raw(self.h, _p(out, C.c_uint64), self.G))
        return out

    def debug_slow_div(self):
        """azx_debug_slow_div: int32 [G], 1 where a slot's scores go through the IEEE divide (a value outside the unscaled
        divide's range has reached its tree since its last reset)."""
        out = np.zeros(self.G, np.int32)
        check(self.L.azx_debug_slow_div(self.h, _p(out, C.c_int32)))
        return out

    def play_steps(self, plies):
        st = PlayStats()
        self._check(self.L.azx_play_steps(self.h, int(plies), C.byref(st)))
        return st.as_dict()

    def _stats(self, fn, names):
        """An option's fixed-size counters (the library fills at most 8 int64) as a dict of ints by `names`."""
        out = np.zeros(8, np.int64)
        check(fn(self.h, _p(out, C.c_int64)))
        return {k: int(out[i]) for i, k in enumerate(names)}

    # ---- playout cap randomisation (azx_set_playout_cap; NOT the reference's behaviour) ------------
    def set_playout_cap(self, full_prob, fast_simulations):
        """azx_set_playout_cap: every ply of the following play / play_device / replay_fill / play_steps calls is with
        probability `full_prob` a full search (cfg.simulations, Dirichlet noise, one replay row) and otherwise a fast
        one of `fast_simulations` (no noise, no row; the move is drawn as always).  search(), the phase API and
        forward() are untouched; Match / Tournament refuse a capped engine.  ValueError, with the library's message,
        for full_prob outside (0, 1] or fast_simulations outside [1, simulations]; the setting before stays then.
        (1.0, simulations) and (1.0, 0) clear the cap."""
        rc = self.L.azx_set_playout_cap(self.h, float(full_prob), int(fast_simulations))
        if rc == -1:                # AZX_EINVAL
            raise ValueError(self.L.azx_last_error().decode(errors="replace"))
        check(rc)

    def clear_playout_cap(self):
        """Self-play as before set_playout_cap: the same kernels, the same bytes."""
        check(self.L.azx_set_playout_cap(self.h, 1.0, 0))

    def playout_cap_stats(self):
        """azx_playout_cap_stats since the cap was last set: dict(full_plies, fast_plies, empty_games) -- empty_games
        are the finished games none of whose plies was a full search (they contributed no rows)."""
        return self._stats(self.L.azx_playout_cap_stats, ("full_plies", "fast_plies", "empty_games"))

    # ---- weighted opening book of self-play (azx_set_selfplay_openings; NOT the reference's behaviour) ------------
    def set_selfplay_openings(self, openings, weights=None):
        """azx_set_selfplay_openings: every game this engine starts from now on -- a slot's restart inside play /
        play_device / replay_fill / play_steps, reset() without moves -- begins from the opening of `openings` (a list
        of move lists, tile + 1 in play order, colour 1 first; [] is the empty board) that its uid draws under
        `weights` (None: uniform): selfplay_opening_index(seed, uid, selfplay_openings_bounds(weights)).  Slots whose
        game has not begun are seated again at once, keeping their uid; games in progress finish as they are.
        reset(moves=...) seats what it is given for that one game.  An empty list clears the book.  ValueError, with the
        library's message, for a book openings_check refuses or weights that are negative, non-finite or all zero; the
        book before stays then.  Match / Tournament refuse an engine with a self-play book."""
        n, stride, mv, ln = _book_arrays(openings)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, np.float64).reshape(-1)
            if w.size != n:
                raise ValueError("selfplay openings: %d weights for %d openings" % (w.size, n))
        _book_error(self.L.azx_set_selfplay_openings(self.h, n, stride, _p(mv, C.c_int16), _p(ln, C.c_int32),
                                                     _p(w, C.c_double) if n else None))
        self._selfplay_book = n

    def clear_selfplay_openings(self):
        """Self-play as before set_selfplay_openings: the same kernels, the same bytes."""
        check(self.L.azx_set_selfplay_openings(self.h, 0, 0, None, None, None))
        self._selfplay_book = 0

    def selfplay_openings_slots(self):
        """azx_selfplay_openings_slots: int32[n_games], the book index of each slot's game in progress, -1 where it did
        not come from the installed book."""
        out = np.zeros(self.G, np.int32)
        check(self.L.azx_selfplay_openings_slots(self.h, _p(out, C.c_int32)))
        return out

    def selfplay_openings_stats(self):
        """azx_selfplay_openings_stats since the book was last set: dict(started, finished, wins_color1, plies) of
        int64[n_openings] arrays -- plies are those of the finished games, counted from the empty board."""
        n = int(getattr(self, "_selfplay_book", 0))
        out = np.zeros((max(n, 1), 4), np.int64)
        rc = self.L.azx_selfplay_openings_stats(self.h, n, _p(out, C.c_int64))
        if rc < 0:
            check(rc)
        out = out[:n]
        return dict(started=out[:, 0].copy(), finished=out[:, 1].copy(), wins_color1=out[:, 2].copy(),
                    plies=out[:, 3].copy())

    # ---- resignation with no-resign calibration games (azx_set_resign; NOT the reference's behaviour) ------------
    def set_resign(self, threshold, min_ply=0, keep_prob=0.1):
        """azx_set_resign: in the following play / play_device / replay_fill / play_steps calls the mover of a game
        that is not exempt resigns at a ply >= `min_ply` whose root value v = root_value / root_visits (the mover's
        view, one float32 division) is below `threshold`; the game ends there, lost by the resigner, and is harvested
        like any finished game.  A share `keep_prob` of the games -- a pure function of (seed, uid),
        resign_is_exempt() -- is exempt, plays to the end and only remembers its first crossing.  Row metric 7 carries
        v while resignation is set.  search(), the phase API and advance() never resign; Match / Tournament refuse a
        resigning engine.  ValueError, with the library's message, for a threshold outside [-1, 1], a negative min_ply
        or a keep_prob outside [0, 1]; the setting before stays then.  Zeroes resign_stats()."""
        rc = self.L.azx_set_resign(self.h, float(threshold), int(min_ply), float(keep_prob))
        if rc == -1:                # AZX_EINVAL
            raise ValueError(self.L.azx_last_error().decode(errors="replace"))
        check(rc)

    def clear_resign(self):
        """Self-play as before set_resign: the same kernels, the same bytes."""
        check(self.L.azx_clear_resign(self.h))

    RESIGN_STATS = ("resigned", "played_out", "exempt", "exempt_crossed", "false_positives", "sum_resign_ply",
                    "sum_plies_saved")

    def resign_stats(self):
        """azx_resign_stats since the last set_resign, over the games that started and finished after it:
        dict(resigned, played_out, exempt, exempt_crossed, false_positives, sum_resign_ply, sum_plies_saved) --
        false_positives are the exempt games whose crossing mover went on to win, sum_plies_saved the plies between
        the exempt games' crossings and their ends."""
        return self._stats(self.L.azx_resign_stats, self.RESIGN_STATS)

    # ---- early stop of decided searches (azx_set_early_stop; NOT the reference's behaviour) ------------
    def set_early_stop(self, on=True):
        """azx_set_early_stop: in the following play / play_device / replay_fill / play_steps calls the search of a ply
        that is drawn at temperature 0 (ply >= exploration_depth, or temperature 0) stops at the first batch boundary at
        which the most-visited root child leads the second by more than the selects still to come: they could change
        neither the move nor the one-hot row (include/azx.h states the rule).  The carried subtree is thinner for it.
        NOT the reference's behaviour, which runs every search to its last simulation; off by default.  search(), the
        phase API and matches are untouched; Match / Tournament refuse an engine with the option set.
        set_early_stop(False) clears it: the same kernels, the same bytes as before.  Zeroes early_stop_stats().  What
        it buys is given in DESIGN 7.11; its effect on playing strength and training efficiency is not measured."""
        if on not in (True, False, 0, 1):
            raise ValueError("early stop: on must be True or False, got %r" % (on,))
        check(self.L.azx_set_early_stop(self.h, 1 if on else 0))

    EARLY_STOP_STATS = ("t0_plies", "stopped_plies", "batches_skipped")

    def early_stop_stats(self):
        """azx_early_stop_stats since the last set_early_stop: dict(t0_plies, stopped_plies, batches_skipped) -- the
        temperature-0 plies searched under the option, those stopped before their last batch, and the sum of the
        batches they had left."""
        return self._stats(self.L.azx_early_stop_stats, self.EARLY_STOP_STATS)

    # ---- training targets of the recorded rows (azx_set_train_targets; NOT the reference's behaviour) ----
    POLICY_ROWS = ("reference", "visits")      # AZX_ROWS_REFERENCE, AZX_ROWS_VISITS

    def set_train_targets(self, policy_rows="reference", value_mix=0.0):
        """azx_set_train_targets: what the rows of the following play / play_device / replay_fill / play_steps calls
        teach.  policy_rows="visits": the row of every recorded ply is counts / sum(counts) of the root's children,
        whatever temperature drew the move (the reference's row is one-hot on the most-visited child from
        exploration_depth on).  value_mix = lambda in [0, 1]: the stored reward is (1 - lambda) * z + lambda * v, z the
        game's outcome and v = root.total_value / root.num_visits after the ply's search, both in the mover's view; row
        metric 7 carries v.  The move draw is untouched: the games are the games of the same seed with the option off
        (include/azx.h has the definition).  NOT the reference's behaviour; off by default.  search(), the phase API
        and matches are untouched; Match / Tournament refuse an engine with the option set.  ("reference", 0.0) is
        "off": the same kernels, the same bytes as before.  Zeroes train_targets_stats().  DESIGN 7.12 has what is
        measured of its effect."""
        if policy_rows not in self.POLICY_ROWS:
            raise ValueError("train targets: policy_rows must be 'reference' or 'visits', got %r" % (policy_rows,))
        value_mix = float(value_mix)
        if not 0.0 <= value_mix <= 1.0:
            raise ValueError("train targets: value_mix must be in [0, 1], got %r" % (value_mix,))
        check(self.L.azx_set_train_targets(self.h, self.POLICY_ROWS.index(policy_rows), value_mix))

    def clear_train_targets(self):
        """set_train_targets("reference", 0.0): the reference's rows and the game's outcome again."""
        check(self.L.azx_set_train_targets(self.h, 0, 0.0))

    def train_targets(self):
        """azx_get_train_targets: the pair (policy_rows, value_mix) in force, ("reference", 0.0) when off."""
        rows, mix = C.c_int(0), C.c_float(0.0)
        if getattr(self.L, "azx_get_train_targets", None) is None:     # an older build (tools/lib_bench.py): never set
            return self.POLICY_ROWS[0], 0.0
        check(self.L.azx_get_train_targets(self.h, C.byref(rows), C.byref(mix)))
        return self.POLICY_ROWS[rows.value], float(mix.value)

    TRAIN_TARGETS_STATS = ("rows", "greedy_rows", "greedy_rows_wide")

    def train_targets_stats(self):
        """azx_train_targets_stats since the last set_train_targets: dict(rows, greedy_rows, greedy_rows_wide) -- the
        rows recorded while the option is on, of those the rows of plies drawn at temperature 0, and of those the rows
        with more than one visited child (the rows that differ from the reference's)."""
        return self._stats(self.L.azx_train_targets_stats, self.TRAIN_TARGETS_STATS)

    # ---- forced playouts and policy target pruning (azx_set_forced_playouts; NOT the reference's behaviour) ----
    def set_forced_playouts(self, k=2.0, prune=True):
        """azx_set_forced_playouts: in the following play / play_device / replay_fill / play_steps calls the root level
        of every select of a full search descends into the lowest-index root child with n > 0 and n * n < (k * P) * S,
        if there is one, instead of the PUCT argmax (n its visits as the select sees them, P the prior the select
        scores with, S the children's visit sum); with prune=True the move draw and the recorded row of a full ply
        that is not drawn greedily (and every full ply's row under set_train_targets("visits")) are made from the pruned
        counts: each child below the maximum gives back the visits PUCT would not have spent on it (include/azx.h
        states both rules).  A playout cap's fast plies neither force nor prune.  NOT the reference's behaviour; off by
        default.  search(), the phase API and matches are untouched; Match / Tournament refuse an engine with the
        option set.  set_forced_playouts(0, False) clears it: the same kernels, the same bytes as before.  Zeroes
        forced_playouts_stats().  DESIGN 7.13 has what was measured; its effect on playing strength and training
        efficiency is not measured."""
        k = float(k)
        if not 0.0 <= k <= 64.0:                    # NaN fails both comparisons
            raise ValueError("forced playouts: k must be in [0, 64], got %r" % (k,))
        if prune not in (True, False, 0, 1):
            raise ValueError("forced playouts: prune must be True or False, got %r" % (prune,))
        if k == 0.0 and prune:
            raise ValueError("forced playouts: pruning needs forcing (k > 0)")
        check(self.L.azx_set_forced_playouts(self.h, k, 1 if prune else 0))

    def clear_forced_playouts(self):
        """set_forced_playouts(0, False): PUCT selects and raw counts again."""
        check(self.L.azx_set_forced_playouts(self.h, 0.0, 0))

    def forced_playouts(self):
        """azx_get_forced_playouts: the pair (k, prune) in force, (0.0, False) when off."""
        k, prune = C.c_float(0.0), C.c_int(0)
        if getattr(self.L, "azx_get_forced_playouts", None) is None:   # an older build (tools/lib_bench.py): never set
            return 0.0, False
        check(self.L.azx_get_forced_playouts(self.h, C.byref(k), C.byref(prune)))
        return float(k.value), bool(prune.value)

    FORCED_PLAYOUTS_STATS = ("full_plies", "forced_selects", "rows_pruned", "visits_removed")

    def forced_playouts_stats(self):
        """azx_forced_playouts_stats since the last set_forced_playouts: dict(full_plies, forced_selects, rows_pruned,
        visits_removed) -- the full plies chosen under the option, the selects whose forced set was non-empty, the
        recorded rows with at least one reduced child and the visits removed from recorded rows."""
        return self._stats(self.L.azx_forced_playouts_stats, self.FORCED_PLAYOUTS_STATS)

    # ---- Gumbel root search with sequential halving (azx_set_gumbel; NOT the reference's behaviour) ----
    def set_gumbel(self, m=16, c_visit=50.0, c_scale=1.0, improved_rows=True):
        """azx_set_gumbel: in the following play / play_device / replay_fill / play_steps calls every search is a Gumbel
        root search (include/azx.h has the definition, DESIGN 7.14 its two deviations from Danihelka et al. 2022):
        min(m, k) root candidates are sampled without replacement by g + ln P, the search's select batches are divided
        among them by sequential halving on g + ln P + sigma(completed Q), no Dirichlet noise is mixed in, the final
        survivor is played, and with improved_rows=True the recorded row is softmax(ln P + sigma) over all children.
        improved_rows=False keeps the row the engine records otherwise (a diagnostic and test mode).  A playout cap's
        fast plies search under the option too.  m = 0 is off; otherwise 2 <= m <= 64, c_visit in [0, 1e4], c_scale in
        (0, 100].  The defaults c_visit = 50 and c_scale = 1.0 are the author's recollection of the paper's board-game
        values and are not checked here.  NOT the reference's behaviour; off by default.  search(), the phase API and
        matches are untouched; Match / Tournament refuse an engine with the option set, and it cannot be set beside
        forced playouts or early stop (rules about PUCT visit leaders).  set_gumbel(0) clears it: the same kernels, the
        same bytes as before.  Zeroes gumbel_stats().  Its effect on playing strength and training efficiency is NOT
        measured."""
        m = int(m)
        if m != 0 and not 2 <= m <= 64:
            raise ValueError("gumbel: m must be 0 (off) or in [2, 64], got %r" % (m,))
        c_visit, c_scale = float(c_visit), float(c_scale)
        if m != 0:
            if not 0.0 <= c_visit <= 1.0e4:             # NaN fails both comparisons
                raise ValueError("gumbel: c_visit must be in [0, 1e4], got %r" % (c_visit,))
            if not 0.0 < c_scale <= 100.0:
                raise ValueError("gumbel: c_scale must be in (0, 100], got %r" % (c_scale,))
            if improved_rows not in (True, False, 0, 1):
                raise ValueError("gumbel: improved_rows must be True or False, got %r" % (improved_rows,))
        check(self.L.azx_set_gumbel(self.h, m, c_visit, c_scale, 1 if (m != 0 and improved_rows) else 0))

    def clear_gumbel(self):
        """set_gumbel(0): PUCT root selects, Dirichlet noise and the move draw from the counts again."""
        check(self.L.azx_set_gumbel(self.h, 0, 0.0, 1.0, 0))

    def gumbel(self):
        """azx_get_gumbel: (m, c_visit, c_scale, improved_rows) in force, (0, 0.0, 0.0, False) when off."""
        if getattr(self.L, "azx_get_gumbel", None) is None:     # an older build (tools/lib_bench.py): never set
            return 0, 0.0, 0.0, False
        m, cv, cs, rows = C.c_int(0), C.c_float(0.0), C.c_float(0.0), C.c_int(0)
        check(self.L.azx_get_gumbel(self.h, C.byref(m), C.byref(cv), C.byref(cs), C.byref(rows)))
        return int(m.value), float(cv.value), float(cs.value), bool(rows.value)

    GUMBEL_STATS = ("plies", "halvings", "root_selects", "improved_rows")

    def gumbel_stats(self):
        """azx_gumbel_stats since the last set_gumbel: dict(plies, halvings, root_selects, improved_rows) -- the plies
        chosen under the option, the halvings performed, the root selects made under the option and the rows recorded
        as the improved policy."""
        return self._stats(self.L.azx_gumbel_stats, self.GUMBEL_STATS)

    def gumbel_state(self):
        """azx_gumbel_state: (candidates, survivors), two uint64[n_games, 3] arrays of bit masks by child index (bit
        c & 63 of word c >> 6) -- the m0 candidates chosen at the top of each slot's last searched ply and the survivors
        left at its end.  Blocking; meant for tests."""
        cand = np.zeros((self.G, 3), np.uint64)
        surv = np.zeros((self.G, 3), np.uint64)
        check(self.L.azx_gumbel_state(self.h, _p(cand, C.c_uint64), _p(surv, C.c_uint64)))
        return cand, surv

    # ---- first-play urgency of the PUCT search (azx_set_fpu; NOT the reference's behaviour) ----
    FPU_MODES = {"off": 0, "absolute": 1, "reduction": 2}

    def set_fpu(self, mode="reduction", value=0.0, reduction=0.25, root_reduction=0.0):
        """azx_set_fpu: first-play urgency.  In EVERY search this engine runs from now on -- search(), the phase API,
        play / play_device / replay_fill / play_steps, and as a side of a Match or Tournament (each engine keeps its own
        setting; they are not refused) -- a child with no visit is scored with Q = fpu instead of Q = 0:
        mode="absolute": fpu = value, in [-1, 1]; mode="reduction": fpu = Qp - r * sqrt(mass), Qp the node's own mean
        value in its mover's view, mass the prior mass of its visited children, r = root_reduction at the search's root
        and reduction below it (include/azx.h has the definition bit for bit, DESIGN 7.20 the interactions).
        mode="off" (or clear_fpu()) is the reference's rule: the same kernels, the same bytes as before.  Forced playouts
        override an argmax computed with FPU; under the Gumbel root search FPU acts below the root only.  The defaults
        (reduction 0.25 below the root, 0 at it) are lc0's / KataGo's customary values as the author recalls them and are
        not checked here.  NOT the reference's behaviour; off by default; outside every parity claim.  Refused
        (AzxError, AZX_ESTATE) between search_begin and the last search_step.  Zeroes fpu_stats().  Its effect on
        playing strength is NOT measured unless profiles/fpu_strength.json says otherwise."""
        if mode not in self.FPU_MODES:
            raise ValueError("fpu: mode must be one of %s, got %r" % (sorted(self.FPU_MODES), mode))
        value, reduction, root_reduction = float(value), float(reduction), float(root_reduction)
        if mode != "off":
            if not -1.0 <= value <= 1.0:                # NaN fails both comparisons
                raise ValueError("fpu: value must be in [-1, 1], got %r" % (value,))
            if not 0.0 <= reduction < float("inf"):
                raise ValueError("fpu: reduction must be finite and >= 0, got %r" % (reduction,))
            if not 0.0 <= root_reduction < float("inf"):
                raise ValueError("fpu: root_reduction must be finite and >= 0, got %r" % (root_reduction,))
        check(self.L.azx_set_fpu(self.h, self.FPU_MODES[mode], value, reduction, root_reduction))

    def clear_fpu(self):
        """set_fpu("off"): an unvisited child scores with Q = 0 again, as in the reference."""
        check(self.L.azx_set_fpu(self.h, 0, 0.0, 0.0, 0.0))

    def fpu(self):
        """azx_get_fpu: dict(mode, value, reduction, root_reduction) in force; mode "off" with zeros when off."""
        if getattr(self.L, "azx_get_fpu", None) is None:        # an older build (tools/lib_bench.py): never set
            return dict(mode="off", value=0.0, reduction=0.0, root_reduction=0.0)
        m, v, r, rr = C.c_int(0), C.c_float(0.0), C.c_float(0.0), C.c_float(0.0)
        check(self.L.azx_get_fpu(self.h, C.byref(m), C.byref(v), C.byref(r), C.byref(rr)))
        name = {n: k for k, n in self.FPU_MODES.items()}[int(m.value)]
        return dict(mode=name, value=float(v.value), reduction=float(r.value), root_reduction=float(rr.value))

    FPU_STATS = ("selects", "levels_with_unvisited", "ended_unvisited", "differs_from_off")

    def fpu_stats(self):
        """azx_fpu_stats since the last set_fpu: dict(selects, levels_with_unvisited, ended_unvisited, differs_from_off)
        -- the selects made under the option, the node levels scored under it that had an unvisited child, the selects
        that ended on a child with no visit; differs_from_off is not computed and always 0 (include/azx.h)."""
        return self._stats(self.L.azx_fpu_stats, self.FPU_STATS)

    # ---- policy temperature of the search's priors (azx_set_policy_temp; NOT the reference's behaviour) ----
    def set_policy_temp(self, eighths, root_eighths):
        """azx_set_policy_temp: a policy temperature of 8 / eighths for the prior rows this engine's searches expand
        from, and of 8 / root_eighths for the priors the root select scores with; both in 1..8, (8, 8) is off.  It holds
        in EVERY search this engine runs from now on -- search(), the phase API, play / play_device / replay_fill /
        play_steps, and as a side of a Match or Tournament (each engine keeps its own setting).  At expansion the
        children's stored prior is temper(row over the legal cells, eighths); at the root PUCT, the noise mix and forced
        playouts read temper(stored priors, root_eighths) while the stored priors stay (include/azx.h has the
        definition bit for bit, DESIGN 7.22 the interactions).  Engines whose evaluator gives one table prior to all
        children (uniform, hash, rollout) are untouched.  (8, 8), or clear_policy_temp(), is the reference's rule: the
        same kernels, the same bytes as before.  NOT the reference's behaviour; off by default; outside every parity
        claim.  Refused (AzxError, AZX_ESTATE) between search_begin and the last search_step.  Zeroes
        policy_temp_stats().  The option has no default setting: both values are given.  (A setting made here directly
        is not known to azalea_amd.policy_temp.apply, which remembers what IT last put on the engine -- as fpu.apply
        does: an engine handed to the policy layers is set through them.)"""
        for name, v in (("eighths", eighths), ("root_eighths", root_eighths)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 8:
                raise ValueError("policy_temp: %s must be an integer in 1..8 (8 is off), got %r" % (name, v))
        check(self.L.azx_set_policy_temp(self.h, int(eighths), int(root_eighths)))

    def clear_policy_temp(self):
        """set_policy_temp(8, 8): the search reads the evaluator's rows as delivered again, as in the reference."""
        check(self.L.azx_set_policy_temp(self.h, 8, 8))

    def policy_temp(self):
        """azx_get_policy_temp: (eighths, root_eighths) as set; (8, 8) when off."""
        if getattr(self.L, "azx_get_policy_temp", None) is None:        # an older build (tools/lib_bench.py): never set
            return (8, 8)
        m, r = C.c_int(8), C.c_int(8)
        check(self.L.azx_get_policy_temp(self.h, C.byref(m), C.byref(r)))
        return int(m.value), int(r.value)

    POLICY_TEMP_STATS = ("tempered", "left_as_delivered", "root_searches", "reserved")

    def policy_temp_stats(self):
        """azx_policy_temp_stats since the last set_policy_temp: dict(tempered, left_as_delivered, root_searches,
        reserved) -- expansions whose row was tempered, rows the guard (or Z == 0) left as delivered at an expansion or
        at a root, searches begun whose root select scores with the tempered priors; reserved is 0 (include/azx.h)."""
        return self._stats(self.L.azx_policy_temp_stats, self.POLICY_TEMP_STATS)

    def resign_values(self):
        """azx_resign_value: float32[n_games], the resign statistic of every slot's current root (NaN where the root
        is unevaluated or unvisited), by the device function the move draw uses."""
        out = np.zeros(self.G, np.float32)
        check(self.L.azx_resign_value(self.h, _p(out, C.c_float)))
        return out


def _collected(out, sink, n_rows, collect):
    """What a collecting Match / Tournament play adds to its result: the rows now in `sink`'s harvest queue."""
    out["n_rows"] = int(n_rows)
    sink._last_rows = int(n_rows)
    if collect is True:
        out["rows"] = sink.rows_read(0, n_rows)
        out["row_metrics"] = sink.play_row_metrics(n_rows)


_KEEP = object()            # play(openings=...) not given: the book stays as set_openings left it


def _book_key(openings):
    """A book as a tuple of move tuples (None = no book = ()): what Match / Tournament remember having set."""
    return tuple(tuple(int(m) for m in o) for o in ([] if openings is None else openings))


def _book_arrays(openings):
    """A list of move lists as the library's opening table: (n, stride, moves int16[n, stride], lengths int32[n])."""
    book = [list(o) for o in _book_key(openings)]
    n = len(book)
    stride = max([1] + [len(o) for o in book])
    mv = np.zeros((max(n, 1), stride), np.int16)
    ln = np.zeros(max(n, 1), np.int32)
    for i, o in enumerate(book):
        if any(m < -32768 or m > 32767 for m in o):
            raise ValueError("opening %d: a move does not fit the int16 of a game record" % i)
        mv[i, :len(o)] = o
        ln[i] = len(o)
    return n, stride, mv, ln


def _book_error(rc):
    """A refused book is the caller's mistake: ValueError with the library's message; anything else as check()."""
    if rc == -1:                # AZX_EINVAL
        raise ValueError(_lib.lib().azx_last_error().decode(errors="replace"))
    check(rc)


def openings_check(board_size, openings):
    """azx_openings_check: ValueError, with the library's message (opening, ply, reason), unless every opening -- a
    list of moves, tile + 1 in play order as in a game record, colour 1 first -- has its moves on the board, plays no
    tile twice and leaves the game undecided after every move.  Host only: no GPU is needed."""
    n, stride, mv, ln = _book_arrays(openings)
    _book_error(_lib.lib().azx_openings_check(int(board_size), n, stride, _p(mv, C.c_int16), _p(ln, C.c_int32), None, None))


def all_openings(board_size, plies=1):
    """Every sequence of `plies` (1 or 2) moves on distinct tiles, in ascending order: n * n openings of one move,
    n * n * (n * n - 1) of two.  Host only.  No position that shallow is decided on a board of size 3 or more; on a
    smaller one filter the list through openings_check."""
    if plies not in (1, 2):
        raise ValueError("plies must be 1 or 2")
    cells = int(board_size) * int(board_size)
    if plies == 1:
        return [[a] for a in range(1, cells + 1)]
    return [[a, b] for a in range(1, cells + 1) for b in range(1, cells + 1) if b != a]


def _opening_index(first_game, n_games, n_openings, first_mover):
    """The opening of games first_game .. first_game + n_games - 1 (the rule of include/azx.h): (u >> 1) % n under the
    alternating first mover, u % n under a fixed one."""
    u = np.arange(int(first_game), int(first_game) + int(n_games), dtype=np.int64)
    return ((u >> 1 if first_mover is None else u) % n_openings).astype(np.int32)


def _refuse_train_targets(engines, what):
    """ValueError for an engine with set_train_targets in force: the harvest of a match or tournament records the
    reference's rows and the outcome (azx_match_play / azx_tournament_play refuse it too, with AZX_EINVAL)."""
    for i, e in enumerate(engines):
        if e.train_targets() != ("reference", 0.0):
            raise ValueError("engine %d has training targets %r set: a %s's harvest records the reference's rows and "
                             "the outcome (clear_train_targets() first)" % (i, e.train_targets(), what))


class _DeviceGames:
    """What Match and Tournament share: a library handle behind the entry points `_PREFIX`* (include/azx.h gives both
    families the same setters), the engines it plays with, and what the library was last told."""
    _PREFIX = None

    def __init__(self, engines, harvest_off):
        self.L = _lib.lib()
        self.engines = list(engines)
        self.h = C.c_void_p()
        self._mode = (harvest_off, -1)    # (harvest / sink, first mover) as set in the library
        self._book = ()                   # the opening book as set in the library (a tuple of move tuples; () = none)

    def _fn(self, name):
        return getattr(self.L, self._PREFIX + name)

    def set_openings(self, openings):
        n, stride, mv, ln = _book_arrays(openings)
        _book_error(self._fn("set_openings")(self.h, n, stride, _p(mv, C.c_int16), _p(ln, C.c_int32)))
        self._book = _book_key(openings)

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _set_modes(self, harvest, first_mover):
        """Harvest (a match: 0 / 1; a tournament: the sink, -1 = off) and first mover, each set only when it changes:
        a plain play touches none of the later entry points of the library."""
        want = (harvest, -1 if first_mover is None else int(first_mover))
        if want[0] != self._mode[0]:
            check(self._fn("set_harvest")(self.h, want[0]))
            self._mode = (want[0], self._mode[1])
        if want[1] != self._mode[1]:
            check(self._fn("set_first_mover")(self.h, want[1]))
        self._mode = want

    def _call(self, fn, *args):
        """check(fn(*args)) for the play calls: what an engine's evaluator raised inside the call surfaces itself,
        chained to the AzxError (Engine._check)."""
        for e in self.engines:
            e._ext_exc = None
        rc = fn(*args)
        exc = next((e._ext_exc for e in self.engines if e._ext_exc is not None), None)
        for e in self.engines:
            e._ext_exc = None
        if rc != 0 and exc is not None:
            try:
                check(rc)
            except AzxError as err:
                raise exc from err
        check(rc)

    def _game_dict(self, outcome, length, mv, stats, first_game, n, first_mover):
        """One pair's result: games first_game .. first_game + n - 1 (`mv`: their records, or None)."""
        out = dict(outcome=outcome, length=length, stats=stats.as_dict())
        if mv is not None:
            out["moves"] = mv
        if self._book:
            out["opening"] = _opening_index(first_game, n, len(self._book), first_mover)
        return out

    def _collect(self, out, sink, collect):
        rows = C.c_int64(0)
        check(self._fn("rows")(self.h, C.byref(rows)))
        _collected(out, sink, rows.value, collect)


class Match(_DeviceGames):
    """azx_match_*: evaluation games between two engines, played entirely on the device.  Agent 0 is `engine_a`,
    agent 1 `engine_b`; game u is first moved by agent u & 1 and both engines draw from their stream seed + u, so
    the games of a call do not depend on the pool size.  The engines stay the caller's (and must stay open while
    the match is); they are reset by every play().  An EVAL_EXTERNAL engine takes part once its evaluator is
    registered (Engine.set_external_evaluator): it is called at every evaluation point with the rows of the slots in
    which its engine is the mover, and an exception it raises is re-raised from play()."""

    _PREFIX = "azx_match_"

    def __init__(self, engine_a, engine_b):
        super().__init__((engine_a, engine_b), 0)
        self.a, self.b = engine_a, engine_b
        self.cells = engine_a.cells
        check(self.L.azx_match_create(engine_a.h, engine_b.h, C.byref(self.h)))

    def set_openings(self, openings):
        """azx_match_set_openings: the following play() calls start game u from opening (u >> 1) % n -- games 2j and
        2j + 1 are one opening with the agents' colours swapped -- or u % n under a fixed first mover.  `openings` is a
        list of move lists (tile + 1 in play order, colour 1 first, [] = the empty board); None or [] clears the book.
        ValueError with the library's message for a book it refuses (openings_check for this board size); the book
        set before stays in place then.  Not in the reference, whose evaluation games all start from the empty
        board; use an even first_game and an even number of games for colour-balanced results."""
        super().set_openings(openings)

    def play(self, n_games, first_game=0, moves=False, collect=False, first_mover=None, openings=_KEEP):
        """Games first_game .. first_game + n_games - 1, each to its end.  Returns outcome int8[n] (+1 agent 0 won,
        -1 agent 1 won, 0 voided by SearchTreeFull), length int16[n] (plies), with `moves` the game records
        int16[n, cells] (tile + 1 in play order, 0-padded), and stats (azx_match_stats as a dict).
        `collect`: harvest the replay rows of every won game -- row p from the agent that moved at ply p, as
        play_game(agents, collect_data=True) records them -- into engine a's harvest queue.  True: the result gains
        "rows" (the dict Engine.play returns; games in the order they settled, a game's rows contiguous with plies
        ascending, game_uid = the game index) and "row_metrics" ([rows, ROW_METRICS], Engine.play_row_metrics);
        "device": the rows stay in engine a's queue for rows_pack / replay_put_records and only their count is
        returned, as "n_rows" (either way).  `first_mover`: None -- agent u & 1 moves first in game u; 0 / 1 -- that
        agent moves first in every game (play_game always starts with agents[0]).
        `openings`: the book to play from, as set_openings takes it (None or [] = none); not given, the book stays
        as it is.  With a book, a record begins with the game's opening, `length` counts it, stats["plies"] does
        not, the rows of a game begin at the opening's length, and the result gains "opening": the opening index of
        each game, int32[n]."""
        if collect not in (False, True, "device"):
            raise ValueError("collect must be False, True or 'device'")
        _refuse_train_targets((self.a, self.b), "match")
        if openings is not _KEEP and _book_key(openings) != self._book:
            self.set_openings(openings)
        self._set_modes(1 if collect else 0, first_mover)
        n = int(n_games)
        outcome = np.zeros(n, np.int8)
        length = np.zeros(n, np.int16)
        mv = np.zeros((n, self.cells), np.int16) if moves else None
        st = MatchStats()
        self._call(self.L.azx_match_play, self.h, int(first_game), n, _p(outcome, C.c_int8), _p(length, C.c_int16),
                   _p(mv, C.c_int16), C.byref(st))
        out = self._game_dict(outcome, length, mv, st, first_game, n, first_mover)
        if collect:
            self._collect(out, self.a, collect)
        return out


class Tournament(_DeviceGames):
    """azx_tournament_*: several matches side by side in ONE ply loop on the device, sharing engines.  `pairs` names
    engines by their index in `engines`; pair s = (i, j) plays, bit for bit, the games of
    Match(engines[i], engines[j]).play(rounds, first_game=first_game + s * rounds) -- engine i is its agent 0 -- while
    every engine searches the slots of all its pairs together.  Every pair gets `tables_per_pair` tables (games in
    flight); an engine that is in d pairs needs n_games >= d * tables_per_pair slots.  The engines stay the caller's,
    as with Match; an exception raised by an engine's external evaluator is re-raised from play()."""

    _PREFIX = "azx_tournament_"

    def __init__(self, engines):
        super().__init__(engines, -1)
        arr = (C.c_void_p * max(len(self.engines), 1))(*[e.h for e in self.engines])
        check(self.L.azx_tournament_create(arr, len(self.engines), C.byref(self.h)))
        self.cells = self.engines[0].cells

    def set_openings(self, openings):
        """azx_tournament_set_openings: as Match.set_openings, for the games of every pair.  The rule is keyed on the
        game index u = first_game + s * rounds + r, so pair s still plays the games of its Match over that range; an
        even first_game and even `rounds` keep every pair colour-balanced."""
        super().set_openings(openings)

    def play(self, pairs, rounds, first_game=0, tables_per_pair=None, moves=False, collect=False, sink=0,
             first_mover=None, openings=_KEEP):
        """`rounds` games of every pair, each to its end.  Returns {pair: dict(outcome int8[rounds], length
        int16[rounds], stats[, moves int16[rounds, cells]])} in the order of `pairs`, each as Match.play returns it
        (stats['seconds'] is the whole call's device time).  tables_per_pair defaults to the most every engine has
        room for, at most `rounds`.
        `collect`, `first_mover`: as Match.play; the rows of ALL pairs go to the harvest queue of engines[sink], and
        the result gains the keys "rows" / "row_metrics" (collect=True) and "n_rows" beside the pairs.  Pair s owns
        the rows with game_uid in [first_game + s * rounds, first_game + (s + 1) * rounds).
        `openings`: as Match.play; with a book every pair's dict gains "opening"."""
        if collect not in (False, True, "device"):
            raise ValueError("collect must be False, True or 'device'")
        _refuse_train_targets(self.engines, "tournament")
        if openings is not _KEEP and _book_key(openings) != self._book:
            self.set_openings(openings)
        self._set_modes(int(sink) if collect else -1, first_mover)
        pairs = [(int(i), int(j)) for i, j in pairs]
        P, rounds = len(pairs), int(rounds)
        if tables_per_pair is None:
            deg = [sum(k in p for p in pairs) for k in range(len(self.engines))]
            room = [e.G // d for e, d in zip(self.engines, deg) if d]
            tables_per_pair = max(1, min([rounds] + room))
        n = max(P * rounds, 0)
        outcome = np.zeros(n, np.int8)
        length = np.zeros(n, np.int16)
        mv = np.zeros((n, self.cells), np.int16) if moves else None
        st = (MatchStats * max(P, 1))()
        pa = np.array([p[0] for p in pairs], np.int32)
        pb = np.array([p[1] for p in pairs], np.int32)
        self._call(self.L.azx_tournament_play, self.h, P, _p(pa, C.c_int32), _p(pb, C.c_int32), int(first_game), rounds,
                   int(tables_per_pair), _p(outcome, C.c_int8), _p(length, C.c_int16), _p(mv, C.c_int16), st)
        out = {}
        for s, pair in enumerate(pairs):
            sl = slice(s * rounds, (s + 1) * rounds)
            out[pair] = self._game_dict(outcome[sl], length[sl], mv[sl] if moves else None, st[s],
                                        int(first_game) + s * rounds, rounds, first_mover)
        if collect:
            self._collect(out, self.engines[int(sink)], collect)
        return out


def tower_choice(board_size, num_blocks, base_chans, flags=0):
    """azx_debug_tower_choice: the `net=` field of kernel_info() of an EVAL_RESNET engine of this shape and these flags
    created now (AZX_TOWER, AZX_HEADS, AZX_TOWER_TILES, AZX_WIDE_STREAMS and AZX_PACK as the environment holds them) --
    which tower and heads kernels it would launch -- from the code the engine itself chooses with, on the host (no GPU
    is needed).  AzxError with the engine's code and message where it would refuse the network."""
    L = _lib.lib()
    buf = C.create_string_buffer(512)
    rc = L.azx_debug_tower_choice(int(board_size), int(num_blocks), int(base_chans), int(flags), buf, len(buf))
    if rc < 0:
        check(rc)
    return buf.value.decode()


def playout_cap_is_full(seed, uid, ply, full_prob):
    """azx_playout_cap_is_full: whether ply `ply` (from the empty board) of game `uid` of an engine created with
    `seed` is a full search under set_playout_cap(full_prob, ...) -- the function the kernels use, on the host (no
    GPU is needed).  ValueError for full_prob outside (0, 1] or a negative ply."""
    L = _lib.lib()
    rc = L.azx_playout_cap_is_full(int(seed) & 0xFFFFFFFFFFFFFFFF, int(uid), int(ply), float(full_prob))
    if rc < 0:
        raise ValueError(L.azx_last_error().decode(errors="replace"))
    return bool(rc)


def selfplay_opening_word(seed, uid):
    """azx_selfplay_opening_word: the 32-bit word game `uid` of an engine created with `seed` draws its opening with
    -- the function the kernels use, on the host (no device call)."""
    out = C.c_uint32(0)
    check(_lib.lib().azx_selfplay_opening_word(int(seed) & 0xFFFFFFFFFFFFFFFF, int(uid), C.byref(out)))
    return int(out.value)


def selfplay_openings_bounds(weights_or_n):
    """azx_selfplay_openings_bounds: uint64[n], the upper bounds of the openings' shares of the 2^32 words -- of `n`
    equally weighted openings (an int) or of the given weights.  ValueError, with the library's message, for weights
    that are negative, non-finite or all zero.  Host only."""
    if isinstance(weights_or_n, (int, np.integer)):
        n, w = int(weights_or_n), None
    else:
        w = np.ascontiguousarray(weights_or_n, np.float64).reshape(-1)
        n = int(w.size)
    ub = np.zeros(max(n, 1), np.uint64)
    _book_error(_lib.lib().azx_selfplay_openings_bounds(n, _p(w, C.c_double), _p(ub, C.c_uint64)))
    return ub[:n]


def selfplay_opening_index(seed, uids, bounds):
    """The opening of each game in `uids` (an int or an array) under `bounds` (selfplay_openings_bounds): the least o
    with selfplay_opening_word(seed, uid) < bounds[o].  Host only."""
    ub = np.asarray(bounds, np.uint64)
    flat = np.atleast_1d(np.asarray(uids, np.int64))
    words = np.array([selfplay_opening_word(seed, int(u)) for u in flat.ravel()], np.uint64)
    idx = np.searchsorted(ub, words, side="right").astype(np.int64).reshape(flat.shape)
    return int(idx[0]) if np.ndim(uids) == 0 else idx


def gumbel_variate(seed, uid, ply, child):
    """azx_gumbel_variate: g = -ln(-ln u) of root child `child` at ply `ply` (from the empty board) of game `uid` of an
    engine created with `seed`, in double precision -- the definition of the Gumbel root search's noise (include/azx.h),
    on the host (no GPU is needed).  ValueError for a negative ply or a child outside [0, 192)."""
    L = _lib.lib()
    g = C.c_double(0.0)
    rc = L.azx_gumbel_variate(int(seed) & 0xFFFFFFFFFFFFFFFF, int(uid), int(ply), int(child), C.byref(g))
    if rc < 0:
        raise ValueError(L.azx_last_error().decode(errors="replace"))
    return float(g.value)


def selftest_gumbel(words, device=0):
    """azx_selftest_gumbel: the device's float32 g of raw Philox words, by the function the tree kernels use."""
    words = np.ascontiguousarray(words, np.uint32)
    out = np.zeros(words.shape, np.float32)
    check(_lib.lib().azx_selftest_gumbel(device, words.size, _p(words, C.c_uint32), _p(out, C.c_float)))
    return out


def fpu_score(mode, nv, tv, prior, nv_p, tv_p, c_puct, is_root=False, value=0.0, reduction=0.25, root_reduction=0.0):
    """azx_fpu_score: the child PUCT takes at ONE node under first-play urgency, on the host (no GPU, no root noise):
    nv, tv, prior are the float32 arrays of its children, (nv_p, tv_p) the node's own visits and total value.  mode
    "off" gives the reference's choice.  The counterpart of Engine.set_fpu for tests and tools."""
    nv, tv, prior = (np.ascontiguousarray(a, np.float32) for a in (nv, tv, prior))
    if not (nv.ndim == 1 and nv.shape == tv.shape == prior.shape):
        raise ValueError("fpu_score: nv, tv and prior must be 1-d arrays of one length")
    if mode not in Engine.FPU_MODES:
        raise ValueError("fpu: mode must be one of %s, got %r" % (sorted(Engine.FPU_MODES), mode))
    out = C.c_int32(-1)
    check(_lib.lib().azx_fpu_score(Engine.FPU_MODES[mode], float(value), float(reduction), float(root_reduction),
                                   1 if is_root else 0, int(nv.size), float(nv_p), float(tv_p), _p(nv, C.c_float),
                                   _p(tv, C.c_float), _p(prior, C.c_float), float(c_puct), C.byref(out)))
    return int(out.value)


def policy_temp_row(eighths, row):
    """azx_policy_temp_row: temper(row, eighths) by the definition (include/azx.h) on the host, no GPU.  row: a 1-d
    float32 array of 1..192 priors.  Returns (out, tempered): the float32 row and whether it was changed (False: eighths
    8, the guard, or Z == 0 -- the row comes back as delivered)."""
    row = np.ascontiguousarray(row, np.float32)
    if row.ndim != 1:
        raise ValueError("policy_temp_row: row must be a 1-d array")
    out = np.empty_like(row)
    flag = C.c_int(0)
    check(_lib.lib().azx_policy_temp_row(int(eighths), int(row.size), _p(row, C.c_float), _p(out, C.c_float),
                                         C.byref(flag)))
    return out, bool(flag.value)


def rollout_value(seed, board, rollouts):
    """azx_rollout_value: the rollout evaluator's definition (include/azx.h) on the host, no GPU.  board: an N x N (or
    flat N*N) array in {0, 1, 2} in the first player's view, the mover being colour 1.  Returns (wins, value)."""
    b = np.ascontiguousarray(board, np.int32).ravel()
    n = int(round(b.size ** 0.5))
    if n * n != b.size:
        raise ValueError("board of %d cells is not square" % b.size)
    wins, value = C.c_int32(0), C.c_float(0.0)
    check(_lib.lib().azx_rollout_value(int(seed) & 0xFFFFFFFFFFFFFFFF, n, _p(b, C.c_int32), int(rollouts),
                                       C.byref(wins), C.byref(value)))
    return wins.value, np.float32(value.value)


def selftest_rollout(boards, rollouts, seed=0, fills=False, device=0):
    """azx_selftest_rollout: the rollout kernel alone on host boards [n, N, N] (or [n, N*N]).  Returns (wins int32 [n],
    value float32 [n], prior float32 [n, cells]) and, with fills=True, the filled boards uint8 [n, min(rollouts, 64),
    cells] of the first rollouts as a fourth entry."""
    b = np.ascontiguousarray(boards, np.int32)
    n = b.shape[0]
    b = b.reshape(n, -1)
    cells = b.shape[1]
    N = int(round(cells ** 0.5))
    if N * N != cells:
        raise ValueError("boards of %d cells are not square" % cells)
    wins = np.zeros(n, np.int32)
    value = np.zeros(n, np.float32)
    prior = np.zeros((n, cells), np.float32)
    f = np.zeros((n, min(max(int(rollouts), 1), 64), cells), np.uint8) if fills else None
    check(_lib.lib().azx_selftest_rollout(device, N, n, _p(b, C.c_int32), int(rollouts), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          _p(wins, C.c_int32), _p(value, C.c_float), _p(prior, C.c_float),
                                          _p(f, C.c_uint8)))
    return (wins, value, prior, f) if fills else (wins, value, prior)


def resign_is_exempt(seed, uid, keep_prob):
    """azx_resign_is_exempt: whether game `uid` of an engine created with `seed` is exempt from resigning under
    set_resign(..., keep_prob=keep_prob) -- the function the kernels use, on the host (no GPU is needed).  ValueError
    for a keep_prob that is not a finite number in [0, 1]."""
    L = _lib.lib()
    rc = L.azx_resign_is_exempt(int(seed) & 0xFFFFFFFFFFFFFFFF, int(uid), float(keep_prob))
    if rc < 0:
        raise ValueError(L.azx_last_error().decode(errors="replace"))
    return bool(rc)


def hex_replay(board_size, moves, lengths, device=0):
    """azx_hex_replay: per-ply result / legal count / empties mask for many move lists."""
    mv = np.ascontiguousarray(moves, np.int32)
    ln = np.ascontiguousarray(lengths, np.int32)
    G, stride = mv.shape
    res = np.zeros((G, stride), np.int32)
    nl = np.zeros((G, stride), np.int32)
    em = np.zeros((G, stride, 4), np.uint64)
    fb = np.zeros((G, board_size, board_size), np.int32)
    check(_lib.lib().azx_hex_replay(device, board_size, G, _p(mv, C.c_int32), _p(ln, C.c_int32),
                                    stride, _p(res, C.c_int32), _p(nl, C.c_int32),
                                    _p(em, C.c_uint64), _p(fb, C.c_int32)))
    return res, nl, em, fb


def random_prefixes(board_size, indices, max_len, seed, device=0):
    """Seeded random legal move prefixes, one per global game index in `indices`, of uniformly drawn
    lengths in [0, max_len] (cut one move short of a win if the random stones happen to finish the game).
    Used to start a pool of concurrent games out of phase (bench.py: a pool that restarts finished games in
    place is, in steady state, spread over all plies -- not lined up on the empty board).  Game i's prefix
    depends on (seed, i) only, so it does not change with the number of ranks.  The rules run on the device
    (azx_hex_replay)."""
    idx = np.asarray(indices, np.int64)
    cells = board_size * board_size
    perms = np.empty((len(idx), cells), np.int32)
    want = np.empty(len(idx), np.int64)
    for j, i in enumerate(idx):
        rng = np.random.RandomState((int(seed) + 0x9E3779B1 * int(i)) % (2 ** 32))
        want[j] = rng.randint(0, max_len + 1)
        perms[j] = rng.permutation(cells) + 1
    res, _, _, _ = hex_replay(board_size, perms, np.full(len(idx), cells, np.int32), device=device)
    won = res != 0
    first_win = np.where(won.any(1), won.argmax(1), cells)      # stones on the board before the winning move
    length = np.minimum(want, first_win)
    return [perms[j, :length[j]].tolist() for j in range(len(idx))]


def selftest_arith(a, b, device=0):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    sq, dv, mul = (np.zeros_like(a) for _ in range(3))
    check(_lib.lib().azx_selftest_arith(device, a.size, _p(a, C.c_float), _p(b, C.c_float),
                                        _p(sq, C.c_float), _p(dv, C.c_float), _p(mul, C.c_float)))
    return sq, dv, mul


def selftest_divide(num, den, device=0):
    """azx_selftest_divide: (num/den through the kernel's unscaled divide, sqrt-table entry of den)."""
    num = np.ascontiguousarray(num, np.float32)
    den = np.ascontiguousarray(den, np.float32)
    q, rt = np.zeros_like(num), np.zeros_like(num)
    check(_lib.lib().azx_selftest_divide(device, len(num), _p(num, C.c_float), _p(den, C.c_float),
                                         _p(q, C.c_float), _p(rt, C.c_float)))
    return q, rt


def selftest_dirichlet(alpha, k, n_rows, seed=1, device=0):
    out = np.zeros((n_rows, k), np.float32)
    check(_lib.lib().azx_selftest_dirichlet(device, float(alpha), k, n_rows, seed, _p(out, C.c_float)))
    return out
