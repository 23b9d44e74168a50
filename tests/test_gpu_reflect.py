"""Random 180-degree reflection of network inputs on the device (AZX_FLAG_RANDOM_REFLECT in the search,
azx_replay_set_reflect in the collate, config["random_reflect"] in train()).  No strength claim: what is held is that
the mechanism is exact -- the evaluator sees a board or its exact reversal, priors come back by ORIGINAL cell, the bit is
a function of (seed, game, ply, request ordinal) only, and with the flag off nothing changes.  The host surface:
tests/test_reflect_api.py.

Run as a program (`python tests/test_gpu_reflect.py child OUT.npz`) this file is the child process of
test_selfplay_does_not_depend_on_the_pipeline: a few self-play moves of a flagged engine, dumped."""
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

TOL = 1e-4                        # the project's bound on value and priors against the torch module
# one asymmetric opening per board (tile + 1, X first): its first six moves leave X to move, all seven O
PREFIX = {7: [1, 2, 9, 4, 16, 11, 23], 13: [1, 2, 15, 4, 28, 17, 45]}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def seeded_net(n, blocks, chans, seed):
    from azalea_amd.network import HexNetwork
    torch.manual_seed(seed)
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.6, 1.4)
    return net


def net_input(n, moves):
    """The unreflected network input of the position after `moves`, by the host rules (mcts.py:178-181)."""
    from azalea_amd.game.hex import HexGame
    g = HexGame(n)
    for m in moves:
        g.step(m)
    st = g.state
    board, legal = st.board[None].astype(np.int32), st.legal_moves[None].astype(np.int32)
    if st.color == 1:
        board, legal = HexGame.flip_player_board_moves(board, legal)
    return board[0], legal[0]


def turned_list(lm, cells):
    return np.where(lm > 0, cells + 1 - lm, 0).astype(lm.dtype)


def torch_eval(net, boards, lm):
    with torch.no_grad():
        out = net(torch.tensor(boards), torch.tensor(lm))
    return out["value"].numpy(), np.exp(out["moves_logprob"].numpy())


@pytest.mark.parametrize("n,blocks,chans,net_seed", [(7, 1, 64, 32), (13, 1, 32, 11)])
def test_evaluation_tape(n, blocks, chans, net_seed):
    """4(a)-(f): 7x7 1x64 runs k_tower_f16x3_s16 + k_heads_mfma, 13x13 1x32 k_tower_mfma<32> + k_heads (three cell
    slots).  The flag-off engine B is fed A's evaluations (azx_put_evals) so that both build the same trees and B's
    rows are the unreflected rows of A's leaves."""
    from azalea_amd import engine as eng
    cells, G = n * n, 512
    net = seeded_net(n, blocks, chans, net_seed)
    state = {k: v.detach().numpy() for k, v in net.state_dict().items() if v.dtype.is_floating_point}
    prefixes = [PREFIX[n][:6 + (g & 1)] for g in range(G)]
    kw = dict(board_size=n, n_games=G, simulations=16, search_batch_size=8, exploration_coef=0.5, exploration_depth=0,
              noise_alpha=0.03, noise_scale=0.0, temperature=0.0, evaluator=eng.EVAL_RESNET, num_blocks=blocks,
              base_chans=chans, seed=777)
    A = eng.Engine(flags=eng.FLAG_RANDOM_REFLECT, **kw)
    B = eng.Engine(**kw)
    info = A.kernel_info()
    assert "reflect=on" in info and "reflect=off" in B.kernel_info()
    assert ("k_heads_mfma" in info) == (n == 7), info
    for E in (A, B):
        E.set_weights(state)
        E.reset(moves=prefixes)
    want_root = [net_input(n, PREFIX[n][:6]), net_input(n, PREFIX[n][:7])]
    assert A.search_begin() == G and B.search_begin() == G
    total = reversed_rows = 0
    told_apart = 0.0
    for point in range(3):
        ba, la, sa, ka = A.get_leaves()
        va, pa = A.get_evals()
        bb, lb, sb, kb = B.get_leaves()
        assert len(ka) == len(kb) > 0 and np.array_equal(sa, sb) and np.array_equal(ka, kb)
        fa, fb = ba.reshape(len(ka), cells), bb.reshape(len(kb), cells)
        assert (fb != fb[:, ::-1]).any(1).all()                   # no position here is its own reversal
        rev = (fa != fb).any(1)
        # (a) the board or its index reversal; (b) the legal row t, or cells + 1 - t on exactly those rows
        assert np.array_equal(fa[~rev], fb[~rev]) and np.array_equal(fa[rev], fb[rev][:, ::-1])
        assert np.array_equal(la[~rev], lb[~rev]) and np.array_equal(la[rev], turned_list(lb[rev], cells))
        if point == 0:                                            # root rows: known from the prefix
            assert np.array_equal(sa, np.arange(G))
            for g in range(G):
                wb, wl = want_root[g & 1]
                assert np.array_equal(bb[g], wb) and np.array_equal(lb[g, :kb[g]], wl), g     # (f), flag off
        kmax = int(ka.max())
        legal = la[:, :kmax] > 0
        assert np.array_equal(legal.sum(1), ka) and not la[:, kmax:].any()
        # (c) the torch module on the rows as handed out
        tv, tp = torch_eval(net, ba, la[:, :kmax])
        dv, dp = np.abs(va - tv).max(), np.abs(pa[:, :kmax] - tp)[legal].max()
        print("n=%d point %d: %d rows, %d reversed, |dv| %.2e |dp| %.2e" % (n, point, len(ka), rev.sum(), dv, dp))
        assert dv <= TOL and dp <= TOL
        # (f) B's rows, deeper ones included, are unreflected rows in their own right: B's own device evaluations
        # of them agree with the torch module on them (B has not been fed A's evaluations of this point yet)
        vb, pb = B.get_evals()
        tv_plain, tp_plain = torch_eval(net, bb, lb[:, :kmax])
        assert np.array_equal(lb[:, :kmax] > 0, legal)
        assert np.abs(vb - tv_plain).max() <= TOL and np.abs(pb[:, :kmax] - tp_plain)[legal].max() <= TOL
        told_apart = max(told_apart, float(np.abs(tp[rev] - tp_plain[rev])[legal[rev]].max()))
        # B continues with A's evaluations: the same trees in both engines
        B.put_evals(va, pa)
        na, done_a = A.search_step()
        nb, done_b = B.search_step()
        assert na == nb and not done_a and not done_b
        if point == 0:                                            # (d) the APPLY wrote the tape's root priors
            for E in (A, B):
                root = E.get_root()
                assert np.array_equal(root["k"], ka)
                for g in range(G):
                    assert np.array_equal(bits(root["child_prior"][g, :ka[g]]), bits(pa[g, :ka[g]])), g
        total += len(ka)
        reversed_rows += int(rev.sum())
    # (c) the check above can tell the two candidates apart
    assert told_apart > 1e-2, told_apart
    # (e) a fair bit
    assert total >= 2000
    share = reversed_rows / total
    print("n=%d: %d of %d requests reversed (%.4f)" % (n, reversed_rows, total, share))
    assert abs(share - 0.5) <= 5 * 0.5 / np.sqrt(total), (reversed_rows, total)
    A.close()
    B.close()


def table_evaluator(cells, invariant, seed=9):
    """value = ((sum over cells of h[i(c)][colour]) mod 65536) / 32768 - 1, prior_j = w_j / sum w with w_j = u[i(t_j)]
    in 1..16, i(c) = min(c, cells - 1 - c) -- exact integer arithmetic, so invariant under the 180-degree turn bit for
    bit -- or i(c) = c: not invariant."""
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(seed)
    h = torch.tensor(rng.randint(0, 1 << 20, (cells, 3)), dtype=torch.int64, device=dev)
    u = torch.tensor(rng.randint(1, 17, cells), dtype=torch.int64, device=dev)
    c = torch.arange(cells, device=dev)
    idx = torch.minimum(c, cells - 1 - c) if invariant else c

    def evaluate(board, legal):
        b = board.reshape(len(board), cells).to(torch.int64)
        s = h[idx[None, :].expand_as(b), b].sum(1)
        value = ((s % 65536).to(torch.float64) / 32768.0 - 1.0).to(torch.float32)
        t = (legal.to(torch.int64) - 1).clamp(min=0)
        w = torch.where(legal > 0, u[idx[t]], torch.zeros((), dtype=torch.int64, device=dev))
        prior = w.to(torch.float32) / w.sum(1, keepdim=True).to(torch.float32)
        return value, prior
    return evaluate


def external_engine(n, G, flag, invariant):
    from azalea_amd import engine as eng
    E = eng.Engine(board_size=n, n_games=G, simulations=20, search_batch_size=5, exploration_coef=0.5,
                   exploration_depth=6, noise_alpha=0.03, noise_scale=0.25, temperature=1.0, seed=12345,
                   evaluator=eng.EVAL_EXTERNAL, flags=eng.FLAG_RANDOM_REFLECT if flag else 0)
    E.set_external_evaluator(table_evaluator(n * n, invariant))
    return E


def snapshot(E):
    games, root = E.get_games(), E.get_root()
    out = {"game_" + k: v for k, v in games.items()}
    out.update({"root_" + k: v for k, v in root.items()})
    for g in range(E.G):
        for k, v in E.tree_dump(g).items():
            out["tree%d_%s" % (g, k)] = np.asarray(v)
    out["counters"] = E.debug_counters()[:10]
    return out


def same(a, b):
    return set(a) == set(b) and all(
        np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                       b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]) for k in a)


@pytest.mark.parametrize("n", [7, 13])
def test_invariant_evaluator_plays_the_same_games(n):
    """5: with an evaluator that is exactly invariant under the turn, and device noise ON, the flag changes nothing
    -- export, import and the separate RNG stream are right end to end; with the invariance dropped it does."""
    G = 64
    shots = {}
    for flag in (False, True):
        E = external_engine(n, G, flag, invariant=True)
        st = E.play_steps(4)
        assert st["plies"] == 4 * G and st["evals"] > 0
        shots[flag] = snapshot(E)
        if n == 7:                                   # ... and whole games: every 7x7 game ends within 49 plies
            rows, st = E.play(50000, max_plies=49)
            assert len(rows["reward"]) > 0
            order = np.argsort(rows["game_uid"], kind="stable")
            shots[flag].update({"rows_" + k: np.asarray(v)[order] for k, v in rows.items()})
            shots[flag]["row_metrics"] = E.play_row_metrics()[order]
        E.close()
    assert same(shots[False], shots[True])
    boards = {}
    for flag in (False, True):
        E = external_engine(n, G, flag, invariant=False)
        E.play_steps(4)
        boards[flag] = snapshot(E)
        E.close()
    assert not same(boards[False], boards[True])


def test_match_does_not_depend_on_the_pool_size():
    """6a: the check of tests/test_gpu_match.py on two flagged engines with the seeded 1x64 device networks."""
    import test_gpu_match as tgm
    from azalea_amd import engine as eng
    n, n_games, first_game = 7, 128, 1000
    res = {}
    for G in (64, 256):
        a = tgm.make_engine(eng, n, G, tgm.AGENT_A, 11, "net", net_seed=3, flags=eng.FLAG_RANDOM_REFLECT)
        b = tgm.make_engine(eng, n, G, tgm.AGENT_B, 1 << 40, "net", net_seed=4, flags=eng.FLAG_RANDOM_REFLECT)
        assert "reflect=on" in a.kernel_info() and "reflect=on" in b.kernel_info()
        m = eng.Match(a, b)
        res[G] = m.play(n_games, first_game=first_game, moves=True)
        m.close()
        a.close()
        b.close()
    for k in ("outcome", "length", "moves"):
        assert np.array_equal(res[64][k], res[256][k]), k
    tgm.check_games(res[64], n, n_games, first_game)


def child(out):
    """Three self-play moves of a flagged 7x7 1x64 engine at the smallest pool the two-half-pool loop takes."""
    from azalea_amd import engine as eng
    n, G = 7, 1024
    net = seeded_net(n, 1, 64, 3)
    E = eng.Engine(board_size=n, n_games=G, simulations=20, search_batch_size=5, exploration_coef=0.5,
                   exploration_depth=6, noise_alpha=0.03, noise_scale=0.25, temperature=1.0, seed=4242,
                   evaluator=eng.EVAL_RESNET, num_blocks=1, base_chans=64, flags=eng.FLAG_RANDOM_REFLECT)
    E.set_weights({k: v.detach().numpy() for k, v in net.state_dict().items() if v.dtype.is_floating_point})
    st = E.play_steps(3)
    games, root = E.get_games(), E.get_root()
    dump = {"game_" + k: v for k, v in games.items()}
    dump.update({"root_" + k: v for k, v in root.items()})
    dump["counters"] = E.debug_counters()[:10]
    dump["plies"] = np.array([st["plies"]])
    np.savez(out, info=np.array(E.kernel_info()), **dump)
    E.close()


def test_selfplay_does_not_depend_on_the_pipeline(tmp_path):
    """6b: AZX_PIPELINE=0 and =1 in fresh child processes, as tests/test_gpu_pipeline.py does."""
    dumps = {}
    for pipeline in (0, 1):
        out = str(tmp_path / ("pipe%d.npz" % pipeline))
        env = dict(os.environ, AZX_PIPELINE=str(pipeline))
        cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "child", out]
        r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=150)
        assert r.returncode == 0, (pipeline, r.returncode, r.stderr.decode()[-2000:])
        dumps[pipeline] = dict(np.load(out))
    info0, info1 = str(dumps[0].pop("info")), str(dumps[1].pop("info"))
    assert "one stream" in info0 and "reflect=on" in info0
    assert "two half-pools on two streams" in info1 and "reflect=on" in info1
    assert int(dumps[0]["plies"][0]) == 3 * 1024 and (dumps[0]["game_ply"] > 0).all()
    assert same(dumps[0], dumps[1])


def test_inline_evaluators_refuse_the_flag():
    """7"""
    from azalea_amd import engine as eng
    from azalea_amd._lib import AzxError
    for ev in (eng.EVAL_UNIFORM, eng.EVAL_UNIFORM_HASH):
        with pytest.raises(AzxError, match=r"azx error -1.*evaluator"):
            eng.Engine(board_size=7, n_games=4, evaluator=ev, flags=eng.FLAG_RANDOM_REFLECT)
        eng.Engine(board_size=7, n_games=4, evaluator=ev).close()         # without it: as before


def host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items()}


def row_bits(plain, seen, cells):
    """Per row: 0 = `seen` is the plain row, 1 = its 180-degree turn (section 2 of the transform); anything else fails."""
    B = len(plain["reward"])
    pb, sb = plain["board"].reshape(B, cells), seen["board"].reshape(B, cells)
    for k in ("color", "reward", "result", "moves_prob"):
        assert np.array_equal(seen[k], plain[k]), k
    assert seen["legal_moves"].shape == plain["legal_moves"].shape
    rot = np.zeros(B, bool)
    for i in range(B):
        if np.array_equal(sb[i], pb[i]) and np.array_equal(seen["legal_moves"][i], plain["legal_moves"][i]):
            continue
        assert np.array_equal(sb[i], pb[i][::-1]), i
        assert np.array_equal(seen["legal_moves"][i], turned_list(plain["legal_moves"][i], cells)), i
        rot[i] = True
    return rot


@pytest.mark.parametrize("n", [5, 13])
def test_collate(n):
    """8"""
    from azalea_amd import engine as eng
    from azalea_amd.device_replay import DeviceReplayBuffer
    from azalea_amd.prep import rot180_batch
    cells = n * n
    E = eng.Engine(board_size=n, n_games=16, simulations=20, search_batch_size=10, evaluator=eng.EVAL_UNIFORM,
                   noise_scale=0.25, temperature=1.0, exploration_depth=15, seed=99)
    buf = DeviceReplayBuffer(E, 4096)
    buf.consume(150)
    rows = len(buf)
    assert rows >= 300
    rng = np.random.RandomState(n)
    idx = rng.randint(0, rows, 256)
    idx2 = rng.randint(0, rows, 256)
    plain, plain2 = host(buf.sample(idx)), host(buf.sample(idx2))
    # (every row shows its bit: even a board that is its own reversal has its ascending legal list turned)
    assert not buf.random_reflect
    buf.reflect_seed = 5
    buf.random_reflect = True
    assert buf.random_reflect
    calls = [row_bits(plain, host(buf.sample(idx)), cells) for _ in range(9)]
    seen_n = sum(len(c) for c in calls)
    seen_rot = sum(int(c.sum()) for c in calls)
    assert seen_n >= 2000
    print("n=%d: %d of %d rows turned (%.4f)" % (n, seen_rot, seen_n, seen_rot / seen_n))
    assert abs(seen_rot / seen_n - 0.5) <= 5 * 0.5 / np.sqrt(seen_n)
    assert not np.array_equal(calls[0], calls[1])                 # the collate count is part of the key
    # the same seed and call count give the same bits whatever the indices; another seed does not
    buf.random_reflect = True
    again = [row_bits(plain2, host(buf.sample(idx2)), cells) for _ in range(3)]
    for c, a in zip(calls, again):
        assert np.array_equal(c, a)
    kept = buf.state_dict()["rows"]                               # checkpoints hold the ring's rows, unturned
    assert buf.random_reflect
    assert np.array_equal(np.asarray(kept["board"]).reshape(rows, cells)[idx], plain["board"].reshape(256, cells))
    buf.reflect_seed = 6
    buf.random_reflect = True
    other = row_bits(plain, host(buf.sample(idx)), cells)
    assert not np.array_equal(other, calls[0])
    # collate_async = the blocking call (same seed, same count)
    dev = buf.device
    out = dict(color=torch.empty(256, dtype=torch.int64, device=dev),
               legal_moves=torch.empty((256, cells), dtype=torch.int32, device=dev),
               result=torch.empty(256, dtype=torch.int64, device=dev),
               board=torch.empty((256, cells), dtype=torch.int32, device=dev),
               moves_prob=torch.empty((256, cells), dtype=torch.float32, device=dev),
               reward=torch.empty(256, dtype=torch.float32, device=dev))
    full = {k: torch.empty_like(v) for k, v in out.items()}
    buf.reflect_seed = 5
    buf.random_reflect = True
    buf.collate_into(idx, full)
    buf.random_reflect = True
    buf.collate_async(idx, out)
    torch.cuda.synchronize()
    for k in out:
        assert torch.equal(out[k], full[k]), k
    assert np.array_equal(row_bits(plain, {k: (v[:, :plain[k].shape[1]] if k in ("legal_moves", "moves_prob") else v)
                                           for k, v in host(full).items()}, cells), calls[0])
    # with the mover view as well: view first, then the turn (prep.rot180_batch is the host twin)
    buf.random_reflect = False
    buf.mover_view = True
    view = buf.sample(idx)
    buf.random_reflect = True
    seen = buf.sample(idx)
    want = rot180_batch(view, torch.as_tensor(calls[0]))
    second = plain["color"] == 1
    assert (second & calls[0]).any() and (second & ~calls[0]).any()
    for k in want:
        assert torch.equal(seen[k], want[k]), k
    # off again: the parent's bytes
    buf.random_reflect = False
    buf.mover_view = False
    back = host(buf.sample(idx))
    for k in plain:
        assert np.array_equal(back[k], plain[k]), k
    E.close()


class LossLog(logging.Handler):
    def __init__(self):
        super().__init__(logging.INFO)
        self.losses, self.lines = [], []

    def emit(self, record):
        if isinstance(record.msg, str):
            if record.msg.startswith("step %d loss"):
                self.losses.append(float(record.args[1]))
            self.lines.append(record.getMessage())


@pytest.mark.parametrize("device_replay", [True, False])
def test_train_smoke(tmp_path, monkeypatch, device_replay):
    """9: a handful of steps on 5x5, 1x16 with config["random_reflect"]."""
    from azalea_amd.parallel_player import Player
    from azalea_amd.policy import Policy
    from azalea_amd.policy_trainer import train
    torch.manual_seed(1)
    policy = Policy()
    policy.initialize(dict(device="cuda:0", network="HexNetwork", board_size=5, num_blocks=1, base_chans=16,
                           simulations=20, search_batch_size=5, exploration_coef=1.0, exploration_depth=4,
                           exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0,
                           seed=1))
    config = dict(seed=1, device="cuda:0", game="azalea_amd.game.hex.HexGame", board_size=5, replaybuf_size=256,
                  replaybuf_oversampling=1.0, batch_size=64, lr_initial=0.05, lr_decay=0.1, lr_decay_epochs=1,
                  momentum=0.9, l2_regularization=1e-4, total_epochs=2, selfplay_games=64, log_interval=1,
                  model_checkpoint_interval=0, random_reflect=True)
    log = LossLog()
    root = logging.getLogger()
    level = root.level
    root.addHandler(log)
    root.setLevel(logging.INFO)
    infos = []
    stop = Player.stop

    def stop_and_tell(player):                  # train() stops its player at the end: ask its engine first
        if player.random_reflect:               # (not the random-mover player that fills the first buffer)
            infos.append(player.device_engine().kernel_info())
        stop(player)
    monkeypatch.setattr(Player, "stop", stop_and_tell)
    try:
        path = train(policy, config, str(tmp_path), device_replay=device_replay)
    finally:
        root.removeHandler(log)
        root.setLevel(level)
    assert os.path.exists(path)
    assert len(log.losses) >= 4 and np.isfinite(log.losses).all(), log.losses
    assert len(infos) == 1 and "reflect=on" in infos[0], infos
    said = [l for l in log.lines if "random_reflect" in l]
    assert len(said) == 1 and ("collate kernel" if device_replay else "rot180_batch") in said[0], said


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "child":
        child(sys.argv[2])
    else:
        raise SystemExit("usage: test_gpu_reflect.py child OUT.npz")
