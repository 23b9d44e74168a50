"""What the hand-written training step (csrc/train_kernels.hip) does with a gradient once it has one -- the part that
moves the weights on every step of a run, which test_gpu_native_train.py sees only at lr = 0 or through 2e-4 / 2e-2
bounds:

  * the SGD update of every segment kind of k_trn_update (SEG_PLAIN, SEG_CONV, SEG_BNW, SEG_BNB, SEG_HCONV, SEG_W1,
    SEG_EMB) and of k_tw_update_conv, element by element against float64 (tests/sgd_reference.py: a few fp32 roundings),
    from non-zero momentum buffers, with lr, momentum and weight decay all at work and changing between two steps;
  * the gradient the update used is that of the weights at the START of the step (conv1.weight and encoder.weight are
    each other's factor and move in the same launch), the BatchNorm running statistics from non-default values;
  * the hyper-parameter ring past its wrap (2 x 256 + 44 steps, new values every step, the host never waiting);
  * all of it, and the gradient tests of test_gpu_native_train.py, under AZX_TRAIN_GRAPH=1 and AZX_TRAIN_FORK=0 -- each
    test reads the mode back through debug("flags"), so none of them can silently run the default path;
  * NativeTrainStep.step_from_ring against step() on the same rows.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_native_train as T
from sgd_reference import EPS, expected
from test_gpu_native_train import DEV, _net, _random_batch

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "graph": {"AZX_TRAIN_GRAPH": "1"}, "nofork": {"AZX_TRAIN_FORK": "0"},
         "graph+nofork": {"AZX_TRAIN_GRAPH": "1", "AZX_TRAIN_FORK": "0"}}


def _set_mode(monkeypatch, mode):
    """The trainer reads both switches when it is created; returns the (use_graph, fork) it must then report."""
    for name in ("AZX_TRAIN_GRAPH", "AZX_TRAIN_FORK"):
        monkeypatch.delenv(name, raising=False)
    for name, value in MODES[mode].items():
        monkeypatch.setenv(name, value)
    return (1 if "graph" in mode else 0, 0 if "nofork" in mode else 1)


def _flags(step):
    f = step.debug("flags")
    assert f.dtype == np.int32 and f.shape == (3,), f
    return tuple(int(x) for x in f)


def _f32(x):
    """A hyper-parameter as the step receives it (azx_train_step takes floats)."""
    return float(np.float32(x))


def _is_wide(n, chans):
    return chans >= 128 or (chans == 64 and n >= 12)


def _kind(name, wide):
    """The update path of a parameter (train_kernels.hip, azx_trn_bind)."""
    if name == "encoder.weight":
        return "SEG_EMB"
    if name == "conv1.weight":
        return "SEG_W1"
    if name.startswith("resblocks.") and ".conv" in name:
        return "k_tw_update_conv" if wide else "SEG_CONV"
    if name in ("value_conv1.weight", "move_conv1.weight"):
        return "SEG_HCONV"
    if "bn" in name:
        return "SEG_BNW" if name.endswith("weight") else "SEG_BNB"
    return "SEG_PLAIN"


def _batch(n, B, seed):
    """_random_batch with one row's moves_prob rescaled to sum 0.7 and one row's all zero: the softmax term of
    dL/dlogit is weighted by the row's sum, which is 1 in every other batch of the suite."""
    batch = _random_batch(n, B, seed)
    mp = batch["moves_prob"]
    sums = mp.sum(1)
    a = int(torch.argmax(sums))                     # a row that has legal moves (on 2x2 a board may be full)
    mp[a] *= 0.7 / float(sums[a])
    mp[(a + 1) % B] = 0.0
    return {k: v.to(DEV) for k, v in batch.items()}


def _preset(net, opt, seed):
    """Non-zero momentum buffers (0.01 randn) and BatchNorm statistics away from torch's (0, 1, 0)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            opt.state[p]["momentum_buffer"] = (0.01 * torch.randn(p.shape, generator=g)).to(DEV)
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.2 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.3 + 1.4 * torch.rand(mod.running_var.shape, generator=g))
                mod.num_batches_tracked.fill_(5)


def _autograd(state, batch, n, blocks, chans, dtype):
    """Train-mode forward + backward of the reference loss at `state` (a state_dict): parameter gradients (float64,
    flat) and the BatchNorm buffers after the forward."""
    from azalea_amd.network import HexNetwork
    net = HexNetwork(board_size=n, num_blocks=blocks, base_chans=chans).to(DEV).to(dtype)
    net.load_state_dict(state)
    net.train()
    B = len(batch["reward"])
    o = net.forward(batch["board"], batch["legal_moves"])
    loss = F.mse_loss(o["value"], batch["reward"].to(dtype)) - (batch["moves_prob"].to(dtype) * o["moves_logprob"]).sum() / B
    loss.backward()
    grads = {name: p.grad.double().cpu().numpy().ravel() for name, p in net.named_parameters()}
    params = dict(net.named_parameters())
    bufs = {name: t.detach().cpu().numpy() for name, t in net.state_dict().items() if name not in params}
    return grads, bufs


_FIRST_STEP = {}      # (n, blocks, chans, B) -> the start state and autograd's answers for the first step (shared, read-only)


def _reference(key, s, state0, batch):
    """Autograd in fp32 and fp64 at the start-of-step state.  The first step starts from the same seeded state under
    every triple and every switch: computed once per shape."""
    if s == 0 and key in _FIRST_STEP:
        kept, ref = _FIRST_STEP[key]
        for name, t in state0.items():
            assert torch.equal(t.cpu(), kept[name]), "the first step's start state is not what the shared reference saw: " + name
        return ref
    ref = (_autograd(state0, batch, *key[:3], torch.float32)[0],) + _autograd(state0, batch, *key[:3], torch.float64)
    if s == 0:
        _FIRST_STEP[key] = ({name: t.cpu().clone() for name, t in state0.items()}, ref)
    return ref


def _ratio(diff, tol):
    """max |diff| / tol; a zero bound demands equality."""
    diff, tol = np.abs(diff), np.asarray(tol)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, diff / tol, np.where(diff > 0, np.inf, 0.0))
    i = int(np.argmax(r))
    return float(r[i]), i


def _close(a, b, tol, what):          # test_gpu_native_train.py's `close`
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max()) / scale
    assert err <= tol, "%s: %.3g (scale %.3g)" % (what, err, scale)


def _update_case(n, blocks, chans, B, triples, want_flags):
    from azalea_amd.native_train import NativeTrainStep
    key, wide = (n, blocks, chans, B), _is_wide(n, chans)
    net = _net(n, blocks, chans, seed=9).train()
    opt = torch.optim.SGD(net.parameters(), lr=triples[0][0], momentum=triples[0][1], weight_decay=triples[0][2])
    _preset(net, opt, 77)
    step = NativeTrainStep(net, opt, B, DEV)
    assert _flags(step) == want_flags + (0,)
    names = [name for name, _ in net.named_parameters()]
    moms = {name: opt.state[p]["momentum_buffer"] for name, p in net.named_parameters()}
    worst = {}
    for s, (lr, mu, wd) in enumerate(triples):
        pg = opt.param_groups[0]
        pg["lr"], pg["momentum"], pg["weight_decay"] = lr, mu, wd
        batch = _batch(n, B, 41 + s)
        state0 = {name: t.clone() for name, t in net.state_dict().items()}
        mom0 = {name: m.clone() for name, m in moms.items()}
        step.step(batch)
        torch.cuda.synchronize()
        assert _flags(step) == want_flags + (want_flags[0],)          # graph mode: instantiated by the first step, replayed by the second
        g32, g64, bn64 = _reference(key, s, state0, batch)
        state1 = net.state_dict()
        failures = []
        for name in names:
            kind = _kind(name, wide)
            g = step.debug("grad:" + name)           # the value the update used: the kernel files it there
            # (a) the update, element by element
            m1, p1, tol_m, tol_p = expected(state0[name].cpu().numpy().ravel(), mom0[name].cpu().numpy().ravel(), g,
                                            _f32(lr), _f32(mu), _f32(wd))
            rm, im = _ratio(moms[name].cpu().numpy().ravel().astype(np.float64) - m1, tol_m)
            rp, ip = _ratio(state1[name].cpu().numpy().ravel().astype(np.float64) - p1, tol_p)
            w = worst.setdefault(kind, [0.0, 0.0])
            w[0], w[1] = max(w[0], rm), max(w[1], rp)
            if rm > 1.0:
                failures.append("step %d %s [%s]: momentum %.3g x tol_m at element %d" % (s, name, kind, rm, im))
            if rp > 1.0:
                failures.append("step %d %s [%s]: parameter %.3g x tol_p at element %d" % (s, name, kind, rp, ip))
            # (b) that gradient is the one of the start-of-step weights: test_odd_batches_and_boards' criterion
            truth = g64[name]
            nt = float(np.linalg.norm(truth))
            e_torch = float(np.linalg.norm(g32[name] - truth))
            e_native = float(np.linalg.norm(g.astype(np.float64) - truth))
            tol = 5e-3 if B * n * n * chans > 200000 else 2e-5
            if not e_native <= max(5.0 * e_torch, tol * nt, 1e-12):
                failures.append("step %d %s [%s]: gradient %.3g from float64 (torch fp32 %.3g, norm %.3g)" % (s, name, kind, e_native, e_torch, nt))
        print("update %s step %d (%g, %g, %g) worst ratio to (tol_m, tol_p): %s"
              % (key, s, lr, mu, wd, ", ".join("%s %.2f %.2f" % (k, v[0], v[1]) for k, v in sorted(worst.items()))))
        assert not failures, "\n".join(failures)
        # (c) BatchNorm statistics: 0.9 old + 0.1 batch (unbiased variance), from the float64 forward at the same state
        for name, want in bn64.items():
            if name.endswith("num_batches_tracked"):
                assert int(state1[name]) == 5 + s + 1 == int(want), name
            else:
                _close(state1[name].cpu().numpy(), want, 2e-5, "step %d %s" % (s, name))
    assert step.steps == len(triples)
    step.close()


TWO_STEPS = {"two": [(0.3, 0.5, 0.1), (0.05, 0.9, 1e-4)], "mu0": [(0.3, 0.0, 0.1), (0.05, 0.9, 1e-4)]}


@pytest.mark.parametrize("variant", ["two", "mu0"])
@pytest.mark.parametrize("n,blocks,chans,B", [(5, 1, 16, 4), (7, 2, 32, 11),     # narrow SEG_CONV
                                              (2, 1, 64, 70),                     # ... with G at its cap of 64, B > 64
                                              (3, 1, 128, 11),                    # k_tw_update_conv, G = 11: one round of eight copies + three
                                              (4, 1, 256, 3), (12, 1, 64, 9)])    # ... at 256 channels; 64 channels through the wide step
def test_update_is_sgd_element_by_element(monkeypatch, n, blocks, chans, B, variant):
    """Two consecutive steps with different (lr, momentum, weight decay) from preset momentum buffers and BatchNorm
    statistics: (a) every element of every parameter and momentum buffer within tol_m / tol_p (sgd_reference.py) of
    float64 SGD on the gradient the update used, (b) that gradient held to float64 autograd at the start-of-step
    weights, (c) running_mean / running_var / num_batches_tracked.  'mu0': the first step at momentum 0."""
    _update_case(n, blocks, chans, B, TWO_STEPS[variant], _set_mode(monkeypatch, "default"))


@pytest.mark.parametrize("mode", ["graph", "nofork", "graph+nofork"])
@pytest.mark.parametrize("n,blocks,chans,B", [(5, 1, 16, 4), (3, 1, 128, 11), (12, 1, 64, 9)])
def test_update_under_graph_and_inline_modes(monkeypatch, n, blocks, chans, B, mode):
    """The same under AZX_TRAIN_GRAPH=1 (the second step is a replay of the captured graph with new hyper-parameters
    and a new batch), AZX_TRAIN_FORK=0 (filter gradients and their update in line) and both."""
    _update_case(n, blocks, chans, B, TWO_STEPS["two"], _set_mode(monkeypatch, mode))


RING_STEPS = 2 * 256 + 44


@pytest.mark.parametrize("mode", ["default", "graph", "nofork"])
def test_hyper_parameter_ring_past_its_wrap(monkeypatch, mode):
    """556 steps of the smallest network (2x2, 1x16, three boards) with new (lr, momentum, weight decay) on every step
    -- cycles of 7, 3 and 2: a slot off by one, or by half a ring of TRN_HP_SLOTS = 256, holds other values -- and
    nothing in the loop that waits for the device (stream-ordered snapshots only): the host queues ahead as far as the
    runtime lets it.  (Measured with the device held back by 170 ms of matrix products: the HIP runtime stalls a launch
    once about a thousand kernels are pending -- 22 .. 26 of these steps, graphed or not --, long before the ring's
    half-ring wait of 128 steps could bind; so no head start is staged here.)  Every step's slot is identified
    afterwards: lr from p_i - p_{i-1} = -lr_i m_i on four tensors, momentum and weight decay from
    m_i = mu_i m_{i-1} + wd_i p_{i-1} on entries whose gradient is exactly zero (cell 0 is occupied on every board:
    move_fc's row 0 never gets a gradient)."""
    from azalea_amd.native_train import NativeTrainStep
    want_flags = _set_mode(monkeypatch, mode)
    n, blocks, chans, B = 2, 1, 16, 3
    cells = n * n
    board = np.array([[[1, 0], [0, 2]], [[2, 0], [1, 0]], [[1, 0], [0, 0]]], np.int32)
    lm, mp = np.zeros((B, 3), np.int32), np.zeros((B, 3), np.float32)
    for i, probs in enumerate(([0.25, 0.75], [0.6, 0.4], [0.2, 0.5, 0.3])):
        e = np.flatnonzero(board[i].ravel() == 0) + 1
        lm[i, :len(e)] = e
        mp[i, :len(e)] = probs
    assert (board[:, 0, 0] != 0).all() and not (lm == 1).any()
    batch = dict(board=torch.tensor(board, device=DEV), legal_moves=torch.tensor(lm, device=DEV),
                 moves_prob=torch.tensor(mp, device=DEV), reward=torch.tensor([1.0, -1.0, 1.0], device=DEV))
    net = _net(n, blocks, chans, seed=9).train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=0.0)
    _preset(net, opt, 78)
    step = NativeTrainStep(net, opt, B, DEV)
    assert _flags(step) == want_flags + (0,)
    lrs = [1e-3 * (1 + i % 7) for i in range(RING_STEPS)]
    mus = [(0.9, 0.5, 0.0)[i % 3] for i in range(RING_STEPS)]
    wds = [(0.0, 1e-3)[i % 2] for i in range(RING_STEPS)]
    params = dict(net.named_parameters())
    watched = ["move_fc.bias", "move_fc.weight", "bn1.weight", "resblocks.0.conv1.weight"]
    P = {k: params[k].detach() for k in watched}
    M = {k: opt.state[params[k]]["momentum_buffer"] for k in watched}
    p_init = {k: P[k].clone().view(-1) for k in watched}
    m_init = {k: M[k].clone().view(-1) for k in watched}
    snap_p = {k: torch.empty((RING_STEPS, P[k].numel()), device=DEV) for k in watched}
    snap_m = {k: torch.empty((RING_STEPS, P[k].numel()), device=DEV) for k in watched}
    pg = opt.param_groups[0]
    for i in range(RING_STEPS):          # no .cpu(), no .item(), no synchronize, no debug in here
        pg["lr"], pg["momentum"], pg["weight_decay"] = lrs[i], mus[i], wds[i]
        step.step(batch)
        for k in watched:
            snap_p[k][i].copy_(P[k].view(-1))
            snap_m[k][i].copy_(M[k].view(-1))
    torch.cuda.synchronize()
    assert step.steps == RING_STEPS
    assert _flags(step) == want_flags + (want_flags[0],)
    lr = np.array([_f32(x) for x in lrs])[:, None]
    mu = np.array([_f32(x) for x in mus])[:, None]
    wd = np.array([_f32(x) for x in wds])[:, None]
    zero_grad = {"move_fc.bias": np.arange(1), "move_fc.weight": np.arange(4 * cells)}     # entry 0; row 0

    def where(bad):
        i = int(np.argmax(bad.any(1)))
        return "first at step %d (slot %d; lr %g, momentum %g, weight decay %g)" % (i, i % 256, lrs[i], mus[i], wds[i])
    for k in watched:
        p = snap_p[k].cpu().numpy().astype(np.float64)
        m = snap_m[k].cpu().numpy().astype(np.float64)
        assert np.isfinite(p).all() and np.isfinite(m).all(), k
        p_prev = np.concatenate([p_init[k].cpu().numpy().astype(np.float64)[None], p[:-1]])
        m_prev = np.concatenate([m_init[k].cpu().numpy().astype(np.float64)[None], m[:-1]])
        bad = np.abs(p - p_prev + lr * m) > 8 * EPS * (np.abs(p_prev) + lr * np.abs(m))
        assert not bad.any(), "%s: p_i - p_(i-1) != -lr_i m_i on %d steps, %s" % (k, int(bad.any(1).sum()), where(bad))
        assert (np.abs(m).max(1) > 0).all(), k               # (the identity above is not 0 = 0)
        if k in zero_grad:
            z = zero_grad[k]
            want, _, tol_m, _ = expected(p_prev[:, z], m_prev[:, z], np.zeros_like(m[:, z]), 0.0, mu, wd)
            bad = np.abs(m[:, z] - want) > tol_m
            assert not bad.any(), "%s: m_i != mu_i m_(i-1) + wd_i p_(i-1) on %d steps, %s" % (k, int(bad.any(1).sum()), where(bad))
    g = step.debug("grad:move_fc.bias")
    assert g[0] == 0 and np.abs(g[1:]).max() > 0
    assert (step.debug("grad:move_fc.weight").reshape(cells, 4 * cells)[0] == 0).all()
    step.close()


def _probe_mode(want_flags):
    """A trainer made in the current environment reports the mode the test meant to set (and, after one step, the
    graph where there should be one)."""
    from azalea_amd.native_train import NativeTrainStep
    net = _net(5, 1, 16)
    step = NativeTrainStep(net, torch.optim.SGD(net.parameters(), lr=0.0, momentum=0.9), 4, DEV)
    assert _flags(step) == want_flags + (0,)
    step.step({k: v.to(DEV) for k, v in _random_batch(5, 4, 1).items()})
    torch.cuda.synchronize()
    assert _flags(step) == want_flags + (want_flags[0],)
    step.close()


@pytest.mark.parametrize("mode", ["graph", "nofork", "graph+nofork"])
def test_intermediates_match_autograd_under_graph_and_inline_modes(monkeypatch, mode):
    """test_gpu_native_train.py's layer-by-layer comparison, narrow and wide, with the step captured as one HIP graph
    and / or the filter gradients in line."""
    _probe_mode(_set_mode(monkeypatch, mode))
    T.test_every_intermediate_matches_autograd(11, 2, 64, 8)
    T.test_every_intermediate_matches_autograd(9, 2, 32, 7)
    T.test_every_intermediate_matches_autograd(13, 1, 128, 5)
    T.test_every_intermediate_matches_autograd(12, 1, 64, 5)


@pytest.mark.parametrize("mode", ["graph", "nofork", "graph+nofork"])
def test_large_batches_under_graph_and_inline_modes(monkeypatch, mode):
    """... and its float64 comparison at batches past TRN_PRESUM_BATCH = 256: the k_trn_totals path inside a captured
    graph, narrow and wide."""
    _probe_mode(_set_mode(monkeypatch, mode))
    T.test_odd_batches_and_boards(7, 2, 32, 300)
    T.test_odd_batches_and_boards(9, 1, 128, 261)


def test_ring_fed_native_step_equals_the_batch_fed_one():
    """NativeTrainStep.step_from_ring (the collate kernel writing straight into the step's input buffers, queued on the
    same stream) against NativeTrainStep.step on DeviceReplayBuffer.sample of the same rows -- the twin of
    test_train_step.py::test_ring_fed_graphed_step_equals_the_batch_fed_one: inputs bit for bit, losses and every
    tensor to that test's 1e-5; the last two steps with the rows turned to the mover's view."""
    from azalea_amd import engine as eng
    from azalea_amd.device_replay import DeviceReplayBuffer
    from azalea_amd.native_train import NativeTrainStep
    from azalea_amd.network import HexNetwork
    dev = torch.device("cuda", 0)
    E = eng.Engine(board_size=5, n_games=64, simulations=20, search_batch_size=10, evaluator=eng.EVAL_UNIFORM,
                   noise_scale=0.25)
    buf = DeviceReplayBuffer(E, 2000, shared=False)
    E.replay_fill(1500)
    B, cells = 32, 25
    nets, opts, steps = [], [], []
    for _ in range(2):
        torch.manual_seed(4)
        net = HexNetwork(board_size=5, num_blocks=1, base_chans=16).to(dev)
        opts.append(torch.optim.SGD(net.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4))
        nets.append(net)
        steps.append(NativeTrainStep(net, opts[-1], B, dev))
    rng = np.random.RandomState(0)
    for i in range(6):
        if i == 4:
            buf.mover_view = True
        idx = rng.randint(0, len(buf), B)
        la = steps[0].step(buf.sample(idx)).cpu().numpy().copy()
        lb, k = steps[1].step_from_ring(buf, idx)
        assert k == cells
        lb = lb.cpu().numpy()
        assert np.isfinite(la).all() and np.abs(la - lb).max() <= 1e-5, (i, la, lb)
        for name in ("board", "legal_moves", "moves_prob", "reward"):
            assert torch.equal(getattr(steps[0], name), getattr(steps[1], name)), (i, name)
    assert steps[0].steps == steps[1].steps == 6
    for (na, a), (_, b) in zip(nets[0].state_dict().items(), nets[1].state_dict().items()):
        assert float((a.double() - b.double()).abs().max()) <= 1e-5, na
    for pa, pb in zip(nets[0].parameters(), nets[1].parameters()):
        ma, mb = opts[0].state[pa]["momentum_buffer"], opts[1].state[pb]["momentum_buffer"]
        assert float((ma.double() - mb.double()).abs().max()) <= 1e-5
    for s in steps:
        s.close()
    E.close()
