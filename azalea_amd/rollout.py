"""RolloutNet: the rollout evaluator behind the reference's network contract -- a network-free MCTS opponent.

NOT the reference's behaviour (its only network-free agent is RandomPolicy).  The value of a position is the share of
`rollouts` uniformly random playouts its mover wins, its priors are uniform; include/azx.h ("Rollout evaluator") has the
definition.  `run` computes it on the host (azx_rollout_value), so it works on CPU tensors and under the host loop
(play_game, evaluate).  Wherever the host builds an EVAL_EXTERNAL engine for a policy -- Policy's own engine,
Player(external_batch=True), the two-agent device-match Player, evaluate_throughput -- a RolloutNet is registered with
Engine.set_rollout_evaluator instead: the rollout kernel runs at the evaluation points, with no torch tensor and no
Python callback in the loop.  It needs no checkpoint and never changes, so a result against it is an absolute one.
"""
import numpy as np
import torch

from . import engine as _eng


class RolloutNet:
    """A duck-typed network (net.run(batch) -> {"value", "moves_logprob"}) with no weights.  `device` only says on
    which GPU the engines built for it live ("cpu": device 0); the class holds no tensors."""

    def __init__(self, rollouts=64, seed=0, device="cpu", **_shape):     # (create_network passes board_size, num_blocks, base_chans)
        rollouts = int(rollouts)
        if not 1 <= rollouts <= 4096:
            raise ValueError("rollouts must be in [1, 4096], got %r" % (rollouts,))
        self.rollouts = rollouts
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.device = torch.device(device)

    def run(self, batch):
        board = batch["board"]
        legal = batch["legal_moves"]
        b = board.detach().cpu().numpy().astype(np.int32)
        k = (legal.detach().cpu().numpy() != 0).sum(axis=1)
        n, kmax = int(legal.shape[0]), int(legal.shape[1])
        value = np.zeros(n, np.float32)
        logprob = np.full((n, kmax), -np.inf, np.float32)
        for i in range(n):
            if k[i] == 0:               # a padding row (policy.external_evaluator pads with empty, move-less rows)
                continue
            _, value[i] = _eng.rollout_value(self.seed, b[i], self.rollouts)
            logprob[i, :k[i]] = np.log(np.float32(1.0) / np.float32(k[i]))
        return {"value": torch.from_numpy(value).to(board.device),
                "moves_logprob": torch.from_numpy(logprob).to(board.device)}

    # ---- what callers do to networks ----
    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def to(self, device):
        self.device = torch.device(device)
        return self

    def state_dict(self):
        return {}

    def load_state_dict(self, state):
        return None

    def parameters(self):
        return iter(())


def is_rollout_net(net):
    return isinstance(net, RolloutNet)


def register_evaluator(eng, net):
    """Give an EVAL_EXTERNAL engine its policy's evaluator: the rollout kernel for a RolloutNet, else the net itself
    through policy.external_evaluator, its forward passes ordered after whatever torch queued last on its device."""
    if is_rollout_net(net):
        eng.set_rollout_evaluator(net.rollouts, net.seed)
        return
    from .parallel_player import _net_device
    from .policy import external_evaluator
    eng.set_external_evaluator(external_evaluator(net))
    dev = _net_device(net)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(dev))
    torch.cuda.ExternalStream(eng.stream, device=dev).wait_event(ev)
