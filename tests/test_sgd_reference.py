"""tests/sgd_reference.py, the float64 reference and the element-wise fp32 bounds the native update is held to
(test_gpu_native_update.py): torch.optim.SGD's own fp32 step sits inside the bounds, the reference agrees with a float64
torch.optim.SGD step, and three wrong updates fall outside them."""
import numpy as np
import pytest
import torch

from sgd_reference import EPS, expected

TRIPLES = [(0.1, 0.9, 1e-4), (0.05, 0.0, 0.0), (0.3, 0.5, 0.1), (0.0, 0.9, 1e-2), (7e-3, 0.9, 1e-3)]
N = 20000


def _data():
    """20 000 entries, magnitudes spread log-uniformly over eight decades (1e-6 .. 1e2), signs at random, the three
    arrays independent: every ratio between gradient, weight-decay term and momentum term occurs."""
    rng = np.random.RandomState(3)
    return [(rng.choice([-1.0, 1.0], N) * 10.0 ** rng.uniform(-6, 2, N)).astype(np.float32) for _ in range(3)]


def _torch_step(p0, m0, g, lr, mu, wd, dtype):
    p = torch.nn.Parameter(torch.tensor(p0, dtype=dtype))
    p.grad = torch.tensor(g, dtype=dtype)
    opt = torch.optim.SGD([p], lr=lr, momentum=mu, weight_decay=wd)
    opt.state[p]["momentum_buffer"] = torch.tensor(m0, dtype=dtype)      # preset, non-zero
    opt.step()
    # (at momentum 0 torch.optim.SGD does not touch a buffer at all: d = g + wd p moves the parameter directly, which is
    # what p0 - lr (0 m0 + d) says -- there is then no torch buffer to compare, only the parameter)
    tm = opt.state[p]["momentum_buffer"].numpy().astype(np.float64) if mu != 0 else None
    return tm, p.detach().numpy().astype(np.float64)


@pytest.mark.parametrize("lr,mu,wd", TRIPLES)
def test_torch_fp32_step_is_inside_the_bounds(lr, mu, wd):
    p0, m0, g = _data()
    m1, p1, tol_m, tol_p = expected(p0, m0, g, lr, mu, wd)
    tm, tp = _torch_step(p0, m0, g, lr, mu, wd, torch.float32)
    if tm is None:
        tm = (torch.tensor(g) + wd * torch.tensor(p0)).numpy().astype(np.float64)      # torch's fp32 d, the buffer at mu = 0
    um = float((np.abs(tm - m1) / (tol_m / 8 + 1e-300)).max())
    up = float((np.abs(tp - p1) / (tol_p / 8 + 1e-300)).max())
    print("torch fp32 worst: %.2f units of 2^-24 S (buffer), %.2f (parameter)" % (um, up))
    assert (np.abs(tm - m1) <= tol_m).all(), um
    assert (np.abs(tp - p1) <= tol_p).all(), up
    # the reference rounded to fp32 is, of course, inside its own bound
    assert (np.abs(m1.astype(np.float32) - m1) <= tol_m).all() and (np.abs(p1.astype(np.float32) - p1) <= tol_p).all()


@pytest.mark.parametrize("lr,mu,wd", TRIPLES)
def test_reference_is_torch_sgd_in_float64(lr, mu, wd):
    """1e-15 relative to the size of what is summed (S for the buffer, |p0| + |lr| S for the parameter: torch adds the
    three terms in another order, so where they cancel the RESULT is no fair scale)."""
    p0, m0, g = _data()
    m1, p1, tol_m, tol_p = expected(p0, m0, g, lr, mu, wd)
    tm, tp = _torch_step(p0, m0, g, lr, mu, wd, torch.float64)
    if tm is not None:
        assert (np.abs(tm - m1) <= 1e-15 * tol_m / (8 * EPS)).all()
    assert (np.abs(tp - p1) <= 1e-15 * tol_p / (8 * EPS)).all()


def _mutants(p0, m0, g, lr, mu, wd):
    """(name, changes anything at this triple, m1, p1) for three wrong updates, each computed in float64."""
    p0, m0, g = (np.asarray(a, np.float64) for a in (p0, m0, g))
    m = mu * m0 + g
    yield "wd dropped", wd != 0, m, p0 - lr * m
    m = 0.97 * mu * m0 + g + wd * p0
    yield "mu -> 0.97 mu", mu != 0, m, p0 - lr * m
    m = mu * m0 + g + wd * p0
    yield "p1 from m0", lr != 0, m, p0 - lr * m0


def test_wrong_updates_fall_outside_the_bounds():
    """Sensitivity: weight decay dropped, a momentum factor 3 % off, the parameter moved by the OLD buffer -- each is
    outside tol_m or tol_p at every one of the five triples at which it changes anything at all (wd = 0, mu = 0 and
    lr = 0 make one of them the identity each), and each changes something at three triples or more."""
    p0, m0, g = _data()
    hits = {}
    for lr, mu, wd in TRIPLES:
        m1, p1, tol_m, tol_p = expected(p0, m0, g, lr, mu, wd)
        for name, applies, mm, pp in _mutants(p0, m0, g, lr, mu, wd):
            # (as fp32, like anything a kernel would leave)
            mm, pp = mm.astype(np.float32).astype(np.float64), pp.astype(np.float32).astype(np.float64)
            bad = int((np.abs(mm - m1) > tol_m).sum() + (np.abs(pp - p1) > tol_p).sum())
            if applies:
                assert bad > N // 10, (name, (lr, mu, wd), bad)      # not one lucky element: a tenth of them
                hits[name] = hits.get(name, 0) + 1
            else:
                assert bad == 0, (name, (lr, mu, wd), bad)
    assert len(hits) == 3 and min(hits.values()) >= 3, hits
