"""Pins tests/forward_accuracy_cases.py, the fixtures and bounds the default towers are held to on the device: every
"peaked" weight set is as peaked as the trained checkpoint (golden G8), and the bound of the fused split-f16 tower can
tell the hi + lo split from one whose lo halves lost three mantissa bits -- a 2^-18 operand error -- on those fixtures,
shown with the split's float64 definition (f16_emulation.forward(lo_bits=...)).  CPU only."""
import numpy as np
import pytest

import f16_emulation
import forward_accuracy_cases as fac

FUSED_FIXTURES = sorted({name for name, env, family in fac.CASES.values() if family == fac.FUSED})


@pytest.mark.parametrize("name", sorted(fac.FIXTURES))
def test_fixture_conditions(name):
    plain, peaked = fac.fixture(name, "plain"), fac.fixture(name, "peaked")
    n, count = plain["n"], len(plain["boards"])
    assert count >= 32 or name == "5x5_1x64"                 # (7 boards there: the dead partner board is the point)
    assert count % 2 == 1 or name == "g8"                    # (the checkpoint's 48 recorded positions)
    for fx in (plain, peaked):
        assert fx["boards"].shape == (count, n, n) and fx["legal"].any(1).all()
        for b, lm in zip(fx["boards"], fx["lm"]):            # the move list is the board's empty cells (G8: in its own order)
            assert np.array_equal(np.sort(lm[lm > 0]), np.flatnonzero(b.ravel() == 0) + 1)
        assert np.isfinite(fx["value"]).all() and np.isfinite(fx["logprob"]).all()
        assert 0 < fx["e32_v"] < 1e-4 and 0 < fx["e32_lp"] < 1e-3         # the units are fp32 noise, not a wrong module
        assert fx["max_act"] < 65504 / 64                    # far inside the f16 range
    # the peaked net: the same tower, heads scaled up (never down) until both conditions hold
    assert peaked["s_p"] >= 1 and peaked["s_v"] >= 1 and peaked["max_act"] == plain["max_act"]
    for k in plain["state"]:
        same = np.array_equal(plain["state"][k], peaked["state"][k])
        assert same or k.startswith(("move_fc.", "value_fc3.")), k
    gap = np.median(fac.logit_gaps(peaked["logprob"], peaked["legal"]))
    share = np.mean(np.abs(peaked["value"]) > fac.SATURATED)
    print("%s: factors %.3g / %.3g; median logit gap %.3g (G8: %.3g); share of |v| > %.1f: %.2f; max activation %.3g; "
          "e32 plain %.3g / %.3g, peaked %.3g / %.3g" % (name, peaked["s_p"], peaked["s_v"], gap, fac.g8_median_gap(),
                                                         fac.SATURATED, share, peaked["max_act"], plain["e32_v"],
                                                         plain["e32_lp"], peaked["e32_v"], peaked["e32_lp"]))
    assert gap >= fac.g8_median_gap()
    assert share >= fac.SATURATED_SHARE


def test_expected_kernels_cover_every_family():
    towers = {}
    for case, (name, env, family) in fac.CASES.items():
        fx = fac.fixture(name, "plain")
        towers.setdefault(fac.expected_kernels(fx["n"], fx["blocks"], fx["chans"], env), family)
    assert len(towers) == 7, towers                           # fused with either heads, three fp32 tilings, wide, VALU
    for info, family in towers.items():
        assert ("f16x3" in info) == (family != fac.FP32), (info, family)


def _emulated(name, kind, bits):
    fx = fac.fixture(name, kind)
    value, logprob = f16_emulation.forward(fx["state"], fx["blocks"], fx["boards"], fx["lm"], lo_bits=bits)
    return fx, fac.errors(fx, value, logprob)


@pytest.mark.parametrize("kind", fac.KINDS)
@pytest.mark.parametrize("name", FUSED_FIXTURES)
def test_split_definition_stays_inside_the_bound(name, kind):
    fx, (k_v, k_lp) = _emulated(name, kind, 10)
    b_v, b_lp = fac.bounds(fx, fac.FUSED)
    print("%s %s, 10 bits: value %.3g (bound %.3g), log-prob %.3g (bound %.3g)" % (name, kind, k_v, b_v, k_lp, b_lp))
    assert k_v <= b_v and k_lp <= b_lp


@pytest.mark.parametrize("name", FUSED_FIXTURES)
def test_seven_bit_lo_halves_fall_outside_the_bound(name):
    fx, (k_v, k_lp) = _emulated(name, "peaked", 7)
    b_v, b_lp = fac.bounds(fx, fac.FUSED)
    print("%s peaked, 7 bits: value %.3g (bound %.3g), log-prob %.3g (bound %.3g)" % (name, k_v, b_v, k_lp, b_lp))
    assert k_v > b_v or k_lp > b_lp


def test_lo_bits_keyword():
    """hi + lo carries 22 significant bits; cutting lo to b bits leaves an error of at most half a unit of its b-th bit;
    without the keyword the emulation is the plain-f16 one, unchanged."""
    x = np.random.RandomState(1).uniform(-4, 4, 4096)
    import torch
    t = torch.as_tensor(x)
    hi = t.float().half().double()
    for bits in (10, 9, 7, 0):
        lo = f16_emulation._lo_half(t - hi, bits)
        rem = (t - hi).float().half().double()               # the full lo half
        unit = 2.0 ** (np.floor(np.log2(np.abs(rem.numpy()).clip(2.0 ** -14))) - bits)
        assert (np.abs((lo - rem).numpy()) <= unit / 2).all(), bits
        if bits == 10:
            assert torch.equal(lo, rem) and float((hi + lo - t).abs().max()) <= 4 * 2.0 ** -22
    fx = fac.fixture("5x5_1x64", "plain")
    args = (fx["state"], fx["blocks"], fx["boards"], fx["lm"])
    plain = f16_emulation.forward(*args)
    again = f16_emulation.forward(*args, rounded=True, lo_bits=None)
    assert all(np.array_equal(a, b) for a, b in zip(plain, again))
    split = f16_emulation.forward(*args, lo_bits=10)
    exact = f16_emulation.forward(*args, rounded=False)
    assert fac.errors(fx, *exact)[1] < 1e-5                   # (the folded weights are stored as fp32)
    assert fac.errors(fx, *split)[1] < fac.errors(fx, *plain)[1] / 100
