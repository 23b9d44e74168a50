"""The default, fp32-class towers and heads on the device against the exact float64 module, in units of fp32's own error.

Every forward test elsewhere holds these kernels to an absolute 1e-4 on seeded nets, where a correct kernel is near
1e-6: a tower that lost one of its three split products on one tap or tile would pass them.  Here every tower kernel
and tiling (forward_accuracy_cases.CASES: the fused split-f16 tower with edge and row tiles and both heads kernels,
the three exact-fp32 MFMA tilings, the wide split-f16 pair, the VALU pair) runs a plain and a "peaked" weight set and
must stay within R * e32 + floor of the float64 truth, where e32 is the distance of torch's fp32 CPU module from the
same truth and the floor is half an fp32 ulp at the output's size.  Each case also pins the dispatch: kernel_info()
must name the tower and heads kernel the case was written for.

R per family is twice the worst ratio measured on an MI355X, rounded up (profiles/forward_accuracy.json holds the raw
table, and which cases diagnostic builds with the lo halves cut to 7 and 9 mantissa bits fail); ratio = (error -
floor) / e32, worst over value and log-prob:
  split-f16 fused   worst 2.16 (5x5 1x64 peaked, log-prob 6.3e-6 against e32 2.4e-6); G8 1.92; R = 5
  split-f16 wide    worst 4.56 (13x13 2x128 peaked, value 6.1e-7 against e32 1.2e-7); 11x11 2x128 4.44; R = 10
  exact fp32, VALU  worst 2.10 (11x11 1x64 under AZX_TOWER=fp32, peaked, log-prob 1.35e-5 against e32 5.9e-6); R = 5
The plain nets sit at 1e-8 .. 1e-7 on the value and 1e-7 .. 1e-6 on the log-probs, mostly inside the floors; the
peaked ones at 1e-7 .. 4e-6 and 4e-6 .. 4e-5.  A correct fp32 convolution in another summation order, the CPU oracle's,
is itself 1.0 .. 3.0 e32 from the truth on the exact-fp32 fixtures, so ratios near 2 are summation order, not loss.
With 7-bit lo halves every peaked case of the fused tower is outside its bound (by 1.3x .. 2.5x), as are the wide
pair's two-block cases; its one-block and stem-only cases (12x12 1x256, 5x5 0x128) stay inside, at 0.85 and 0.37 of
the bound, whatever the head factors: fewer sums see a cut operand there.  The exact-fp32 and VALU cases do not move."""
import numpy as np
import pytest

import forward_accuracy_cases as fac
from azalea_amd import engine as eng

pytestmark = pytest.mark.gpu


def run_case(case, kind):
    """Create the case's engine, pin its kernels, run the forward: the outputs and the figures the bounds are about."""
    name, env, family = fac.CASES[case]
    fx = fac.fixture(name, kind)
    with fac.environ(**env):
        E = eng.Engine(board_size=fx["n"], n_games=8, simulations=10, search_batch_size=10, evaluator=eng.EVAL_RESNET,
                       num_blocks=fx["blocks"], base_chans=fx["chans"])
    try:
        info = E.kernel_info()
        assert fac.expected_kernels(fx["n"], fx["blocks"], fx["chans"], env) in info, info
        for k, v in env.items():
            assert "%s=%s" % (k, v) in info, info
        E.set_weights(fx["state"])
        value, logprob = E.forward(fx["boards"], fx["lm"])
    finally:
        E.close()
    k_v, k_lp = fac.errors(fx, value, logprob)
    return dict(case=case, kind=kind, family=family, value=value, logprob=logprob, k_v=k_v, k_lp=k_lp,
                e32_v=fx["e32_v"], e32_lp=fx["e32_lp"], floor_v=fac.FLOOR_V, floor_lp=fac.floor_lp(fx))


@pytest.mark.parametrize("case,kind", fac.PAIRS)
def test_forward_accuracy(case, kind):
    f = run_case(case, kind)
    fx = fac.fixture(fac.CASES[case][0], kind)
    b_v, b_lp = fac.bounds(fx, f["family"])
    print("%s %s (%s): kernel vs exact: value %.3g, log-prob %.3g; fp32 torch vs exact: value %.3g, log-prob %.3g; "
          "bounds: value %.3g, log-prob %.3g" % (case, kind, f["family"], f["k_v"], f["k_lp"], f["e32_v"], f["e32_lp"],
                                                 b_v, b_lp))
    assert np.isfinite(f["value"]).all() and np.isfinite(f["logprob"]).all()
    assert f["k_v"] <= b_v, (f["k_v"], f["e32_v"], b_v)
    assert f["k_lp"] <= b_lp, (f["k_lp"], f["e32_lp"], b_lp)
