"""The conditions under which tests/test_gpu_evaluator_edges.py means something, checked on the CPU oracle alone: the
pools of tests/evaluator_edge_cases.py do hand every dirty game out-of-range values from its first search on, no clean
game ever gets one, zero priors reach roots, and the backed-up sums leave the +-2000 the older tests cover on both
sides.  And the arithmetic claim behind the guard, in exact rational arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import evaluator_edge_cases as ec

F32 = np.float32


def test_this_process_keeps_denormals():
    """A CPU that flushed denormals would make the oracle agree with a device that does: it must fail here instead."""
    assert F32(1e-40) / F32(2) != 0
    assert F32(1.4e-45) > 0 and F32(1.4e-45) + F32(1.4e-45) == F32(2.8e-45)
    assert (np.array([1e-40], F32) * F32(0.5))[0] != 0


def test_value_lists_are_on_the_intended_side_of_the_guard():
    assert not ec.in_fast_range(ec.OUT_OF_RANGE).any() and np.isfinite(ec.OUT_OF_RANGE).all()
    assert ec.in_fast_range(ec.EDGE_IN).all()
    assert ec.in_fast_range(np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -15], F32)).all()
    want = [1e-40, -1e-40, 1.4e-45, 1e-30, -3e-25, 2.0 ** -61, 3e35]
    assert set(ec.bits(np.array(want, F32))) <= set(ec.bits(ec.OUT_OF_RANGE))
    below, above = np.nextafter(ec.LO, F32(0)), np.nextafter(ec.HI, F32(np.inf))
    assert below < ec.LO and below in ec.OUT_OF_RANGE and -above in ec.OUT_OF_RANGE and above > ec.HI
    assert ec.LO == F32(8.67361738e-19) and ec.HI == F32(1.0e30)          # the literals of value_in_fast_range
    tiny = np.abs(ec.OUT_OF_RANGE) < F32(2.0 ** -126)
    assert tiny.sum() == 3 and F32(1.4e-45).view(np.uint32) == 1


def test_evaluator_is_a_pure_function_of_its_row():
    rng = np.random.RandomState(0)
    boards = rng.randint(0, 3, (40, 5, 5)).astype(np.int32)
    boards[:, 0, 0] = 0
    legal = np.zeros((40, 25), np.int32)
    for i in range(40):
        e = np.flatnonzero(boards[i].ravel() == 0) + 1
        legal[i, :len(e)] = e
    for cls in ec.VALUE_CLASSES:
        v, p = ec.evaluate(boards, legal, True, cls)
        kmax = int(np.count_nonzero(legal, axis=1).max())
        for i in (0, 7, 39):                       # alone, in another batch width: the same bits
            v1, p1 = ec.evaluate(boards[i:i + 1], legal[i:i + 1, :kmax], True, cls)
            assert ec.bits(v1)[0] == ec.bits(v)[i] and np.array_equal(ec.bits(p1[0]), ec.bits(p[i, :kmax]))
        assert np.isfinite(v).all() and (p >= 0).all() and (p[legal == 0] == 0).all()
        assert np.abs(p.astype(np.float64).sum(1) - 1.0).max() < 1e-6          # the ABI asks for 1e-4
        vc, pc = ec.evaluate(boards, legal, False, cls)
        assert ec.in_fast_range(vc).all() and np.array_equal(ec.bits(pc), ec.bits(p))
        assert not np.signbit(vc[vc == 0]).any()
    v, _ = ec.evaluate(boards, legal, True, "negzero")
    assert (np.signbit(v) & (v == 0)).sum() >= 10
    v, _ = ec.evaluate(boards, legal, True, "edge-in")
    assert ec.in_fast_range(v).all() and np.isin(ec.bits(v), ec.bits(ec.EDGE_IN)).sum() >= 4


@pytest.mark.parametrize("n", [5, 9, 13])
def test_pools_reach_the_edges(n):
    run = ec.oracle_run(n)
    G = run.G
    assert G == (8 if n == 13 else 12) and len(run.rounds) == 4
    for parity in (0, 1):                                    # both colours to move, dirty and clean
        assert len({run.colors[g] for g in range(parity, G, 2)}) == 2
    assert all(len(p) <= n * n // 3 for p in run.prefixes)
    rows = out = zero = 0
    root_zero = False
    small = large = False
    for rnd, row in enumerate(run.rounds):
        for g, rec in enumerate(row):
            bad = ~ec.in_fast_range(rec["values"])
            if run.dirty[g]:
                if rnd == 0:
                    assert bad.sum() >= 1, g           # in its FIRST search
            else:
                assert not bad.any(), (rnd, g)
            assert rec["result"] == 0 or rnd == 3, (rnd, g)  # no game ends before the fourth search
            rows += len(bad)
            out += int(bad.sum())
            zero += int(rec["zero_prior"].sum())
            root_zero |= bool((rec["root_prior"] == 0).any())
            tv = rec["total_value"]
            assert np.isfinite(tv).all()
            a = np.abs(tv[tv != 0])
            small |= bool((a < F32(2.0 ** -83)).any())
            large |= bool((a > F32(2.0 ** 100)).any())
    print("n=%d rows=%d out-of-range=%d zero-prior=%d" % (n, rows, out, zero))
    assert out * 10 >= rows and zero * 4 >= rows and root_zero
    assert small and large
    assert run.flags(0)[run.dirty].all() and not run.flags(3)[~run.dirty].any()
    # the register slots the root uses: one (k <= 64), two (k > 64), three (k > 128), in a dirty game, in every search
    want = {5: (1, 25), 9: (65, 81), 13: (129, 169)}[n]
    assert any(all(want[0] <= row[g]["k_root"] <= want[1] for row in run.rounds) for g in range(0, G, 2))


def test_edge_in_and_negzero_pools_stay_in_range():
    for cls in ("edge-in", "negzero"):
        run = ec.oracle_run(9, cls)
        assert not run.flags(3).any()
        vals = np.concatenate([rec["values"] for row in run.rounds for rec in row[0::2]])
        if cls == "edge-in":
            for x in ec.EDGE_IN:
                assert (ec.bits(vals) == ec.bits(x)).any(), x
        else:
            assert (np.signbit(vals) & (vals == 0)).sum() * 3 >= len(vals)
        assert all(rec["result"] == 0 or rnd == 3 for rnd, row in enumerate(run.rounds) for rec in row)


def test_round_f32_is_numpy_rounding():
    rng = np.random.RandomState(1)
    x = np.concatenate([np.ldexp(rng.uniform(1, 2, 300), rng.randint(-160, 120, 300)), [2.0 ** -149 * 0.5, 2.0 ** -149 * 1.5,
                       2.0 ** -126 * (1 - 2.0 ** -25), 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24]])
    for v in x:
        assert float(ec.round_f32(Fraction(v))) == float(F32(v)), v


def test_unscaled_divide_is_exact_inside_the_guard():
    """div2_unscaled in rational arithmetic, every fma rounded once, the reciprocal tried as the correctly rounded
    value and one unit to either side of it: inside the guard (total_value sums that are multiples of 2^-83, up to 2^24
    backups of 1e30) it always equals the IEEE quotient -- provided denormal intermediates are kept."""
    for name, (num, den) in ec.guard_divide_cases(400).items():
        for a, d in zip(num, den):
            fa, fd = Fraction(float(a)), Fraction(float(d))
            want = ec.round_f32(fa / fd)
            assert float(want) == float(a / d)
            for u in (-1, 0, 1):
                assert ec.div_unscaled_exact(fa, fd, u) == want, (name, float(a), float(d), u)
