"""Pins tests/f16_wide_emulation.py, the yardstick the plain-f16 wide tower is held to on the device: without the f16
rounding it is the network itself (the float64 HexNetwork), with it it differs from the exact module by what was
measured when the switch was specified -- so the yardstick cannot drift silently.  CPU only."""
import numpy as np
import pytest

import f16_wide_emulation as emu

# max |d value|, max |d log-prob| over legal moves of the rounded emulation against the exact module, as specified
MEASURED = {"5x5": (8.6e-6, 4.1e-5), "9x9": (2.0e-5, 5.3e-5), "13x13": (1.8e-5, 6.1e-5), "19x256": (4.7e-5, 2.3e-4)}


def test_fixtures_are_the_specified_ones():
    assert emu.FIXTURES == {"5x5": (5, 1, 128, 5, 31), "9x9": (9, 3, 128, 9, 41), "13x13": (13, 2, 256, 11, 51),
                            "19x256": (13, 19, 256, 4, 61)}


@pytest.mark.parametrize("name", sorted(MEASURED))
def test_emulation_against_the_exact_module(name):
    c = emu.case(name)
    legal = c["legal"]
    v, lp = emu.forward(c["state"], c["blocks"], c["boards"], c["lm"], rounded=False)
    print(name, "exact:", np.abs(v - c["value"]).max(), np.abs(lp - c["logprob"])[legal].max())
    assert np.abs(v - c["value"]).max() <= 2e-5
    assert np.abs(lp - c["logprob"])[legal].max() <= 2e-5
    dv, dlp = np.abs(c["emu_value"] - c["value"]).max(), np.abs(c["emu_logprob"] - c["logprob"])[legal].max()
    print(name, "rounded:", dv, dlp)
    for got, want in zip((dv, dlp), MEASURED[name]):
        assert want / 2 <= got <= want * 2, (got, want)


def test_the_heads_are_not_rounded():
    """What sets this definition apart from tests/f16_emulation.py: there the head filters and their input are f16."""
    import f16_emulation
    c = emu.case("5x5")
    v6, lp6 = f16_emulation.forward(c["state"], c["blocks"], c["boards"], c["lm"], rounded=True)
    assert np.abs(v6 - c["emu_value"]).max() > 0 or np.abs(lp6 - c["emu_logprob"]).max() > 0
    # ... and without any rounding the two are the same network
    a = f16_emulation.forward(c["state"], c["blocks"], c["boards"], c["lm"], rounded=False)
    b = emu.forward(c["state"], c["blocks"], c["boards"], c["lm"], rounded=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
