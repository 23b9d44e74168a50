"""Pins tests/f16_emulation.py, the yardstick the plain-f16 tower is held to on the device: without the f16 rounding
it is the network itself (the golden outputs of the reference), with it it differs from them by what was measured
when the switch was specified -- so the yardstick cannot drift silently.  CPU only."""
import os

import numpy as np
import pytest

import f16_emulation

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# max |d value|, max |d log-prob| over legal moves of the rounded emulation against the golden outputs, as specified
MEASURED = {"g3_forward_11_6x64.npz": (9.3e-5, 4.8e-4), "g8_checkpoint.npz": (9.8e-4, 2.5e-2)}


@pytest.mark.parametrize("name", sorted(MEASURED))
def test_emulation_against_the_golden_outputs(name):
    z = np.load(os.path.join(GOLDEN, name))
    n, blocks, chans = [int(x) for x in z["cfg"]]
    assert (n, blocks, chans) == (11, 6, 64)
    state = {k[2:]: z[k] for k in z.files if k.startswith("w:")}
    legal = z["legal_moves"] > 0
    v, lp = f16_emulation.forward(state, blocks, z["board"], z["legal_moves"], rounded=False)
    print(name, "exact:", np.abs(v - z["value"]).max(), np.abs(lp - z["moves_logprob"])[legal].max())
    assert np.abs(v - z["value"]).max() <= 2e-5
    assert np.abs(lp - z["moves_logprob"])[legal].max() <= 2e-5
    v, lp = f16_emulation.forward(state, blocks, z["board"], z["legal_moves"], rounded=True)
    dv, dlp = np.abs(v - z["value"]).max(), np.abs(lp - z["moves_logprob"])[legal].max()
    print(name, "rounded:", dv, dlp)
    for got, want in zip((dv, dlp), MEASURED[name]):
        assert want / 2 <= got <= want * 2, (got, want)
    # the rounding moves no board's best legal move
    best = lambda a: np.where(legal, a, -np.inf).argmax(1)   # noqa: E731
    assert np.array_equal(best(lp), best(z["moves_logprob"]))
