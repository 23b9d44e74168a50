"""Writes tests/golden/tower_choice.json: which tower and heads kernels azx_net_create gives every network shape under
the flag and the switches that bear on the choice, as azx_debug_tower_choice answers (no GPU is needed).
tests/test_tower_choice.py reads the file and asks the library the same questions; it never writes it.

Made ONCE, from the selection logic of the commit BEFORE the choice was folded into one descriptor (TowerChoice,
net_priv.h): that commit's lines of azx_net_create -- the `if` chain over tower_variant, the chain that names the
kernels, the refusals of AZX_FLAG_TOWER_F16 -- were first moved verbatim behind the new accessor, this file was dumped
from that build, and only then was the logic rewritten.  The fixture is what says the rewrite chooses as the chains did.

    python tests/golden/make_tower_choice.py

The grid: board 2..13 x blocks {0, 1, 2} x channels {16, 32, 64, 128, 192, 256} x AZX_TOWER {unset, fp32, f16} x flag
{0, AZX_FLAG_TOWER_F16}; AZX_HEADS=valu and AZX_TOWER_TILES=rows each over board 2..13 x channels {64, 128} at one
block.  An answer is the accessor's text with the shape ("<blocks>x<channels> on <n>x<n>") replaced by "{shape}", or
the error code with its message; each distinct answer is stored once, with the cases [n, blocks, channels, flags,
"SWITCH=value" or ""] that give it.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "tower_choice.json")

F16 = 4                     # AZX_FLAG_TOWER_F16
BOARDS, BLOCKS, CHANS = range(2, 14), (0, 1, 2), (16, 32, 64, 128, 192, 256)
SWITCHES = ("AZX_TOWER", "AZX_TOWER_TILES", "AZX_WIDE_STREAMS", "AZX_HEADS", "AZX_PACK")


def cases():
    out = [(n, b, c, flags, switch) for n in BOARDS for b in BLOCKS for c in CHANS
           for switch in ("", "AZX_TOWER=fp32", "AZX_TOWER=f16") for flags in (0, F16)]
    out += [(n, 1, c, 0, switch) for switch in ("AZX_HEADS=valu", "AZX_TOWER_TILES=rows") for n in BOARDS for c in (64, 128)]
    return out


def shape(n, blocks, chans):
    return "%dx%d on %dx%d" % (blocks, chans, n, n)


def ask(n, blocks, chans, flags, switch):
    """The accessor's answer under `switch` alone: its text, or (error code, message)."""
    from azalea_amd import _lib
    L = _lib.lib()
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    if switch:
        os.environ.update([switch.split("=")])
    try:
        buf = C.create_string_buffer(512)
        rc = L.azx_debug_tower_choice(n, blocks, chans, flags, buf, len(buf))
        return buf.value.decode() if rc >= 0 else (rc, L.azx_last_error().decode())
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def answer(case):
    """The answer as the fixture stores it: {"text": with {shape}} or {"error": code, "message": text}."""
    got = ask(*case)
    if isinstance(got, tuple):
        return dict(error=got[0], message=got[1])
    assert got.count(shape(*case[:3])) == 1, got
    return dict(text=got.replace(shape(*case[:3]), "{shape}"))


def main():
    sys.path.insert(0, ROOT)
    answers = {}
    for case in cases():
        answers.setdefault(json.dumps(answer(case), sort_keys=True), []).append(list(case))
    rows = [dict(answer=json.loads(a), cases=c) for a, c in sorted(answers.items())]
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n")
    print("wrote %s: %d answers to %d cases" % (FIXTURE, len(rows), len(cases())))


if __name__ == "__main__":
    main()
