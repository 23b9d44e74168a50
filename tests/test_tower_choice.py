"""The choice of the tower (TowerChoice, azalea_amd/csrc/net_priv.h) held on the CPU through the host-only
accessor azx_debug_tower_choice, which answers from the code azx_net_create chooses with:
  * every case of tests/golden/tower_choice.json -- dumped from the selection logic of the commit before the choice was
    folded into one descriptor (tests/golden/make_tower_choice.py) -- still gets its answer or its error;
  * the two Python restatements of the choice, forward_accuracy_cases.expected_kernels and policy.tower_flags, agree with
    the library on the whole grid."""
import importlib.util
import json
import os
import re

import pytest

from azalea_amd import _lib, engine
from forward_accuracy_cases import expected_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_tower_choice", os.path.join(GOLDEN, "make_tower_choice.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mk = _load_maker()

with open(mk.FIXTURE) as _f:
    WANT = json.load(_f)


def test_the_fixture_holds_the_grid_of_the_script_once():
    cases = [tuple(c) for row in WANT for c in row["cases"]]
    assert len(cases) == len(set(cases)) == 12 * 3 * 6 * 3 * 2 + 2 * 12 * 2
    assert set(cases) == set(mk.cases())
    answers = [json.dumps(row["answer"], sort_keys=True) for row in WANT]
    assert len(answers) == len(set(answers))
    # not vacuous: every tower and both heads kernels are chosen somewhere, and both refusals are met
    texts = " | ".join(row["answer"].get("text", row["answer"].get("message")) for row in WANT)
    for needle in ("k_stem_generic + k_conv_generic (VALU)", "k_tower_mfma<64,4,2,1,2>", "k_tower_mfma<64,6,1,2,2>",
                   "k_tower_mfma<32,6,2,2,1>", "k_tower_f16x3_s16 + k_heads_mfma", "k_tower_f16x3_s16 + k_heads (",
                   "k_tower_f16_s16 +", "k_stem_wide_f16x3 + k_conv_wide_f16x3_s16 per layer",
                   "k_stem_wide_f16 + k_conv_wide_f16_s16 per layer", "AZX_TOWER_TILES=rows", "AZX_HEADS=valu",
                   "AZX_TOWER=fp32 forces the fp32 tower", "with at least one block"):
        assert needle in texts, needle
    assert {row["answer"]["error"] for row in WANT if "error" in row["answer"]} == {-1}      # AZX_EINVAL


@pytest.mark.parametrize("row", range(len(WANT)))
def test_every_case_of_an_answer_still_gets_it(row):
    want = WANT[row]["answer"]
    for case in WANT[row]["cases"]:
        assert mk.answer(tuple(case)) == want, case


def test_the_header_the_binding_and_the_wrapper():
    with open(os.path.join(ROOT, "include", "azx.h")) as f:
        text = f.read()
    assert re.search(r"^int azx_debug_tower_choice\(int board_size, int num_blocks, int base_chans, int flags, "
                     r"char \*buf, int cap\);", text, re.M)
    assert "dlsym azx_debug_tower_choice" in text
    assert "azx_debug_tower_choice" in _lib.SYMBOLS and "azx_debug_tower_choice" not in _lib.OPTIONAL
    assert _lib.lib().azx_version() == 7
    assert engine.tower_choice(5, 1, 64) == mk.ask(5, 1, 64, 0, "")
    assert engine.tower_choice(5, 1, 64).startswith("k_tower_f16x3_s16 + k_heads_mfma (1x64 on 5x5; AZX_TOWER=default ")
    assert engine.tower_choice(5, 1, 128, engine.FLAG_TOWER_F16).startswith("k_stem_wide_f16 + k_conv_wide_f16_s16 per layer")
    with pytest.raises(_lib.AzxError, match=r"azx error -1: net: the plain-f16 tower \(AZX_FLAG_TOWER_F16\) exists for"):
        engine.tower_choice(5, 1, 32, engine.FLAG_TOWER_F16)
    with pytest.raises(_lib.AzxError, match="azx error -1: net: board size out of range"):
        engine.tower_choice(14, 1, 64)
    # the text is truncated to the buffer, its full length is returned
    import ctypes as C
    buf = C.create_string_buffer(8)
    assert _lib.lib().azx_debug_tower_choice(5, 1, 64, 0, buf, 8) == len(engine.tower_choice(5, 1, 64))
    assert buf.value == b"k_tower"


def test_expected_kernels_is_the_start_of_the_accessors_text_on_the_whole_grid():
    """For the flag-off cases it models: AZX_TOWER unset or fp32 (it has no plain-f16 names), AZX_HEADS=valu."""
    seen = 0
    for n, blocks, chans, flags, switch in mk.cases():
        if flags or switch in ("AZX_TOWER=f16", "AZX_TOWER_TILES=rows"):
            continue
        env = dict([switch.split("=")]) if switch else {}
        got = mk.ask(n, blocks, chans, 0, switch)
        assert isinstance(got, str) and got.startswith(expected_kernels(n, blocks, chans, env)), (n, blocks, chans, switch, got)
        seen += 1
    assert seen == 12 * 3 * 6 * 2 + 12 * 2


def test_tower_flags_accepts_f16_on_exactly_the_shapes_the_library_accepts_the_flag_on():
    from azalea_amd.policy import Policy, tower_flags
    pol = Policy()
    pol.initialize(dict(device="cpu", network="HexNetwork", board_size=5, num_blocks=1, base_chans=16,
                        simulations=20, search_batch_size=4, exploration_coef=0.5, exploration_depth=4,
                        exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0, seed=1))
    pol.tower_precision = "f16"
    accepted = 0
    for n in mk.BOARDS:
        for blocks in mk.BLOCKS:
            for chans in mk.CHANS:
                pol.board_size, pol.num_blocks, pol.base_chans = n, blocks, chans       # all tower_flags reads of the shape
                try:
                    python = tower_flags(pol) == engine.FLAG_TOWER_F16
                except ValueError:
                    python = False
                library = isinstance(mk.ask(n, blocks, chans, mk.F16, ""), str)
                assert python == library, (n, blocks, chans, python, library)
                accepted += library
    assert 0 < accepted < len(mk.BOARDS) * len(mk.BLOCKS) * len(mk.CHANS)
