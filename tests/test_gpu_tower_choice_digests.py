"""Every tower azx_net_create can choose still packs and computes what it did before the choice was folded into one
descriptor (TowerChoice, azalea_amd/csrc/net_priv.h): one case per row of the choice's table at the smallest
shape that reaches it, held to tests/golden/tower_forward_digests.json -- the kernels named, the digest of the packed
operands under the device pack and under AZX_PACK=host, and a SHA-256 over forward()'s values and log-probabilities.
The fixture was written by tests/golden/make_tower_forward_digests.py on the commit before that change; this file runs
the script's cases and never writes the fixture."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_tower_forward_digests",
                                                  os.path.join(GOLDEN, "make_tower_forward_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mk = _load_maker()

with open(mk.FIXTURE) as _f:
    WANT = json.load(_f)

# the tower each case is there to reach, as its `net=` field begins
REACHES = {
    "generic": "k_stem_generic + k_conv_generic (VALU) + k_heads (1x16 on 5x5;",
    "mfma_64_4": "k_tower_mfma<64,4,2,1,2> (fp32 MFMA) + k_heads (0x64 on 5x5;",
    "mfma_64_6": "k_tower_mfma<64,6,1,2,2> (fp32 MFMA) + k_heads (1x64 on 12x12;",
    "mfma_32_6": "k_tower_mfma<32,6,2,2,1> (fp32 MFMA) + k_heads (1x32 on 5x5;",
    "fused": "k_tower_f16x3_s16 + k_heads_mfma (1x64 on 5x5; AZX_TOWER=default AZX_TOWER_TILES=edge ",
    "fused_f16": "k_tower_f16_s16 + k_heads_mfma (1x64 on 5x5; AZX_TOWER=f16 ",
    "fused_rows": "k_tower_f16x3_s16 + k_heads_mfma (1x64 on 5x5; AZX_TOWER=default AZX_TOWER_TILES=rows ",
    "fused_heads_valu": "k_tower_f16x3_s16 + k_heads (1x64 on 5x5;",
    "fused_fp32": "k_tower_mfma<64,4,2,1,2> (fp32 MFMA) + k_heads (1x64 on 5x5; AZX_TOWER=fp32 ",
    "wide": "k_stem_wide_f16x3 + k_conv_wide_f16x3_s16 per layer + k_heads (1x128 on 5x5; AZX_TOWER=default AZX_TOWER_TILES=edge AZX_WIDE_STREAMS=2 ",
    "wide_f16": "k_stem_wide_f16 + k_conv_wide_f16_s16 per layer + k_heads (1x128 on 5x5; AZX_TOWER=f16 ",
    "wide_streams1": "k_stem_wide_f16x3 + k_conv_wide_f16x3_s16 per layer + k_heads (1x128 on 5x5; AZX_TOWER=default AZX_TOWER_TILES=edge AZX_WIDE_STREAMS=1 ",
    "wide_stem": "k_stem_wide_f16x3 + k_conv_wide_f16x3_s16 per layer + k_heads (0x128 on 5x5;",
}


def test_the_fixture_holds_the_cases_of_the_script():
    assert set(WANT["cases"]) == set(mk.CASES) == set(REACHES) and len(mk.CASES) == 13
    assert (WANT["seed"], WANT["positions"]) == (mk.SEED, mk.POSITIONS)
    for name, c in WANT["cases"].items():
        assert c["net"].startswith(REACHES[name]), name
        assert c["weights_device"] == c["weights_host"], name
    # the switches that choose another kernel change the outputs' bits or the kernels named; those that do not (the
    # tile map, the stream split) leave the bits alone
    fwd = {name: c["forward"] for name, c in WANT["cases"].items()}
    assert fwd["fused"] == fwd["fused_rows"] and fwd["wide"] == fwd["wide_streams1"]
    assert len({fwd[k] for k in ("fused", "fused_f16", "fused_heads_valu", "fused_fp32")}) == 4
    assert fwd["wide"] != fwd["wide_f16"]


@pytest.mark.parametrize("name", list(mk.CASES))
def test_a_case_names_packs_and_computes_what_the_fixture_holds(name):
    from azalea_amd import engine
    n, blocks, chans, flags, env = mk.CASES[name]
    got, want = mk.run_case(mk.CASES[name]), WANT["cases"][name]
    print(name, got)
    # the accessor answers for the engine: the same text, from the same code, with no device call
    with mk.switches(dict(env, AZX_PACK="device")):
        assert engine.tower_choice(n, blocks, chans, flags) == got["net"]
    assert got["net"] == want["net"]
    assert got["weights_device"] == want["weights_device"]
    assert got["weights_host"] == want["weights_host"]
    assert got["forward"] == want["forward"]
