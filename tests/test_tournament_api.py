"""The tournament entry points (azx_tournament_*: several matches side by side in one ply loop on the device) at the
C boundary and the argument checks of evaluation.evaluate_throughput(pooled=True) -- everything that can be held
without a GPU.  The games themselves are tests/test_gpu_tournament.py's."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from option_api_stubs import _Agent  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOURNAMENT_SYMBOLS = ("azx_tournament_create", "azx_tournament_destroy", "azx_tournament_play")
AZX_EINVAL = -1


def header():
    return open(os.path.join(ROOT, "include", "azx.h")).read()


def test_header_declares_the_tournament_entry_points_and_the_library_exports_them():
    from azalea_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(azx_[a-z_0-9]+)\s*\(", code))
    for name in TOURNAMENT_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(_lib.lib(), name), name
    assert "typedef struct azx_tournament azx_tournament;" in code


def test_the_ctypes_signature_is_the_headers():
    """The argument list of azx_tournament_play, type by type (a wrong width here corrupts the call silently)."""
    from azalea_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    decl = re.search(r"int\s+azx_tournament_play\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    types = [re.sub(r"\s*\w+$", "", " ".join(a.split())).replace("const ", "") for a in decl.split(",")]
    assert types == ["azx_tournament *", "int", "int32_t *", "int32_t *", "int64_t", "int64_t", "int32_t",
                     "int8_t *", "int16_t *", "int16_t *", "azx_match_stats *"]
    res, args = _lib.SYMBOLS["azx_tournament_play"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64, C.c_int64, C.c_int32,
                    C.POINTER(C.c_int8), C.POINTER(C.c_int16), C.POINTER(C.c_int16), C.POINTER(_lib.MatchStats)]


def test_abi_revision_is_unchanged():
    """The tournament calls are an addition within revision 7: callers detect them by symbol."""
    from azalea_amd import _lib
    assert _lib.lib().azx_version() == 7


def test_null_and_short_arguments_are_refused():
    from azalea_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.azx_tournament_create(None, 2, C.byref(h)) == AZX_EINVAL
    assert not h.value and L.azx_last_error()
    two_nulls = (C.c_void_p * 2)(None, None)
    assert L.azx_tournament_create(two_nulls, 2, None) == AZX_EINVAL           # nowhere to put the handle
    assert L.azx_tournament_create(two_nulls, 2, C.byref(h)) == AZX_EINVAL     # null engines
    assert not h.value and b"engine 0" in L.azx_last_error()
    for n in (-1, 0, 1):                                                       # fewer than two engines
        assert L.azx_tournament_create(two_nulls, n, C.byref(h)) == AZX_EINVAL
        assert not h.value and b"two engines" in L.azx_last_error()
    pa, pb = (C.c_int32 * 1)(0), (C.c_int32 * 1)(1)
    assert L.azx_tournament_play(None, 1, pa, pb, 0, 1, 1, None, None, None, None) == AZX_EINVAL
    assert L.azx_last_error()
    L.azx_tournament_destroy(None)                                             # a null tournament is ignored


def test_evaluate_throughput_pooled_makes_the_same_checks_before_the_gpu():
    import torch
    from azalea_amd import evaluation
    from azalea_amd.policy import Policy
    from azalea_amd.random_policy import RandomPolicy

    sig = inspect.signature(evaluation.evaluate_throughput)
    assert sig.parameters["pooled"].default is False and sig.parameters["pooled"].kind is inspect.Parameter.KEYWORD_ONLY

    class Duck(torch.nn.Module):
        def run(self, batch):
            raise AssertionError("never evaluated")

    duck = Policy()
    duck.net = Duck()
    good = Policy()
    good.initialize(dict(device="cpu", network="HexNetwork", board_size=5, num_blocks=1, base_chans=32,
                         simulations=10, search_batch_size=2, exploration_coef=0.5, exploration_depth=3,
                         exploration_noise_alpha=0.3, exploration_noise_scale=0.25, exploration_temperature=1.0))
    for bad in (_Agent(RandomPolicy()), _Agent(duck), _Agent(None)):
        with pytest.raises(TypeError):
            evaluation.evaluate_throughput([_Agent(good), bad, _Agent(good)], 4, pooled=True)
        with pytest.raises(TypeError):
            evaluation.evaluate_throughput([bad, _Agent(good)], 4, pooled=True)
    with pytest.raises(ValueError):
        evaluation.evaluate_throughput([_Agent(good), _Agent(good)], 0, pooled=True)
