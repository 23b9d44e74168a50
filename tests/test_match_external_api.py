"""Matches and tournaments with custom networks, as far as they can be held without a GPU: the argument checks of
evaluation.evaluate_throughput(external_batch=True) and what the header says about external engines in a match.
The games themselves are tests/test_gpu_match_external.py's."""
import inspect
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from option_api_stubs import SEARCH, _Agent, no_engines  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex_policy():
    from azalea_amd.policy import Policy
    p = Policy()
    p.initialize(dict(device="cpu", network="HexNetwork", board_size=5, num_blocks=1, base_chans=32, **SEARCH))
    return p


def _custom_policy():
    """A Policy around a network that is not a HexNetwork, on the CPU."""
    import torch
    from azalea_amd.policy import Policy

    class Custom(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = torch.nn.Linear(25, 26)

        def run(self, batch):
            raise AssertionError("never evaluated")

    p = _hex_policy()
    p.net = Custom()
    assert isinstance(p, Policy) and not p._uses_device_net()
    return p


def test_external_batch_is_a_keyword_of_evaluate_throughput_and_off_by_default():
    from azalea_amd import evaluation
    p = inspect.signature(evaluation.evaluate_throughput).parameters["external_batch"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_a_custom_network_on_the_cpu_is_a_value_error_that_names_the_device(no_engines):
    from azalea_amd import evaluation
    good, custom = _Agent(_hex_policy()), _Agent(_custom_policy())
    for agents in ([good, custom], [custom, good], [custom, custom]):
        with pytest.raises(ValueError, match=r"CUDA \(ROCm\) device.*\bcpu\b"):
            evaluation.evaluate_throughput(agents, 4, external_batch=True)
    with pytest.raises(TypeError):                   # and without the switch nothing has changed
        evaluation.evaluate_throughput([good, custom], 4)


def test_an_agent_without_a_policy_stays_a_type_error(no_engines):
    from azalea_amd import evaluation
    from azalea_amd.random_policy import RandomPolicy
    good = _Agent(_hex_policy())
    for bad in (_Agent(RandomPolicy()), _Agent(None)):
        with pytest.raises(TypeError):
            evaluation.evaluate_throughput([good, bad], 4, external_batch=True)
        with pytest.raises(TypeError):
            evaluation.evaluate_throughput([bad, good], 4, external_batch=True)


def match_section():
    text = open(os.path.join(ROOT, "include", "azx.h")).read()
    start = text.index("evaluation matches between two engines")
    return re.sub(r"\s*\n \*\s*", " ", text[start:text.index("azx_match_stats;", start)])


def test_the_header_admits_external_engines_to_a_match():
    sec = match_section()
    assert "not supported" not in sec
    assert re.search(r"AZX_EVAL_EXTERNAL with an evaluator registered", sec)
    # no evaluator: refused at create (AZX_EINVAL), AZX_ESTATE when it has gone by the time of azx_match_play
    assert re.search(r"AZX_EINVAL[^.]*AZX_EVAL_EXTERNAL engine with no evaluator registered", sec)
    assert re.search(r"unregistered[^.]*azx_match_play[^.]*AZX_ESTATE", sec)
    assert "AZX_EEXTERNAL" in sec and "AZX_MATCH_INTERLEAVE=0" in sec
    # and the evaluator's own section lists the match among its callers
    text = open(os.path.join(ROOT, "include", "azx.h")).read()
    ev = text[text.index("a caller-supplied evaluator on the device"):text.index("typedef int (*azx_eval_fn)")]
    assert "azx_match_play calls fn" in ev


def test_abi_revision_is_still_7():
    from azalea_amd import _lib
    assert _lib.lib().azx_version() == 7
