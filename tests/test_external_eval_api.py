"""The external-evaluator surface without a GPU: ABI revision 7 as the header declares it and the library exports it,
and Player(external_batch=True) refusing, with a ValueError, every setup it does not cover."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_revision_7():
    from azalea_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "azx.h")).read()
    assert re.search(r"AZX_EEXTERNAL\s*=\s*-7\b", hdr)
    assert re.search(r"typedef int \(\*azx_eval_fn\)\(", hdr)
    assert re.search(r"int azx_set_external_evaluator\(azx_engine \*e, azx_eval_fn fn, void \*user\);", hdr)
    assert "azx_set_external_evaluator" in _lib.SYMBOLS
    assert _lib.EEXTERNAL == -7
    L = _lib.lib()
    assert hasattr(L, "azx_set_external_evaluator")
    assert L.azx_version() == 7


class Duck(torch.nn.Module):
    """A network that is not a HexNetwork, with the reference's run() contract."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(1, 1)

    def run(self, batch):
        raise AssertionError("not called")


def _policy(net):
    from azalea_amd import Policy
    p = Policy()
    p.net = net
    return p


def test_external_batch_refuses_what_it_does_not_cover():
    from azalea_amd import Player
    from azalea_amd.network import HexNetwork
    duck = types.SimpleNamespace(policy=_policy(Duck()))
    with pytest.raises(ValueError, match="CUDA"):
        Player(None, [duck], n_games=4, external_batch=True)        # the net is on the CPU
    with pytest.raises(ValueError, match="single agent"):
        Player(None, [duck, duck], n_games=4, external_batch=True)
    with pytest.raises(ValueError, match="HexNetwork"):
        Player(None, [types.SimpleNamespace(policy=_policy(HexNetwork(board_size=5, num_blocks=1, base_chans=16)))],
               n_games=4, external_batch=True)
    with pytest.raises(ValueError, match="Policy"):
        Player(None, [types.SimpleNamespace(policy=None)], n_games=4, external_batch=True)
    # the default stays the host loop: no check, no engine
    p = Player(None, [duck], n_games=4)
    assert not p.external_batch and p._engine is None
