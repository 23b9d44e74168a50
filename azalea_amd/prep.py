"""Batching helpers: list of dataclass rows -> dict of zero-padded arrays (azalea/prep.py)."""
import dataclasses as dc
from typing import Dict, Sequence

import numpy as np
import torch


def pad(mats, size=None):
    """Stack scalars, or zero-pad n-d arrays of ragged shape to a common size (prep.py:70-86)."""
    first = mats[0]
    if isinstance(first, (int, float)):
        assert size is None
        return np.array(mats)
    shapes = np.array([np.shape(m) for m in mats], dtype=np.int64).reshape(len(mats), -1)
    largest = shapes.max(axis=0)
    if size is None:
        size = largest
    else:
        assert (largest <= np.asarray(size)).all()
    out = np.zeros((len(mats),) + tuple(int(s) for s in size), dtype=first.dtype)
    for i, m in enumerate(mats):
        out[(i,) + tuple(slice(s) for s in np.shape(m))] = m
    return out


def _columns(seq: Sequence) -> Dict[str, list]:
    names = [f.name for f in dc.fields(seq[0])]
    return {n: [getattr(row, n) for row in seq] for n in names}


def batch_games(seq) -> Dict[str, np.ndarray]:
    """Game states -> {'color','legal_moves','result','board'} arrays (prep.py:15-21)."""
    return {name: pad(col) for name, col in _columns(seq).items()}


def batch_replays(seq) -> Dict[str, np.ndarray]:
    """Replay records -> flat dict: the state's fields, then moves_prob and reward (prep.py:24-33)."""
    cols = _columns([rec.state for rec in seq])
    for name, col in _columns(seq).items():
        if name != "state":
            cols[name] = col
    return {name: pad(col) for name, col in cols.items()}


def torch_batch_replays(seq) -> Dict[str, torch.Tensor]:
    return {k: torch.from_numpy(v) for k, v in batch_replays(seq).items()}


def rot180_batch(batch: Dict[str, torch.Tensor], mask) -> Dict[str, torch.Tensor]:
    """The rows of a padded batch (torch_batch_replays, DeviceReplayBuffer.sample) where `mask` is set, turned by 180
    degrees -- the one board symmetry of Hex that keeps each player's direction (game/hex.py:124-134 names it;
    HexGame.random_reflect itself stays the reference's identity).  board: the cell index reversed; legal_moves: every
    entry t > 0 becomes cells + 1 - t in its list position, zeros (padding) stay; moves_prob, color, result and
    reward are untouched, so moves_prob stays aligned by list position.  What the collate kernel does under
    DeviceReplayBuffer.random_reflect.  Works on CPU and device tensors; returns a new dict, the inputs are not
    modified."""
    board, moves = batch["board"], batch["legal_moves"]
    mask = torch.as_tensor(mask, device=board.device).to(torch.bool).reshape(-1)
    B = board.shape[0]
    if mask.shape[0] != B:
        raise ValueError("rot180_batch: mask has %d entries for %d rows" % (mask.shape[0], B))
    cells = board[0].numel() if B else 0
    out = dict(batch)
    if B == 0:
        return out
    turned = board.reshape(B, cells).flip(1).reshape(board.shape)
    out["board"] = torch.where(mask.reshape((B,) + (1,) * (board.dim() - 1)), turned, board)
    mapped = torch.where(moves > 0, (cells + 1) - moves, moves)
    out["legal_moves"] = torch.where(mask.to(moves.device).reshape(B, 1), mapped, moves)
    return out
