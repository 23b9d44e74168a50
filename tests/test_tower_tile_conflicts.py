"""LDS bank conflicts of the fused split-f16 tower's position tiles, scored on the CPU with the key model of
azalea_amd/csrc/tower_tiles.h (restated here) through the host-only export azx_debug_tower_tiles.

The block's LDS image holds board 1 eight rows behind board 0's 128: LDS row of a table entry L = L + 8 * (L >> 7).  An
LDS row starts on slot (row mod 16); ds_read_b128 serves a wave in groups of 16 lanes that mix the tile rows {4-7, 12-15}
of one k-group with the rows {0-3, 8-11} of the next, 8 slots further.  Two rows of a tile on one key share their banks.
Score = for each tile and key kind, the rows beyond the first on a key, summed."""
import ctypes as C

import numpy as np
import pytest

SIZES = list(range(2, 12))
# the builder before this one on its own layout (boards 128 rows apart), measured with this score
PARENT_SCORE = {2: 24, 3: 50, 4: 50, 5: 54, 6: 64, 7: 68, 8: 100, 9: 88, 10: 88}


def tiles(n, name):
    from azalea_amd import _lib
    rows = np.zeros(256, np.uint8)
    skip = np.zeros(4, np.uint32)
    slot = C.c_int32(-1)
    rc = _lib.lib().azx_debug_tower_tiles(n, name.encode(), rows.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          skip.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(slot))
    assert rc in (0, 1), (n, name, rc)
    return rows.reshape(16, 16).astype(np.int64)


def lds_row(entry):
    return entry + 8 * (entry >> 7)


def slot_keys(row, tile_row):
    a = (tile_row & 4) == 0                                # tile rows {0-3, 8-11}
    return (row + (8 if a else 0)) & 15, (row + (0 if a else 8)) & 15


def score(table):
    total = 0
    for tile in table:
        for kind in range(2):
            keys = [slot_keys(lds_row(int(e)), r)[kind] for r, e in enumerate(tile)]
            total += len(keys) - len(set(keys))
    return total


def test_the_headline_board_has_no_conflict_and_every_tile_is_a_full_residue_system():
    table = tiles(11, "edge")
    assert score(table) == 0
    for t, tile in enumerate(table):
        assert sorted(lds_row(int(e)) & 15 for e in tile) == list(range(16)), t


@pytest.mark.parametrize("n", sorted(PARENT_SCORE))
def test_smaller_boards_score_no_higher_than_the_builder_before(n):
    got = score(tiles(n, "edge"))
    print("N = %d: score %d (before: %d)" % (n, got, PARENT_SCORE[n]))
    assert got <= PARENT_SCORE[n]


@pytest.mark.parametrize("n", SIZES)
def test_rows_scores_zero(n):
    assert score(tiles(n, "rows")) == 0


@pytest.mark.parametrize("name", ("edge", "rows"))
@pytest.mark.parametrize("n", SIZES)
def test_no_allowed_tap_reaches_the_gap_rows_or_the_other_board(n, name):
    """A tap the kernel's `tapok` allows (the lane's cell is live and the neighbour is on the board) addresses LDS row
    (own row + dy * N + dx): for every live cell of either board that is a live row of the same board, never one of
    the rows 128..135 between the boards."""
    table = tiles(n, name)
    live = 0
    for e in table.ravel().tolist():
        board, cell = e >> 7, e & 127
        if cell >= n * n:
            continue
        live += 1
        y, x = divmod(cell, n)
        for tap in range(9):
            dy, dx = tap // 3 - 1, tap % 3 - 1
            if not (0 <= y + dy < n and 0 <= x + dx < n):
                continue                                   # padding: the kernel reads the zero rows instead
            target = lds_row(e) + dy * n + dx
            lo = 136 * board
            assert lo <= target < lo + n * n, (n, name, e, tap, target)
            assert not 128 <= target < 136
    assert live == 2 * n * n
