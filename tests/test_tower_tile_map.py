"""The position-tile map of the fused split-f16 tower (azalea_amd/csrc/tower_tiles.h) through the host-only
debug export azx_debug_tower_tiles: which cell sits in which row of which 16-row tile, and which taps a wave skips for
its light tile.  No GPU: the bit-exactness of the kernel under the two maps is tests/test_gpu_tower_edge_tiles.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
SIZES = list(range(2, 12))
MAPS = ("edge", "rows")


def L():
    from azalea_amd import _lib
    return _lib.lib()


def tiles(n, name):
    rows = np.zeros(256, np.uint8)
    skip = np.zeros(4, np.uint32)
    slot = C.c_int32(-1)
    rc = L().azx_debug_tower_tiles(n, name.encode(), rows.ctypes.data_as(C.POINTER(C.c_uint8)),
                                   skip.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(slot))
    assert rc in (0, 1), (n, name, rc, L().azx_last_error())
    return rows.reshape(4, 4, 16).astype(np.int64), [int(s) for s in skip], slot.value, rc


def is_padding(n, lds_row, tap):
    """tap (3 * (dy + 1) + dx + 1) of LDS row 128 * board + cell reads no cell of the board."""
    cell = lds_row & 127
    if cell >= n * n:
        return True
    y, x = cell // n + tap // 3 - 1, cell % n + tap % 3 - 1
    return not (0 <= y < n and 0 <= x < n)


def test_the_header_declares_the_export_and_the_binding_requires_it():
    from azalea_amd import _lib
    text = open(os.path.join(ROOT, "include", "azx.h")).read()
    assert re.search(r"^int azx_debug_tower_tiles\(", text, re.M)
    assert "azx_debug_tower_tiles" in _lib.SYMBOLS and "azx_debug_tower_tiles" not in _lib.OPTIONAL
    assert L().azx_version() == 7
    assert EINVAL == int(re.search(r"AZX_EINVAL\s*=\s*(-?\d+)", text).group(1))


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("n", SIZES)
def test_the_map_is_a_permutation_that_holds_every_live_cell_once(n, name):
    rows, skip, slot, _ = tiles(n, name)
    assert sorted(rows.ravel().tolist()) == list(range(256))
    live = [r for r in rows.ravel().tolist() if (r & 127) < n * n]
    assert sorted(live) == [128 * b + c for b in range(2) for c in range(n * n)]
    assert 0 <= slot < 4                               # one slot index for all four waves
    assert all(0 <= s < 512 for s in skip)


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("n", SIZES)
def test_every_skipped_tap_is_padding_for_all_sixteen_rows_of_the_light_tile(n, name):
    rows, skip, slot, _ = tiles(n, name)
    for w in range(4):
        for tap in range(9):
            if skip[w] >> tap & 1:
                assert all(is_padding(n, int(r), tap) for r in rows[w, slot]), (n, name, w, tap)


@pytest.mark.parametrize("n", SIZES)
def test_rows_is_the_identity_with_nothing_skipped(n):
    rows, skip, slot, rc = tiles(n, "rows")
    assert rc == 0 and skip == [0, 0, 0, 0]
    assert np.array_equal(rows.ravel(), np.arange(256))       # 64 wh + 16 m + row on board wb = 128 wb + that


@pytest.mark.parametrize("n", SIZES)
def test_edge_gives_each_wave_one_edge_of_the_two_boards(n):
    """Waves 0..3: top row, bottom row, left column, right column (the columns without the corners), dead rows where
    the class is short; what the wave skips is at least its edge's three taps."""
    rows, skip, slot, rc = tiles(n, "edge")
    assert rc == 1                                     # 2..11 all reach 16 rows per class with dead rows
    want = ({0, 1, 2}, {6, 7, 8}, {0, 3, 6}, {2, 5, 8})
    for w in range(4):
        got = {t for t in range(9) if skip[w] >> t & 1}
        assert want[w] <= got, (n, w, got)
        for r in rows[w, slot].tolist():
            cell = r & 127
            if cell >= n * n:
                continue
            y, x = divmod(cell, n)
            assert (y == 0, y == n - 1, x == 0 and 0 < y < n - 1, x == n - 1 and 0 < y < n - 1)[w], (n, w, r)
        # a class that has 16 cells on the two boards fills its tile without a dead row
        size = 2 * n if w < 2 else 2 * (n - 2)
        nlive = sum(1 for r in rows[w, slot].tolist() if (r & 127) < n * n)
        assert nlive == min(16, size), (n, w, nlive)


def test_the_headline_board():
    rows, skip, slot, rc = tiles(11, "edge")
    assert rc == 1
    assert [{t for t in range(9) if s >> t & 1} for s in skip] == [{0, 1, 2}, {6, 7, 8}, {0, 3, 6}, {2, 5, 8}]
    for w in range(4):
        assert all((r & 127) < 121 for r in rows[w, slot].tolist())          # 16 live cells
        boards = {r >> 7 for r in rows[w, slot].tolist()}
        assert boards == {0, 1}                                              # of both boards
    # per block and layer 4 waves x 3 taps x 2 k-steps x 12 MFMAs fewer: 41 696 -> 38 240 over 12 layers
    per_layer = sum(bin(s).count("1") for s in skip) * 2 * 12
    assert per_layer == 288 and 41696 - 12 * per_layer == 38240


def test_the_map_is_deterministic_and_bad_arguments_are_refused():
    a, b = tiles(11, "edge"), tiles(11, "edge")
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]
    f = L().azx_debug_tower_tiles
    rows = (C.c_uint8 * 256)()
    skip = (C.c_uint32 * 4)()
    slot = C.c_int32()
    for n in (1, 0, -3, 12, 13):
        assert f(n, b"edge", rows, skip, C.byref(slot)) == EINVAL and b"board size" in L().azx_last_error()
    assert f(11, b"columns", rows, skip, C.byref(slot)) == EINVAL and b"neither" in L().azx_last_error()
    assert f(11, None, rows, skip, C.byref(slot)) == EINVAL
    assert f(11, b"edge", None, skip, C.byref(slot)) == EINVAL
