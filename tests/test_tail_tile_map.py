"""The throughput grid's workgroup -> bots mapping with a split-lane tail (pbForceXcdTile, the function k_force
decodes its workgroup with): every bot of every XCD's share is covered exactly once, main tiles lead each XCD's
share and the tail workgroups -- the last ones dispatched on their XCD -- end it.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

TILE = 256


@pytest.fixture(scope="module")
def lib():
    from particlerobotsimulations_amd import _capi
    return _capi.lib()


def _lanes(lib):
    f, b = C.c_uint(), C.c_uint()
    assert lib.pbForceXcdTile(0, 1, 1, C.byref(f), C.byref(b)) == 0
    assert TILE % b.value == 0
    return TILE // b.value


@pytest.mark.parametrize("per_xcd", [1, 2, 9, 64, 489, 1000])
def test_every_slot_covered_once(lib, per_xcd):
    lanes = _lanes(lib)
    assert lanes >= 2
    f, b = C.c_uint(), C.c_uint()
    for tail in sorted({0, 1, per_xcd // 3, per_xcd // 2, 32 if per_xcd >= 32 else 0, per_xcd}):
        grid = 8 * (per_xcd + tail * (lanes - 1))
        cover = np.zeros(8 * per_xcd * TILE, np.int32)
        split = 0
        for wg in range(grid):
            assert lib.pbForceXcdTile(wg, per_xcd, tail, C.byref(f), C.byref(b)) == 0
            first, bots = f.value, b.value
            assert bots in (TILE, TILE // lanes)
            # the workgroup stays inside its XCD's contiguous share
            xcd = wg % 8
            assert xcd * per_xcd * TILE <= first and first + bots <= (xcd + 1) * per_xcd * TILE
            # main tiles first, tail workgroups at the end of the XCD's dispatch order
            assert (bots != TILE) == (wg // 8 >= per_xcd - tail), (wg, per_xcd, tail)
            split += bots != TILE
            cover[first:first + bots] += 1
        assert (cover == 1).all(), (per_xcd, tail)
        assert split == 8 * tail * lanes
        # one past the grid, and a tail longer than the share, are refused
        assert lib.pbForceXcdTile(grid, per_xcd, tail, C.byref(f), C.byref(b)) != 0
    assert lib.pbForceXcdTile(0, per_xcd, per_xcd + 1, C.byref(f), C.byref(b)) != 0
