"""Small, rectangular and anisotropic grids without a GPU: the inputs of tests/test_gpu_grid_geometry.py can tell x
from y (a kernel that swapped gridX / gridY, cellX / cellY or originX / originY would not pass on them), the helper
that builds them round-trips into SimParams, the preconditions of every geometry hold, and pbSimCreate[Batch]'s
argument checks accept and refuse the right grids."""
import ctypes as C

import numpy as np
import pytest

import geometry_cases as gc
import stream_ref as sr
from helpers import GEOMETRIES, simparams_from_orc, with_geometry

SWAPS = (("gridSizeX", "gridSizeY"), ("cellSizeX", "cellSizeY"), ("worldOriginX", "worldOriginY"))
RECTANGULAR = ("r8x64", "r64x8", "r16x512", "aniso")


def swapped(P, a, b):
    Q = type(P).from_buffer_copy(P)
    va, vb = getattr(P, a), getattr(P, b)
    setattr(Q, a, vb), setattr(Q, b, va)
    return Q


def bots_with_other_candidates(orc, P, Q, pos):
    n = len(pos)
    codes = []
    for R in (P, Q):
        i, j = sr.candidate_pairs(orc, R, pos)
        codes.append(np.unique(i * n + j))
    return np.unique(np.setxor1d(codes[0], codes[1], assume_unique=True) // n).size


def one_step(orc, P, pos, vel, rad):
    n = len(rad)
    osim = orc.Sim(P, reset=False)
    for key, a in (("pos", pos), ("vel", vel), ("rad", rad), ("phase", np.zeros(n, np.float32)),
                   ("dead", np.zeros(n, np.int32))):
        osim.set(key, a)
    assert osim.run(1, sort_interval=gc.SORT_INTERVAL)
    out = gc.snapshot(osim)
    osim.close()
    return out


@pytest.mark.parametrize("name", RECTANGULAR)
def test_inputs_tell_x_from_y(orc, name):
    """Under each pair of fields swapped (where the two differ: a rectangular grid with the default cell has only its
    gridSize to swap) at least half of the bots get another candidate set, and one oracle step gives other bits."""
    P, pos, vel, rad = gc.case(name, 1025)
    true = one_step(orc, P, pos, vel, rad)
    tried = 0
    for a, b in SWAPS:
        if getattr(P, a) == getattr(P, b):
            continue
        tried += 1
        Q = swapped(P, a, b)
        assert bots_with_other_candidates(orc, P, Q, pos) >= len(pos) // 2 + 1, (name, a)
        other = one_step(orc, Q, pos, vel, rad)
        assert not np.array_equal(other["vel"].view(np.uint32), true["vel"].view(np.uint32)), (name, a)
        assert not np.array_equal(other["absForce_a"].view(np.uint32), true["absForce_a"].view(np.uint32)), (name, a)
    assert tried == (3 if name == "aniso" else 1)


def test_both_orientations_see_the_same_state(orc):
    """r8x64 and r64x8 are run from the same bots: a swap of gridX / gridY survives in neither"""
    a, b = gc.case("r8x64", 1025), gc.case("r64x8", 1025)
    for k in (1, 2, 3):
        assert np.array_equal(a[k], b[k])
    assert (a[0].gridSizeX, a[0].gridSizeY) == (b[0].gridSizeY, b[0].gridSizeX) == (8, 64)


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_with_geometry_round_trips(orc, name):
    P = gc.case_params(orc, name, 10)
    gx, gy, cell, origin, wall = GEOMETRIES[name]
    assert (P.gridSizeX, P.gridSizeY, P.numCells) == (gx, gy, gx * gy)
    if cell is not None:
        assert (P.cellSizeX, P.cellSizeY) == tuple(np.float32(cell))
    else:
        assert P.cellSizeX == P.cellSizeY == np.float32(2 * float(P.max_radius))
    if name == "g8fit":
        assert P.worldOriginX == P.worldOriginY == -P.wallHalf == np.float32(-4) * np.float32(P.cellSizeX)
    elif origin is not None:
        assert (P.worldOriginX, P.worldOriginY) == tuple(np.float32(origin)) and P.wallHalf == 64.0
    else:
        assert P.worldOriginX == P.worldOriginY == -64.0 and P.wallHalf == 64.0
    sp, keep = simparams_from_orc(P)
    assert (sp.gridSize.x, sp.gridSize.y, sp.numCells) == (P.gridSizeX, P.gridSizeY, P.numCells)
    assert (sp.cellSize.x, sp.cellSize.y) == (P.cellSizeX, P.cellSizeY)
    assert (sp.worldOrigin.x, sp.worldOrigin.y) == (P.worldOriginX, P.worldOriginY)
    # a copy: the parameters it was made from keep their square default
    base = orc.default_params(nCells=10)
    Q = with_geometry(base, 8, 64, wall_half=3.0)
    assert (base.gridSizeX, base.gridSizeY, base.numCells, base.wallHalf) == (512, 512, 512 * 512, 64.0)
    assert (Q.gridSizeX, Q.gridSizeY, Q.numCells, Q.wallHalf) == (8, 64, 512, 3.0)


@pytest.mark.parametrize("name,n", [(g, n) for g in sorted(GEOMETRIES) for n in ((gc.FIT_N,) if g == "g8fit" else (1024, 1025))]
                         + [("g8", n) for n in (1, 2, 65, 257)])
def test_preconditions_of_every_case(orc, name, n):
    P, pos, vel, rad = gc.case(name, n)
    gc.check_preconditions(orc, name, P, pos)
    w = float(P.wallHalf)
    assert (np.abs(pos) < w).all()      # inside the walls from the start


def test_pass_counts(orc):
    """one, one, one and two passes on the small squares; two for a pair of 16 x 16 members, one for three 8 x 8
    members, four for five members on 2048^2; three on everything the rest of the suite runs"""
    for name, want in gc.PASSES.items():
        assert gc.sort_passes(gc.case_params(orc, name, 10)) == want
    assert gc.sort_passes(gc.case_params(orc, "g8", 10), 3) == 1
    assert gc.sort_passes(gc.case_params(orc, "g16", 10), 2) == 2
    big = orc.default_params(nCells=10, grid=2048, arena_half=240.0)
    assert gc.sort_passes(big, 5) == 4 and gc.sort_passes(big, 4) == 3
    for grid in (512, 2048, 4096):
        assert gc.sort_passes(orc.default_params(nCells=10, grid=grid)) == 3


def test_create_checks_on_small_and_rectangular_grids():
    import torch

    from particlerobotsimulations_amd import _capi as capi
    L = capi.lib()
    h = C.c_void_p()

    def params(gx, gy, num_cells=None):
        return capi.make_params({"gridSize": (gx, gy), "numCells": gx * gy if num_cells is None else num_cells,
                                 "nCells": 10, "cellSize": (0.235, 0.235), "worldOrigin": (-64.0, -64.0)})

    for gx, gy, cells in ((4, 8, None), (8, 4, None), (8, 12, None), (8, 8, 63)):
        p, keep = params(gx, gy, cells)
        assert L.pbSimCreate(C.byref(h), C.byref(p), 0.0) == 2, (gx, gy)         # PB_ERR_ARG
        assert b"power of two" in L.pbGetLastErrorString() and not h.value
    for gx, gy in ((8, 8), (8, 64), (64, 8)):
        p, keep = params(gx, gy)
        if not torch.cuda.is_available():
            assert L.pbSimCreate(C.byref(h), C.byref(p), 0.0) == 3, (gx, gy)     # PB_ERR_NO_DEVICE: the checks passed
            assert b"no HIP device" in L.pbGetLastErrorString() and not h.value
    # a batch whose members differ in gridSize.y alone (numCells is only checked against the grid for member 0)
    a, ka = params(8, 8)
    b, kb = params(8, 16, 64)
    arr = (capi.SimParams * 2)(a, b)
    assert L.pbSimCreateBatch(C.byref(h), arr, 2, 0.0) == 2 and b"must share" in L.pbGetLastErrorString()
    b2, kb2 = params(16, 8, 64)
    arr = (capi.SimParams * 2)(a, b2)
    assert L.pbSimCreateBatch(C.byref(h), arr, 2, 0.0) == 2 and b"must share" in L.pbGetLastErrorString()
