"""The inputs of the grid-geometry tests (tests/test_grid_geometry_ref.py on the CPU, tests/test_gpu_grid_geometry.py
on the device): a jittered blob under each geometry of helpers.GEOMETRIES, the preconditions that make a geometry
exercise what it is there for (computed from the oracle's orc_calcHash alone), and the oracle's snapshots, run once per
(geometry, n) and shared by every kernel form."""
import ctypes as C
import functools

import numpy as np

from helpers import GEOMETRIES, geometry, jittered_blob, with_geometry, wrap_centre

SNAP_STEPS = (1, 2, 60, 260)
SORT_INTERVAL = 0.5          # 260 steps of 0.01: a re-sort at the start and at 0.5, 1.0, 1.5, 2.0, 2.5
STATE_KEYS = ("pos", "vel", "rad", "phase", "absForce_a", "absForce_r")
FIT_N = 64                   # g8fit's arena is 8 x 8 cells of 0.235: room for 64 bots and no more


def case_params(orc, name, n, **kw):
    base = dict(nCells=n, nDead=0, seed=5, phase_std=0.4, max_time=1e9, light_x=-4.0, light_y=1.0)
    base.update(kw)
    return geometry(orc.default_params(**base), name)


def blob_centre(name, P):
    """g8fit: the 9 x 8 bots reach to within a cell of the left and right walls, which are the wraps, from the middle;
    moved up by 0.4 they reach to within a fifth of a cell of the upper one as well.  Everywhere else a crossing of an
    x-wrap and a y-wrap line.  r8x64 and r64x8 get the same point, a wrap line of the 64-cell period on both axes
    (which is one of the 8-cell period too): the same state for both"""
    if name == "g8fit":
        return (0.0, 0.4)
    if name in ("r8x64", "r64x8"):
        return wrap_centre(with_geometry(P, 64, 64))
    return wrap_centre(P)


@functools.lru_cache(maxsize=None)
def case(name, n):
    """(P, pos, vel, rad) of the named geometry: shared, read-only"""
    from oracle import orclib as orc
    P = case_params(orc, name, n)
    rng = np.random.default_rng(1000 + n)
    pos, vel, rad = jittered_blob(n, 0.16, rng, center=blob_centre(name, P))
    for a in (pos, vel, rad):
        a.setflags(write=False)
    return P, pos, vel, rad


def cells(orc, P, pos):
    """(cx, cy) of every bot: the oracle's orc_calcHash, taken apart"""
    n = len(pos)
    h, idx = np.empty(n, np.uint32), np.empty(n, np.uint32)
    orc.lib().orc_calcHash(C.byref(P), h, idx, np.ascontiguousarray(pos, np.float32).reshape(-1), n)
    h = h.astype(np.int64)
    assert (h < int(P.numCells)).all()
    return h % int(P.gridSizeX), h // int(P.gridSizeX)


def wrap_fractions(orc, P, pos):
    """the share of bots whose 5 x 5 stencil wraps in x, and in y"""
    cx, cy = cells(orc, P, pos)
    gx, gy = int(P.gridSizeX), int(P.gridSizeY)
    return float(((cx < 2) | (cx >= gx - 2)).mean()), float(((cy < 2) | (cy >= gy - 2)).mean())


def widest_cell_spread(orc, P, pos):
    """the largest distance, per axis, between two bots that share a cell: (dx, dy) in world units"""
    cx, cy = cells(orc, P, pos)
    h = cy * int(P.gridSizeX) + cx
    p = np.asarray(pos, np.float64)
    out = []
    for axis in (0, 1):
        lo, hi = np.full(int(P.numCells), np.inf), np.full(int(P.numCells), -np.inf)
        np.minimum.at(lo, h, p[:, axis])
        np.maximum.at(hi, h, p[:, axis])
        filled = np.isfinite(lo)
        out.append(float((hi[filled] - lo[filled]).max()))
    return tuple(out)


def key_bits(num_keys):
    b = 0
    while b < 32 and num_keys > (1 << b):
        b += 1
    return max(b, 1)


def sort_passes(P, nsims=1):
    """8-bit radix passes of the engine's re-sort: the cell bits, and the member bits of a batch on top"""
    bits = key_bits(int(P.numCells)) + (key_bits(nsims) if nsims > 1 else 0)
    return -(-bits // 8)


PASSES = {"g8": 1, "g8fit": 1, "g16": 1, "g32": 2}


def check_preconditions(orc, name, P, pos):
    """What each geometry claims to exercise, asserted from the cells alone (no device): a case that fails here has
    silently stopped testing what it is there for."""
    n = len(pos)
    fx, fy = wrap_fractions(orc, P, pos)
    if name != "g8fit" and n >= 64:
        # an 8-wide axis: half of its columns have a wrapping stencil; a blob far wider than 8 cells fills them evenly
        if int(P.gridSizeX) == 8:
            assert fx >= 0.25, (name, fx)
        if int(P.gridSizeY) == 8:
            assert fy >= 0.25, (name, fy)
        # every other axis: the 33 x 33-bot blob spans at most 24 cells and lies across the wrap line, 4 of those
        # columns wrap: a sixth of the bots; a twelfth is asked for
        assert fx >= 1.0 / 12 and fy >= 1.0 / 12, (name, fx, fy)
    dx, dy = widest_cell_spread(orc, P, pos)
    if name == "g8" and n >= 1024:   # (the small blobs of g8 are narrower than the grid)
        assert max(dx / float(P.cellSizeX), dy / float(P.cellSizeY)) > 3.0      # aliased bots share a cell
    if name == "g8fit":
        assert n <= FIT_N and np.hypot(dx, dy) <= np.hypot(float(P.cellSizeX), float(P.cellSizeY))   # nothing aliases
        assert fx > 0 and fy > 0
    if name in PASSES:
        assert sort_passes(P) == PASSES[name], (name, sort_passes(P))


def snapshot(osim):
    return {k: osim.get(k) for k in STATE_KEYS}


@functools.lru_cache(maxsize=None)
def oracle_snapshots(name, n):
    """the oracle's state after SNAP_STEPS steps from case(name, n), phases 0, nobody dead: run once, read-only"""
    from oracle import orclib as orc
    P, pos, vel, rad = case(name, n)
    osim = orc.Sim(P, reset=False)
    for key, a in (("pos", pos), ("vel", vel), ("rad", rad), ("phase", np.zeros(n, np.float32)),
                   ("dead", np.zeros(n, np.int32))):
        osim.set(key, a)
    out, step = {}, 0
    for k in SNAP_STEPS:
        assert osim.run(k - step, sort_interval=SORT_INTERVAL)
        step = k
        out[k] = snapshot(osim)
    osim.close()
    return out


__all__ = ["GEOMETRIES", "SNAP_STEPS", "SORT_INTERVAL", "STATE_KEYS", "FIT_N", "case", "case_params", "cells",
           "check_preconditions", "oracle_snapshots", "sort_passes", "snapshot", "wrap_fractions",
           "widest_cell_spread", "blob_centre"]
