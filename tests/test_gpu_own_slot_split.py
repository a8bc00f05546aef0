"""The throughput sweep walks a stencil range that holds the bot's own slot as [lo, self) and (self, hi) instead of
testing every trip for it (pb_sweep.hpp), and roots the attraction magnitude without the clamp (pb_device.hpp).
Neither may change a bit: arenas built around the corner cases of the
split, both magnitude-sum modes, several steps, against the oracle.  Each arena's property is first checked on the CPU
from the oracle's own cell hashes (test_arena_has_its_property, no GPU)."""
import numpy as np
import pytest

from helpers import assert_bit_equal, jittered_blob, simparams_from_orc

CELL = 0.235
ARENAS = ("range_starts_at_self", "range_ends_at_self", "single_bot_cells", "left_its_stencil", "coincident_pair",
          "x_wrap", "payload")


@pytest.fixture(scope="module")
def orc():
    from oracle import orclib
    return orclib


def cells_of(P, pos):
    """(gx, gy) as calcGridPos computes them (float32 arithmetic)."""
    o = np.array([P.worldOriginX, P.worldOriginY], np.float32)
    c = np.array([P.cellSizeX, P.cellSizeY], np.float32)
    return np.floor((pos.astype(np.float32) - o) / c).astype(np.int64)


def sorted_slots(P, pos):
    """slot of every bot after the stable sort by cell hash, and the hash of every bot"""
    g = cells_of(P, pos)
    h = (g[:, 1] & (P.gridSizeY - 1)) * P.gridSizeX + (g[:, 0] & (P.gridSizeX - 1))
    order = np.argsort(h, kind="stable")
    slot = np.empty(len(h), np.int64)
    slot[order] = np.arange(len(h))
    return slot, h, g


def own_row_range(P, pos, i):
    """[lo, hi) in slots of bot i's own stencil row (cells gx-2 .. gx+2, no wrap) and its own slot"""
    slot, h, g = sorted_slots(P, pos)
    gx, gy = g[i]
    assert 2 <= gx < P.gridSizeX - 2
    row = (gy & (P.gridSizeY - 1)) * P.gridSizeX
    hs = np.sort(h)
    lo = np.searchsorted(hs, row + gx - 2, "left")
    hi = np.searchsorted(hs, row + gx + 2, "right")
    return int(lo), int(hi), int(slot[i])


def make_arena(orc, name):
    """(P, state, probe bots, steps checked).  Hand-placed bots sit on the cell grid: k cells from the origin."""
    n = 1200
    kw = dict(nCells=n, nDead=0, seed=77, phase_std=0.0, max_time=1e9, light_x=-3.0, light_y=0.5)
    if name == "payload":
        kw.update(nDead=-1, attractionFactor=0.5, massFactor=2.0)
    P = orc.default_params(**kw)
    rng = np.random.default_rng(4242)
    pos, vel, rad = jittered_blob(n, 0.158, rng, center=(5.3, -4.2), jitter=0.12)
    at = lambda cx, cy, fx=0.5, fy=0.5: (np.float32(P.worldOriginX + (cx + fx) * CELL), np.float32(P.worldOriginY + (cy + fy) * CELL))
    probes = []
    if name in ("range_starts_at_self", "range_ends_at_self"):
        # three bots in one row of cells, nothing else within the row's reach: the first one's own-row range starts
        # at its slot (cells gx-2, gx-1 empty), the last one's ends at its slot
        for k, cx in enumerate((200, 201, 202)):
            pos[k] = at(cx, 300)
            vel[k] = 0.0
        probes = [0] if name == "range_starts_at_self" else [2]
    elif name == "single_bot_cells":
        for k in range(40):  # a sparse lattice, 6 cells apart: every stencil holds the bot alone
            pos[k] = at(100 + 6 * (k % 8), 100 + 6 * (k // 8))
            vel[k] = 0.0
        probes = list(range(40))
    elif name == "left_its_stencil":
        pos[0] = at(150, 150)
        vel[0] = (14.0, 9.0)  # 0.14 per step: three cells from where it was sorted after 6 steps
        pos[1] = at(156, 154)  # someone to meet on the way
        vel[1] = 0.0
        probes = [0]
    elif name == "coincident_pair":
        pos[1] = pos[0]
        probes = [0, 1]
    elif name == "x_wrap":
        # cells 510, 511 | 0, 1 of a 512-cell row: the stencil rows of these bots split into two ranges
        for k, cx in enumerate((509, 510, 511, 511)):
            pos[k] = at(cx, 256, 0.3 + 0.1 * k, 0.5)
            vel[k] = 0.0
        probes = [1, 2, 3]
    steps = (1, 2, 12) if name == "left_its_stencil" else (1, 2, 8)
    return P, dict(pos=pos, vel=vel, rad=rad), probes, steps


@pytest.mark.parametrize("name", ARENAS)
def test_arena_has_its_property(orc, name):
    P, st, probes, steps = make_arena(orc, name)
    assert abs(P.cellSizeX - CELL) < 1e-6 and P.gridSizeX == 512
    pos = st["pos"]
    wall = P.wallHalf
    assert (np.abs(pos) < wall - 0.2).all()
    if name == "range_starts_at_self":
        lo, hi, me = own_row_range(P, pos, probes[0])
        assert lo == me and hi > me + 1
    elif name == "range_ends_at_self":
        lo, hi, me = own_row_range(P, pos, probes[0])
        assert hi == me + 1 and lo < me
    elif name == "single_bot_cells":
        for i in probes:
            lo, hi, me = own_row_range(P, pos, i)
            assert (lo, hi) == (me, me + 1)
    elif name == "left_its_stencil":
        # run the oracle: sorted at step 0 (sort_interval 180 steps), the bot ends more than two cells away from the
        # cell it was sorted into, in x and in y, so no row of its stencil holds its slot
        osim = orc.Sim(P, reset=True)
        for k, v in st.items():
            osim.set(k, v)
        g0 = cells_of(P, pos[:1])[0]
        osim.run(steps[-1])
        g1 = cells_of(P, osim.get("pos")[:1])[0]
        assert abs(g1[0] - g0[0]) > 2 and abs(g1[1] - g0[1]) > 2 and P.sort_interval > steps[-1]
    elif name == "coincident_pair":
        assert (pos[0] == pos[1]).all()
    elif name == "x_wrap":
        g = cells_of(P, pos[probes])
        assert ((g[:, 0] + 2 >= P.gridSizeX) | (g[:, 0] - 2 < 0)).all()
    elif name == "payload":
        assert P.nDead == -1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ARENAS)
def test_bit_identical_to_the_oracle(orc, name, mode):
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    P, state, probes, steps = make_arena(orc, name)
    osim = orc.Sim(P, reset=True)
    sp, keep = simparams_from_orc(P)
    gsim = pb.Sim(sp, keepalive=keep)
    gsim.set_lanes_per_bot(1)  # the throughput form, whatever the batch size
    gsim.set_force_variant(2)
    gsim.set_force_sums(mode)
    full = dict(pos=osim.get("pos"), vel=osim.get("vel"), rad=osim.get("rad"), phase=osim.get("phase"),
                dead=osim.get("dead"))
    full.update(state)
    for k, v in full.items():
        osim.set(k, v)
    gsim.set_state(**full)
    cfg = gsim.config()
    assert cfg["lanes_per_bot"] == 1 and cfg["attraction_sums"] == mode
    step = 0
    for upto in steps:
        osim.run(upto - step)
        assert gsim.step(upto - step) == upto - step
        step = upto
        st = gsim.get_state()
        keys = ("pos", "vel", "rad", "phase", "absForce_r") + (("absForce_a",) if mode == 1 else ())
        for key in keys:
            a, b = st[key], osim.get(key)
            both = np.isnan(a) & np.isnan(b)  # NaN payloads are not compared (the coincident pair)
            assert_bit_equal(np.where(both, 0, a).astype(a.dtype), np.where(both, 0, b).astype(b.dtype),
                             f"{name}, mode {mode}, step {upto}: {key}")


@pytest.mark.gpu
def test_unclamped_magnitude_root_equals_sqrtf_on_its_whole_domain():
    """pbRootNewtonPositive against sqrtf for every float of [2^-96, FLT_MAX): a superset of [2^-95, 2^99), what
    pbAttractionMagnitudeSafe (constants >= 2^-20) and pbFastMathAllowed (<= 2^30) let the both-sums form hand it."""
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    r = pb.self_test_magnitude_root()
    assert r["checked"] == 0x7F7FFFFF - 0x0F800000 and r["mismatches"] == 0, r
