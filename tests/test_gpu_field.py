"""GPU: the field maps (pbSimFieldMap / pbSimFieldMapOf, csrc/pb_field.hip) against tests/field_ref.py on states read
back from the device.  Every comparison is exact equality of every field of every cell and of the totals.
tests/test_field_api.py pins the reference to a plain loop and to known answers on the CPU, and shows that the recipes
used here keep every bot measured, and inside where a test says so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import field_ref as FR
from helpers import assert_bit_equal
from test_field_api import (BATCH, LATTICE_BOTS, OFF_CENTRE, WAVE_BOTS, covering_view, dead_flags, half_view,
                            known_answer, lattice_state, minus_zero_answer)
from test_gpu_series import layout_of, make_batch, sim_with
from test_series_api import SIZES, recipe, unmeasured_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
DT = 0.01


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def with_dead(sim, dead):
    st = sim.get_state()
    sim.set_state(pos=st["pos"], vel=st["vel"], rad=st["rad"], phase=st["phase"], dead=np.asarray(dead, np.int32))
    return sim


def device_map(sim, view, member=None):
    cells, totals = sim.field_map(view["nx"], view["ny"], view["center"], view["half"], member=member)
    assert cells.dtype.itemsize == 64 and cells.shape[-2:] == (view["ny"], view["nx"])
    assert (cells["rr_lo"] < 1 << 32).all() and (cells["vv_lo"] < 1 << 32).all()  # normalised by the host
    return cells, totals


def check_map(sim, view, what, member=0, state=None, of=False):
    """One member's map of the state as it is now against the reference on the state read back; returns the reference."""
    st = state if state is not None else sim.get_state()
    want, want_tot = FR.field_map(st["pos"], st["vel"], st["rad"], st["dead"], **view)
    if of:
        cells, tot = device_map(sim, view, member=member)
    else:
        cells, tot = device_map(sim, view)
        cells, tot = cells[member], tot[member]
    got = FR.from_device(cells)
    print(what, tot, sum(1 for row in got for c in row if c["count"]), "cells hold bots")
    assert tot == want_tot, (what, tot, want_tot)
    if got != want:
        bad = [(iy, ix, got[iy][ix], want[iy][ix]) for iy in range(view["ny"]) for ix in range(view["nx"])
               if got[iy][ix] != want[iy][ix]]
        raise AssertionError((what, len(bad), bad[:3]))
    return want, want_tot


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_wave_and_the_workgroup(pb, orc, n):
    pos, vel, rad = recipe(n)
    sim = with_dead(sim_with(pb, orc, pos, vel, rad), dead_flags(n))
    st = sim.get_state()
    assert_bit_equal(st["pos"], pos, "pos")
    assert_bit_equal(st["vel"], vel, "vel")
    want, tot = check_map(sim, covering_view(pos, 8, 8), f"n {n} 8x8", state=st)
    assert tot == {"measured": n, "inside": n, "outside": 0, "unmeasured": 0}
    assert sum(c["dead"] for row in want for c in row) == int(dead_flags(n).sum())
    # the whole wave in one key, against the moments row of the same state: a cross-check with existing code
    want, tot = check_map(sim, covering_view(pos, 1, 1), f"n {n} 1x1", state=st)
    row, c = sim.moments()[0], want[0][0]
    assert (c["count"], c["sum_qr"], c["sum_wx"], c["sum_wy"], c["rr"], c["vv"]) == tuple(
        row[k] for k in ("measured", "sum_qr", "sum_wx", "sum_wy", "rr", "vv"))
    assert c["count"] == n


def test_every_lane_a_cell_of_its_own(pb, orc):
    pos, vel, rad = recipe(257)
    sim = with_dead(sim_with(pb, orc, pos, vel, rad), dead_flags(257))
    want, tot = check_map(sim, covering_view(pos, 1024, 1024), "257 on 1024x1024", of=True)
    assert tot["inside"] == 257 and sum(1 for row in want for c in row if c["count"]) >= 250


def test_off_centre_view_with_unequal_half_extents(pb, orc):
    pos, vel, rad = recipe(300)
    sim = with_dead(sim_with(pb, orc, pos, vel, rad), dead_flags(300))
    want, tot = check_map(sim, OFF_CENTRE, "5x3 off centre")
    assert tot["outside"] > 0 and tot["inside"] > 100
    counts = np.array([[c["count"] for c in row] for row in want])
    assert not np.array_equal(counts, counts[::-1]) and not np.array_equal(counts, counts[:, ::-1])
    # a view covering half the blob: outside is counted and nothing lands in the edge cells by clamping
    view = half_view(pos)
    want, tot = check_map(sim, view, "half the blob")
    assert tot["inside"] > 75 and tot["outside"] > 75 and tot["measured"] == 300
    assert sum(c["count"] for row in want for c in row) == tot["inside"]


def test_known_answers_set_with_set_state(pb, orc):
    for name, ((pos, vel, rad, dead), view, cells, totals) in (("four bots", known_answer()),
                                                              ("minus zero", minus_zero_answer())):
        sim = with_dead(sim_with(pb, orc, pos, vel, rad), dead)
        st = sim.get_state()
        for k, a in (("pos", pos), ("vel", vel), ("rad", rad)):
            assert_bit_equal(st[k], a, k)  # the sign of -0.0f survives the round trip
        assert check_map(sim, view, name, state=st, of=True) == (cells, totals)
        assert check_map(sim, view, name, state=st) == (cells, totals)


def test_unmeasured_bots_of_every_kind(pb, orc):
    pos, vel, rad, bad = unmeasured_state()
    sim = sim_with(pb, orc, pos, vel, rad)
    _, tot = check_map(sim, covering_view(recipe(257)[0], 8, 8), "unmeasured")
    assert tot["unmeasured"] == len(bad) == 25 and tot["measured"] == 232 and tot["outside"] >= 1


def test_more_bots_than_one_pass_of_the_launch_covers(pb, orc):
    pos, vel, rad = lattice_state()
    sim = with_dead(sim_with(pb, orc, pos, vel, rad), dead_flags(LATTICE_BOTS))
    want, tot = check_map(sim, covering_view(pos, 32, 32), "lattice 32x32", of=True)
    assert tot["inside"] == LATTICE_BOTS and max(c["rr"] for row in want for c in row) > 1 << 36


def test_batch_of_three_members_do_not_leak_into_each_other(pb, orc):
    members, n = BATCH
    ens = make_batch(pb, orc, members, n)
    states = [ens.get_state_of(k) for k in range(members)]
    view = dict(nx=8, ny=6, center=(2.0, -2.0), half=(6.5, 5.0))  # all three blobs, each in a place of its own
    cells, totals = device_map(ens, view)
    assert cells.shape == (members, 6, 8) and len(totals) == members
    maps = []
    for k in range(members):
        want, want_tot = FR.field_map(states[k]["pos"], states[k]["vel"], states[k]["rad"], states[k]["dead"], **view)
        assert FR.from_device(cells[k]) == want and totals[k] == want_tot, k
        of_cells, of_tot = device_map(ens, view, member=k)  # Of equals the member's slice
        assert np.array_equal(of_cells, cells[k]) and of_tot == totals[k]
        assert want_tot["inside"] > n // 2
        maps.append(want)
    assert maps[0] != maps[1] != maps[2]
    with pytest.raises(RuntimeError, match="code 2.*pbSimFieldMapOf.*member out of range"):
        ens.field_map(8, 6, (0.0, 0.0), 4.0, member=members)
    again, _ = device_map(ens, view)
    assert np.array_equal(again, cells)  # twice: the same map


@pytest.fixture(scope="module")
def wave_sim(pb, orc):
    """5 000 bots under light-wave control, a quarter of them dead."""
    pos, vel, rad = recipe(WAVE_BOTS)
    sim = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0, phase_update_interval=0.3)  # LIGHT_WAVE
    return with_dead(sim, dead_flags(WAVE_BOTS))


def test_map_before_and_after_stepping_with_resorts(wave_sim):
    sim = wave_sim
    view = covering_view(recipe(WAVE_BOTS)[0], 24, 20)
    before, _ = check_map(sim, view, "before the steps")
    assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    lay = layout_of(sim)
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(WAVE_BOTS))  # sorted: the slots are not in original order
    after, tot = check_map(sim, view, "after 60 steps")
    assert after != before and tot["measured"] == WAVE_BOTS
    assert 0 < sum(c["dead"] for row in after for c in row) < tot["inside"]


def test_a_map_changes_nothing(wave_sim):
    sim = wave_sim
    if sim.stats()["steps"] == 0:
        assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    before, stats, lay, t = sim.get_state(), sim.stats(), layout_of(sim), sim.time
    maps0, _ = sim.field_times()
    view = covering_view(before["pos"], 16, 16)
    first, tot = device_map(sim, view)
    again, _ = device_map(sim, view, member=0)
    assert np.array_equal(first[0], again)
    after = sim.get_state()
    for k in before:
        assert_bit_equal(before[k], after[k], k)
    assert sim.stats() == stats and sim.time == t
    for a, b in zip(lay, layout_of(sim)):
        assert np.array_equal(a, b)
    n, ms = sim.field_times()
    assert n == maps0 + 2 and ms > 0.0
    assert sim.step(5, dt=DT, sort_interval=0.2) == 5  # and the engine steps on


def live_memory():
    from particlerobotsimulations_amd import _capi
    buffers, nbytes = C.c_ulonglong(0), C.c_ulonglong(0)
    _capi.check(_capi.lib().pbDeviceMemoryLive(C.byref(buffers), C.byref(nbytes)), "pbDeviceMemoryLive")
    return int(buffers.value), int(nbytes.value)


def test_scratch_grows_and_is_given_back(pb, orc):
    start = live_memory()
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad)
    made = live_memory()
    assert sim.field_times() == (0, 0.0) and live_memory() == made  # nothing is allocated until a map is asked for
    small = check_map(sim, covering_view(pos, 8, 8), "8x8")
    one = live_memory()
    assert one[0] == made[0] + 2 and one[1] == made[1] + 8 * 8 * 64 + 16
    check_map(sim, covering_view(pos, 64, 64), "64x64")
    two = live_memory()
    assert two[0] == one[0] and two[1] == made[1] + 64 * 64 * 64 + 16
    assert check_map(sim, covering_view(pos, 8, 8), "8x8 again") == small  # the larger scratch is zeroed as far as it is used
    assert live_memory() == two
    sim.close()
    assert live_memory() == start


def test_argument_errors_on_a_live_batch(pb, orc):
    ens = make_batch(pb, orc, 33, 65)
    before = live_memory()
    with pytest.raises(RuntimeError, match="code 2.*pbSimFieldMap.*2\\^31 bytes"):
        ens.field_map(1024, 1024, (0.0, 0.0), 4.0)  # 33 x 2^20 x 64 bytes; 32 members would be 2^31 exactly
    assert live_memory() == before
    cells, tot = ens.field_map(1024, 1024, (0.0, 0.0), 4.0, member=32)  # one member of it is counted as one
    assert cells.shape == (1024, 1024) and int(cells["count"].sum()) == tot["inside"]
    before = live_memory()
    for bad in (dict(nx=0, ny=8, center=(0.0, 0.0), half=1.0), dict(nx=8, ny=8, center=(0.0, 0.0), half=(1.0, 0.0)),
                dict(nx=8, ny=8, center=(float("nan"), 0.0), half=1.0)):
        with pytest.raises(RuntimeError, match="code 2.*pbSimFieldMap"):
            ens.field_map(**bad)
    assert live_memory() == before and ens.field_times()[0] == 1  # the refused calls computed nothing


# ---- the runner ------------------------------------------------------------------------------------------------------

HEADER = "time,step,ix,iy,count,dead,sum_qr,sum_wx,sum_wy,rr,vv"


def block_of(time, step, cells):
    lines = []
    for iy, row in enumerate(cells):
        for ix, c in enumerate(row):
            if c["count"]:
                lines.append(",".join(["%.9g" % time, str(step), str(ix), str(iy)] +
                                      [str(c[k]) for k in FR.CELL_FIELDS]))
    return lines


# the example as the issue runs it (dump_interval 60: the one block at time 0), and with a dump row every 0.5 s
@pytest.mark.parametrize("extra", [{}, {"dump_interval": "0.5"}], ids=["as_written", "dump_0.5"])
def test_runner_writes_a_block_at_every_dump_time(tmp_path, extra):
    from particlerobotsimulations_amd import host
    over = dict(max_time="2", **extra)
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--field", "f.csv", "--field-cells", "16"], capture_output=True,
                       text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "f.csv").read().splitlines()
    assert lines[0] == HEADER
    # the same blocks from the class driven in-process, stopped at the same steps
    flat = host.load_config(CFG, **over)
    di = f32(flat.dump_interval)

    def due(t):  # the gate of dumpParticlebot, in its fp32 operations
        t = f32(t)
        return not (t - di * np.floor(t / di) > f32(0.01))

    h = host.HostSim(CFG, engine="fused", **over)
    want, steps, blocks = [], 0, 0
    while True:
        if due(h.time):
            cells, totals = h.field_map(16, 16, (0.0, 0.0), flat.wallHalf, member=0)
            assert totals["inside"] == 300
            want += block_of(h.time, steps, FR.from_device(cells))
            blocks += 1
        if h.finished:
            break
        ran = h.advance(h.steps_until_dump())
        if ran == 0:
            break
        steps += ran
    assert blocks >= (4 if extra else 1), blocks  # (the dump gate holds at time 0 and again one step later)
    assert lines[1:] == want and len(want) >= 2 * blocks
    assert len({l.split(",")[1] for l in lines[1:]}) == blocks
    h.close()
