"""GPU: the structure factor (pbSimStructureFactor / pbSimStructureFactorOf, csrc/pb_sfactor.hip) against
tests/sfactor_ref.py on states read back from the device.  Every comparison is exact equality of every integer of every
row.  tests/test_sfactor_ref.py pins the reference to a plain loop, to known answers and to the derived bound of a
float64 evaluation on the CPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import sfactor_ref as KR
from helpers import assert_bit_equal
from test_field_api import LATTICE_BOTS, lattice_state
from test_gpu_series import layout_of, make_batch, sim_with
from test_series_api import BELOW, recipe, unmeasured_state
from test_sfactor_ref import ALIAS, ONE, lattice

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
DT = 0.01
# 17 vectors: the origin, both axes, both signs, large integers, and the aliasing pair of the CPU test
V17 = [(0, 0), (1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (3, -5), (-7, 2), (16, 16), (40, 17), (-1280, 999), (255, -256),
       (65536, 1), (-65537, 65535), ALIAS, (-2 ** 31, 2 ** 31 - 1), (12345678, -87654321)]
assert len(V17) == 17


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def check(sim, vectors, e, kind, what, member=0, state=None, of=False):
    """One member's rows of the state as it is now against the reference on the state read back; returns the reference."""
    st = state if state is not None else sim.get_state()
    want = KR.structure_factor(st["pos"], st["vel"], st["rad"], vectors, e, kind)
    if of:
        rows = sim.structure_factor(vectors, e, kind=kind, member=member)
    else:
        rows = sim.structure_factor(vectors, e, kind=kind)[member]
    assert rows.dtype.itemsize == 80 and rows.shape == (len(vectors),)
    for k in KR.SUMS:
        assert (rows[k + "_lo"] < 1 << 32).all()  # normalised by the host
    assert not rows["reserved"].any()
    got = KR.from_device(rows)
    if got != want:
        bad = [(g, w) for g, w in zip(got, want) if g != w]
        raise AssertionError((what, kind, e, len(bad), bad[:3]))
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_around_the_wave_and_the_workgroup(pb, orc, n):
    pos, vel, rad = recipe(n)
    sim = sim_with(pb, orc, pos, vel, rad)
    st = sim.get_state()
    assert_bit_equal(st["pos"], pos, "pos")
    for kind in KR.KINDS:
        want = check(sim, V17, 4, kind, f"n {n}", state=st, of=kind == "radius")
        assert all(r["measured"] == n for r in want)
        assert want[1]["im"] != 0 or n == 1
    sim.close()


@pytest.fixture(scope="module")
def sim257(pb, orc):
    pos, vel, rad = recipe(257)
    return sim_with(pb, orc, pos, vel, rad)


@pytest.mark.parametrize("nvec", [1, 255, 256, 257, 544, 4096])
def test_lists_around_the_tile_of_wavevectors(pb, sim257, nvec):
    if nvec == 544:
        vectors = pb.half_plane_vectors(16).tolist()
    else:
        vectors = np.random.default_rng(5200 + nvec).integers(-70, 71, (nvec, 2)).tolist()
    vectors[-1] = [-3, 2]  # the last lane of the list has work of its own
    for kind in KR.KINDS if nvec in (257, 4096) else ("density",):
        want = check(sim257, vectors, 3, kind, f"nvec {nvec}")
        assert want[-1]["measured"] == 257 and (want[-1]["re"], want[-1]["im"]) != (0, 0)


@pytest.mark.parametrize("e", [-8, 0, 12])
def test_box_lengths_at_both_ends(sim257, e):
    for kind in KR.KINDS:
        want = check(sim257, V17, e, kind, f"e {e}", of=True)
        assert want[0]["im"] == 0 and want[0]["re"] > 0 or kind == "velocity"
    # the boxes differ: the same integers mean another wavevector
    a = KR.from_device(sim257.structure_factor(V17, e, member=0))
    b = KR.from_device(sim257.structure_factor(V17, 4, member=0))
    assert a[0] == b[0] and a[1:] != b[1:]


def test_lattice_known_answers_set_with_set_state(pb, orc):
    pos, vel, rad = lattice()
    sim = sim_with(pb, orc, pos, vel, rad)
    st = sim.get_state()
    assert_bit_equal(st["pos"], pos, "pos")
    vectors = [(16, 0), (8, 0), (4, 0), (0, 16), (0, 0), (1, 0)]
    want = check(sim, vectors, 3, "density", "lattice", state=st)
    assert [(r["re"], r["im"]) for r in want[:5]] == [(256 * ONE, 0), (0, 0), (0, 0), (256 * ONE, 0), (256 * ONE, 0)]
    want = check(sim, vectors, 3, "radius", "lattice", state=st, of=True)
    assert (want[0]["re"], want[0]["im"]) == (256 * (1 << 18) * ONE, 0)
    v = pb.structure_factor_values(sim.structure_factor(vectors, 3))
    assert v["s"][0].tolist()[:5] == [256.0, 0.0, 0.0, 256.0, 256.0]  # Bragg peaks of height N, nothing in between
    assert v["s"][0][5] < 1e-12  # the first harmonic of 16 equal steps around the circle: only the entries' rounding
    sim.close()


def test_unmeasured_bots_of_every_kind(pb, orc):
    pos, vel, rad, bad = unmeasured_state()
    sim = sim_with(pb, orc, pos, vel, rad)
    st = sim.get_state()
    for k, a in (("pos", pos), ("vel", vel), ("rad", rad)):
        assert_bit_equal(st[k], a, k)
    # five bad values in each of x, y, vx, vy, rad: each kind ignores what it does not read
    for kind, count in (("density", 257 - 10), ("radius", 257 - 15), ("velocity", 257 - 20)):
        want = check(sim, V17, 4, kind, "unmeasured", state=st)
        assert all(r["measured"] == count for r in want), (kind, want[0]["measured"])
    # the largest float below 2048 is in range, in every input
    ok, qx, _, _, _ = KR.weights(pos, vel, rad, "velocity")
    assert ok[100] and ok[101] and ok[102] and ok[103] and ok[104] and qx[100] == (1 << 31) - 128
    assert BELOW < 2048.0
    sim.close()


def test_more_bots_than_one_pass_of_the_launch_covers(pb, orc):
    pos, vel, rad = lattice_state()
    assert LATTICE_BOTS > 256 * 256 and "#define PB_SK_BLOCKS 256u" in open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    sim = sim_with(pb, orc, pos, vel, rad)
    st = sim.get_state()
    vectors = V17[:6] + [(40, 17), ALIAS]
    for kind in KR.KINDS:
        want = check(sim, vectors, 6, kind, "lattice of 70000", state=st, of=True)
        assert want[0]["measured"] == LATTICE_BOTS
        if kind == "radius":
            assert want[0]["re"] > 1 << 61 and want[0]["im"] == 0  # sum qr * 2^30: the rest accumulator carries the sum
    sim.close()


def test_batch_of_three_members_do_not_leak_into_each_other(pb, orc):
    members, n = 3, 300
    ens = make_batch(pb, orc, members, n)
    states = [ens.get_state_of(k) for k in range(members)]
    for kind in KR.KINDS:
        rows = ens.structure_factor(V17, 4, kind=kind)
        assert rows.shape == (members, 17)
        refs = []
        for k in range(members):
            want = KR.structure_factor(states[k]["pos"], states[k]["vel"], states[k]["rad"], V17, 4, kind)
            assert KR.from_device(rows[k]) == want, (kind, k)
            one = ens.structure_factor(V17, 4, kind=kind, member=k)  # Of equals the member's slice
            assert one.tobytes() == rows[k].tobytes()
            refs.append(want)
        assert refs[0] != refs[1] != refs[2]
        assert ens.structure_factor(V17, 4, kind=kind).tobytes() == rows.tobytes()  # twice: the same rows
    with pytest.raises(RuntimeError, match="code 2.*pbSimStructureFactorOf.*member out of range"):
        ens.structure_factor(V17, 4, member=members)
    ens.close()


def test_example_before_and_after_stepping_and_re_sorting():
    from particlerobotsimulations_amd import host
    vectors = [list(v) for v in V17]
    seen = []
    for over in ({}, {"sort_interval": "0.05"}):  # as written, and with a re-sort every few steps
        h = host.HostSim(CFG, engine="fused", max_time="1e9", **over)
        assert h.n == 300
        for steps in (0, 200):
            if steps:
                assert h.advance(steps) > 0
            for kind in KR.KINDS:
                want = KR.structure_factor(h.get("pos"), h.get("vel"), h.get("rad"), vectors, 4, kind)
                got = KR.from_device(h.structure_factor(vectors, 4, kind=kind, member=0))
                assert got == want, (over, steps, kind)
                assert want[0]["measured"] == 300
            seen.append(want)
        h.close()
    assert seen[0] != seen[1]  # the blob moved


def live_memory():
    from particlerobotsimulations_amd import _capi
    buffers, nbytes = C.c_ulonglong(0), C.c_ulonglong(0)
    _capi.check(_capi.lib().pbDeviceMemoryLive(C.byref(buffers), C.byref(nbytes)), "pbDeviceMemoryLive")
    return int(buffers.value), int(nbytes.value)


def test_a_call_changes_nothing(pb, orc):
    pos, vel, rad = recipe(1000)
    sim = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0, phase_update_interval=0.3)
    assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    lay = layout_of(sim)
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(1000))  # sorted: the slots are not in original order
    view = (16, 16, (0.0, 0.0), 8.0)
    before, stats, t = sim.get_state(), sim.stats(), sim.time
    field, moments = sim.field_map(*view), sim.moments()
    count0, _ = sim.structure_factor_times()
    assert count0 == 0
    first = sim.structure_factor(V17, 4, kind="velocity")
    again = sim.structure_factor(V17, 4, kind="velocity", member=0)
    assert first[0].tobytes() == again.tobytes()
    check(sim, V17, 4, "velocity", "after 60 steps", state=before)
    after = sim.get_state()
    for k in before:
        assert_bit_equal(before[k], after[k], k)
    assert sim.stats() == stats and sim.time == t
    for a, b in zip(lay, layout_of(sim)):
        assert np.array_equal(a, b)
    field2, moments2 = sim.field_map(*view), sim.moments()
    assert field2[0].tobytes() == field[0].tobytes() and field2[1] == field[1] and moments2 == moments
    n, ms = sim.structure_factor_times()
    assert n == 3 and ms > 0.0
    assert sim.step(5, dt=DT, sort_interval=0.2) == 5  # and the engine steps on
    sim.close()


def test_scratch_grows_and_is_given_back(pb, orc):
    start = live_memory()
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad)
    made = live_memory()
    assert sim.structure_factor_times() == (0, 0.0) and live_memory() == made  # nothing until a structure factor is asked for
    fixed = 4096 * 8 + 4096 * 8 + 4  # the table, the list, one member's counter
    small = check(sim, V17, 4, "density", "17 vectors")
    one = live_memory()
    assert one[0] == made[0] + 4 and one[1] == made[1] + fixed + 17 * 16
    big = np.random.default_rng(5300).integers(-70, 71, (4096, 2)).tolist()
    check(sim, big, 4, "velocity", "4096 vectors")
    two = live_memory()
    assert two[0] == one[0] and two[1] == made[1] + fixed + 4096 * 64
    assert check(sim, V17, 4, "density", "17 vectors again") == small  # the larger scratch is zeroed as far as it is used
    assert live_memory() == two
    sim.close()
    assert live_memory() == start


def test_argument_errors_on_a_live_batch(pb, orc):
    from helpers import simparams_from_orc
    members, n = 6554, 65  # 6554 x 4096 x 80 bytes is above 2^31, 6553 members are below
    assert 6553 * 4096 * 80 <= 1 << 31 < members * 4096 * 80
    sp, keep = simparams_from_orc(orc.default_params(nCells=n, nDead=0, seed=70, max_time=1e9))
    ens = pb.Ensemble([sp] * members, wall_half=4.0e6, keepalive=[keep])
    pos, vel, rad = recipe(n)
    last = members - 1
    ens.set_state_of(last, pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    before = live_memory()
    big = np.random.default_rng(5400).integers(-70, 71, (4096, 2)).tolist()
    with pytest.raises(RuntimeError, match="code 2.*pbSimStructureFactor:.*2\\^31 bytes"):
        ens.structure_factor(big, 4)
    assert live_memory() == before and ens.structure_factor_times()[0] == 0
    check(ens, big, 4, "radius", "one member of many", member=last, state=ens.get_state_of(last), of=True)
    before = live_memory()
    for bad in (dict(vectors=V17, box_log2=13), dict(vectors=V17, box_log2=4, kind=3), dict(vectors=V17, box_log2=-9, member=0),
                dict(vectors=np.zeros((0, 2), np.int32), box_log2=4), dict(vectors=V17, box_log2=4, member=members)):
        with pytest.raises(RuntimeError, match="code 2.*pbSimStructureFactor"):
            ens.structure_factor(**bad)
    assert live_memory() == before and ens.structure_factor_times()[0] == 1  # the refused calls computed nothing
    check(ens, V17, 4, "density", "still usable", member=last, state=ens.get_state_of(last), of=True)
    ens.close()


# ---- the runner ------------------------------------------------------------------------------------------------------

def block_of(time, step, kind, e, rows):
    lines = ["time,%.9g,step,%d,kind,%s,box_log2,%d,vectors,%d" % (time, step, kind, e, len(rows))]
    for r in rows:
        lines.append(",".join(str(r[k]) for k in KR.ROW_FIELDS))
    return lines


# the example as written (dump_interval 60: the one block at time 0), and with a dump row every 0.5 s
@pytest.mark.parametrize("extra,flags,kind,nmax", [({}, [], "density", 16),
                                                   ({"dump_interval": "0.5"}, ["--sk-kind", "velocity", "--sk-nmax", "3"], "velocity", 3)],
                         ids=["as_written", "dump_0.5_velocity"])
def test_runner_writes_a_block_at_every_dump_time(pb, tmp_path, extra, flags, kind, nmax):
    from particlerobotsimulations_amd import host
    over = dict(max_time="2", **extra)
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--sk", "s.csv"] + flags, capture_output=True, text=True,
                       timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "s.csv").read().splitlines()
    flat = host.load_config(CFG, **over)
    e = min(12, max(-8, math.ceil(math.log2(2.0 * flat.wallHalf))))  # the smallest box that holds the walls
    assert 2.0 ** e >= 2.0 * flat.wallHalf and (e == -8 or 2.0 ** (e - 1) < 2.0 * flat.wallHalf)
    vectors = pb.half_plane_vectors(nmax)
    assert len(vectors) == (544 if nmax == 16 else 24)
    di = f32(flat.dump_interval)

    def due(t):  # the gate of dumpParticlebot, in its fp32 operations
        t = f32(t)
        return not (t - di * np.floor(t / di) > f32(0.01))

    # the same blocks from the class driven in-process, stopped at the same steps
    h = host.HostSim(CFG, engine="fused", **over)
    want, steps, blocks, last_is_final = [], 0, 0, False
    while True:
        last_is_final = bool(due(h.time))
        if last_is_final:
            rows = KR.from_device(h.structure_factor(vectors, e, kind=kind, member=0))
            assert rows[0]["measured"] == 300
            # the API's rows are the reference's of the state they were taken from
            assert rows == KR.structure_factor(h.get("pos"), h.get("vel"), h.get("rad"), vectors, e, kind), blocks
            want += block_of(h.time, steps, kind, e, rows)
            blocks += 1
        if h.finished:
            break
        ran = h.advance(h.steps_until_dump())
        if ran == 0:
            break
        steps += ran
    assert blocks >= (4 if extra else 1), blocks
    assert lines == want and len(lines) == blocks * (1 + len(vectors))
    # with a dump row every 0.5 s the run ends on a dump time: its last block is the final state's, and it was compared
    # with the reference of that state above (as written, the only blocks are the two around time 0)
    print("blocks", blocks, "steps", steps, "time", h.time, "the last block is the final state's:", last_is_final)
    assert last_is_final == bool(extra)
    h.close()
