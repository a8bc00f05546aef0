"""GPU: the time series (pbSimMoments / pbSimSetSeries / pbSimGetSeriesOf, csrc/pb_moments.hip) against
tests/series_ref.py on states read back from the device.  Every comparison is exact: a row holds integers only, the
record's time is compared as the fp32 value it is.  A recorded series is compared with a twin run that has the series
off and is stopped in front of every step the gate names.  tests/test_series_api.py pins the reference to a plain loop
and to known answers on the CPU, and shows that the recipes used here keep every bot measured."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import series_ref as SR
from helpers import assert_bit_equal, simparams_from_orc
from test_series_api import (CORNER, SIZES, known_answer_state, recipe, tie_state, unmeasured_state)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
PASS_BOTS = 512 * 256  # PB_MOMENTS_BLOCKS workgroups of 256 lanes: the bots of a member one pass of the launch covers
DT = 0.01


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def sim_with(pb, orc, pos, vel, rad, wall_half=4.0e6, **over):
    pos = np.asarray(pos, f32).reshape(-1, 2)
    n = pos.shape[0]
    over.setdefault("nDead", 0)
    over.setdefault("max_time", 1e9)
    P = orc.default_params(nCells=n, seed=3, **over)
    sp, keep = simparams_from_orc(P)
    sim = pb.Sim(sp, wall_half=wall_half, keepalive=keep)
    sim.set_state(pos=pos, vel=vel, rad=np.asarray(rad, f32), phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    return sim


def sums(row):
    return {k: row[k] for k in SR.FIELDS}


def check_now(sim, what, member=0, state=None, row=None):
    """One member's row of the state as it is now against the reference on the state read back; returns the reference."""
    st = state if state is not None else sim.get_state()
    want = SR.moments(st["pos"], st["vel"], st["rad"])
    if row is None:
        row = sim.moments()[member]
    print(what, row)
    assert sums(row) == want, (what, row, want)
    assert set(row) == set(SR.FIELDS) | {"time", "step"}
    return want


# ---- the state as it is now ------------------------------------------------------------------------------------------

def test_header_constant_is_the_one_used_here():
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    assert "#define PB_MOMENTS_BLOCKS 512u" in header


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", ["origin", "corner"])
def test_sizes_around_the_wave_and_the_workgroup(pb, orc, n, where):
    pos, vel, rad = recipe(n, CORNER if where == "corner" else (0.0, 0.0))
    sim = sim_with(pb, orc, pos, vel, rad)
    st = sim.get_state()
    assert_bit_equal(st["pos"], pos, "pos")
    assert_bit_equal(st["vel"], vel, "vel")
    want = check_now(sim, f"n {n} {where}", state=st)
    assert want["measured"] == n
    row = sim.moments()[0]
    assert row["time"] == 0.0 and row["step"] == 0
    if where == "corner" and n > 1:
        assert want["xy"] < 0 < want["xx"] and want["sum_qx"] < 0 < want["sum_qy"]


def test_more_bots_than_one_pass_of_the_launch_covers(pb, orc):
    n = PASS_BOTS + 321  # the grid-stride loop runs twice for 321 lanes, and the last workgroups' tails differ
    assert PASS_BOTS < n < 300000
    pos, vel, rad = recipe(n)
    pos += np.array([-300.0, 700.0], f32)  # (off the origin: sums that do not cancel)
    sim = sim_with(pb, orc, pos, vel, rad)
    want = check_now(sim, f"n {n}")
    assert want["measured"] == n and want["xx"] > 1 << 64 and want["yy"] > 1 << 64


def test_known_answers_set_with_set_state(pb, orc):
    for name, (pos, vel, rad) in (("three bots", known_answer_state()), ("ties", tie_state())):
        sim = sim_with(pb, orc, pos, vel, rad)
        st = sim.get_state()
        for k, a in (("pos", pos), ("vel", vel), ("rad", rad)):
            assert_bit_equal(st[k], a, k)
        want = check_now(sim, name, state=st)
        assert want["measured"] == 3
    assert want["sum_qx"] == 2 and want["yy"] == 24  # the ties went to even on the device too
    # no measured bot: an all-zero row, the box included
    pos, vel, rad = recipe(65)
    rad[:] = np.inf
    sim = sim_with(pb, orc, pos, vel, rad)
    assert sums(sim.moments()[0]) == dict.fromkeys(SR.FIELDS, 0)


def test_unmeasured_bots_of_every_kind(pb, orc):
    pos, vel, rad, bad = unmeasured_state()
    sim = sim_with(pb, orc, pos, vel, rad)
    st = sim.get_state()
    for k, a in (("pos", pos), ("vel", vel), ("rad", rad)):
        assert np.array_equal(np.isnan(st[k]), np.isnan(a)) and np.array_equal(st[k][~np.isnan(a)], a[~np.isnan(a)]), k
    want = check_now(sim, "unmeasured", state=st)
    assert want["measured"] == 257 - len(bad) and want["max_qx"] == (1 << 31) - 128 and want["min_qy"] == 128 - (1 << 31)


def make_batch(pb, orc, members, n, **over):
    plist, keeps = [], []
    over.setdefault("max_time", 1e9)
    for k in range(members):
        P = orc.default_params(nCells=n, nDead=0, seed=70 + k, **over)
        sp, keep = simparams_from_orc(P)
        plist.append(sp)
        keeps.append(keep)
    ens = pb.Ensemble(plist, wall_half=4.0e6, keepalive=keeps)
    rng = np.random.default_rng(77)
    from helpers import jittered_blob
    for k in range(members):
        pos, vel, rad = jittered_blob(n, 0.15 + 0.01 * k, rng, center=(3.0 * k - 1.0, -2.0 * k), jitter=0.3)
        ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    return ens


def test_batch_of_three_members_do_not_leak_into_each_other(pb, orc):
    ens = make_batch(pb, orc, 3, 257)
    rows = ens.moments()
    assert len(rows) == 3
    wants = [check_now(ens, f"member {k}", state=ens.get_state_of(k), row=rows[k]) for k in range(3)]
    assert all(w["measured"] == 257 for w in wants)
    assert wants[0] != wants[1] != wants[2] and wants[0]["sum_qx"] < 0 < wants[2]["sum_qx"]
    assert ens.moments() == rows  # twice: the same rows


def layout_of(sim, k=0):
    from particlerobotsimulations_amd import _capi
    orig, keys, srt = np.empty(sim.n, np.uint32), np.empty(sim.n, np.uint32), C.c_int(0)
    _capi.check(_capi.lib().pbSimGetLayoutOf(sim._h, k, _capi.np_ptr(orig), _capi.np_ptr(keys), C.byref(srt)), "layout")
    return orig, keys, srt.value


def test_reading_the_moments_changes_nothing(pb, orc):
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, phase_update_interval=0.3)
    assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    before, stats, lay, t = sim.get_state(), sim.stats(), layout_of(sim), sim.time
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(300))  # sorted: the slots are not in original order
    first = sim.moments()
    assert first == sim.moments() and first[0]["step"] == 60 and f32(first[0]["time"]) == f32(t)
    check_now(sim, "after 60 steps", state=before, row=first[0])
    after = sim.get_state()
    for k in before:
        assert_bit_equal(before[k], after[k], k)
    assert sim.stats() == stats and sim.time == t
    for a, b in zip(lay, layout_of(sim)):
        assert np.array_equal(a, b)
    n, ms = sim.series_times()
    assert n == 0 and ms > 0.0  # no record was taken; the last row's launches were timed


# ---- recording while stepping ----------------------------------------------------------------------------------------

STEPS, INTERVAL, SORT, PUI = 300, 0.25, 0.375, 0.625
FORMS = {"fused": dict(resident=1), "resident": dict(resident=2), "throughput": dict(resident=1, lanes=1),
         "every_step": dict(resident=1)}


def light_wave_sim(pb, orc, form, **over):
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0, phase_update_interval=PUI, **over)  # LIGHT_WAVE
    sim.set_resident(form["resident"])
    if "lanes" in form:
        sim.set_lanes_per_bot(form["lanes"])
    return sim


def reference_rows(twin, gates, nsteps, state_of=None, sort_interval=SORT):
    """Steps the twin (series off) in pieces that stop in front of every step `gates` names; the reference row of the
    state read back at each stop, with the record's time and step.  Runs the twin to nsteps."""
    state_of = state_of or (lambda: twin.get_state())
    rows, at = [], 0
    for k, t in gates:
        if k > at:
            assert twin.step(k - at, dt=DT, sort_interval=sort_interval) == k - at
            at = k
        assert f32(twin.time) == f32(t), (k, twin.time, t)
        st = state_of()
        states = st if isinstance(st, list) else [st]
        rows.append([dict(SR.moments(s["pos"], s["vel"], s["rad"]), time=float(f32(t)), step=k) for s in states])
    if nsteps > at:
        twin.step(nsteps - at, dt=DT, sort_interval=sort_interval)
    return rows


@pytest.mark.parametrize("name", list(FORMS))
def test_recorded_rows_equal_a_twin_stopped_in_front_of_every_gate_step(pb, orc, name):
    form = FORMS[name]
    interval, steps = (0.0, 120) if name == "every_step" else (INTERVAL, STEPS)
    gates = SR.gate_steps(0.0, DT, interval, steps, 1e9)
    rec = [k for k, _ in gates]
    sorts = [k for k, _ in SR.gate_steps(0.0, DT, SORT, steps, 1e9)]
    phases = [k for k, _ in SR.gate_steps(0.0, DT, PUI, steps, 1e9)]
    assert len(rec) >= 8
    assert set(sorts[1:]) & set(rec) and set(phases[1:]) & set(rec)  # a re-sort and a phase update on a record's step
    if interval:
        assert set(sorts) - set(rec) and set(phases) - set(rec)      # and one of each between records
    a = light_wave_sim(pb, orc, form)
    cfg = a.config()
    assert cfg["resident"] == (1 if name == "resident" else 0)
    if "lanes" in form:
        assert cfg["lanes_per_bot"] == 1
    a.set_series(interval, 512)
    assert a.series_info() == {"interval": float(f32(interval)), "capacity": 512, "records": 0}
    assert a.step(steps, dt=DT, sort_interval=SORT) == steps  # one call
    assert a.series_info()["records"] == len(rec)
    got = a.series_of(0)
    b = light_wave_sim(pb, orc, form)
    want = [r[0] for r in reference_rows(b, gates, steps)]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (name, g, w)  # the sums, the box, the fp32 time and the step
    assert [g["step"] for g in got] == rec
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert_bit_equal(sa[k], sb[k], f"{name} {k}")
    assert a.time == b.time and a.stats()["steps"] == b.stats()["steps"] == steps
    assert a.stats()["resorts"] == b.stats()["resorts"] == len(sorts)
    assert a.stats()["phase_updates"] == b.stats()["phase_updates"] == len(phases)
    if name == "resident":
        assert a.stats()["resident_launches"] > 0
    if name == "every_step":
        assert a.stats()["fused_launches"] == 0  # interval 0 costs the fusion
    elif name != "resident":
        assert a.stats()["fused_launches"] > 0
    # the summary's curve moves: the blob breathes under the light wave
    s0, s1 = pb.moments_summary(got[0]), pb.moments_summary(got[-1])
    assert s0["mean_radius"] != s1["mean_radius"] and s0["centroid"] != s1["centroid"]
    n, ms = a.series_times()
    assert n == len(rec) and ms > 0.0


def test_ring_keeps_the_last_capacity_records(pb, orc):
    gates = SR.gate_steps(0.0, DT, INTERVAL, STEPS, 1e9)
    assert len(gates) >= 8
    a = light_wave_sim(pb, orc, FORMS["fused"])
    a.set_series(INTERVAL, 5)
    assert a.step(STEPS, dt=DT, sort_interval=SORT) == STEPS
    assert a.series_info() == {"interval": INTERVAL, "capacity": 5, "records": len(gates)}
    b = light_wave_sim(pb, orc, FORMS["fused"])
    want = [r[0] for r in reference_rows(b, gates, STEPS)]
    assert a.series_of(0) == want[-5:]
    first = len(gates) - 5
    assert a.series_of(0, first=first + 1, count=3) == want[first + 1:first + 4]
    assert a.series_of(0, first=len(gates), count=0) == [] and a.series_of(0, first=first, count=0) == []
    for bad in (dict(first=first - 1, count=1), dict(first=first - 1, count=6), dict(first=first, count=6),
                dict(first=len(gates), count=1), dict(first=len(gates) + 1, count=0), dict(first=0, count=1)):
        with pytest.raises(RuntimeError, match="code 2.*pbSimGetSeriesOf.*window"):
            a.series_of(0, **bad)
    with pytest.raises(RuntimeError, match="code 2.*member out of range"):
        a.series_of(1)
    assert a.series_of(0) == want[-5:]  # refused reads changed nothing


def test_restart_switch_off_and_argument_errors(pb, orc):
    a = light_wave_sim(pb, orc, FORMS["fused"])
    none = {"interval": 0.0, "capacity": 0, "records": 0}
    assert a.series_info() == none and a.series_times() == (0, 0.0)
    with pytest.raises(RuntimeError, match="code 2.*the series is off"):
        a.series_of(0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="code 2.*interval"):
            a.set_series(bad, 8)
    with pytest.raises(RuntimeError, match="code 2.*2\\^31 bytes"):
        a.set_series(0.0, (1 << 31) // 152 + 1)
    assert a.series_info() == none
    a.set_series(0.0, 64)
    assert a.step(20, dt=DT, sort_interval=SORT) == 20 and a.series_info()["records"] == 20
    # again: restarts at record 0, with the time and the step count as they are now
    a.set_series(0.05, 64)
    assert a.series_info() == {"interval": float(f32(0.05)), "capacity": 64, "records": 0} and a.series_of(0) == []
    t20 = a.time
    gates = SR.gate_steps(t20, DT, 0.05, 30, 1e9)
    assert a.step(30, dt=DT, sort_interval=SORT) == 30
    got = a.series_of(0)
    assert [(g["step"] - 20, g["time"]) for g in got] == gates and 5 <= len(gates) <= 7
    # capacity 0 frees: later steps record nothing
    a.set_series(0.05, 0)
    assert a.series_info() == none
    stats = a.stats()
    assert a.step(30, dt=DT, sort_interval=SORT) == 30 and a.series_info() == none
    assert a.stats()["fused_launches"] == stats["fused_launches"] + 29  # every step but the call's last is fused again
    with pytest.raises(RuntimeError, match="code 2.*the series is off"):
        a.series_of(0)


def test_no_record_for_the_step_that_max_time_stops(pb, orc):
    gates = SR.gate_steps(0.0, DT, 0.0, 50, 0.1)
    a = light_wave_sim(pb, orc, FORMS["fused"], max_time=0.1)
    a.set_series(0.0, 64)
    done = a.step(50, dt=DT, sort_interval=SORT)
    assert done == len(gates) and 10 <= done <= 12
    assert a.series_info()["records"] == done and a.step(5, dt=DT, sort_interval=SORT) == 0
    assert a.series_info()["records"] == done
    assert [(g["step"], g["time"]) for g in a.series_of(0)] == gates


def test_batch_of_three_members_records_each_members_own_rows(pb, orc):
    steps = 100
    gates = SR.gate_steps(0.0, DT, INTERVAL, steps, 1e9)
    a = make_batch(pb, orc, 3, 300, control=0, phase_update_interval=PUI)
    b = make_batch(pb, orc, 3, 300, control=0, phase_update_interval=PUI)
    a.set_series(INTERVAL, 16)
    assert a.step(steps, dt=DT, sort_interval=SORT) == steps
    want = reference_rows(b, gates, steps, state_of=lambda: [b.get_state_of(k) for k in range(3)])
    for k in range(3):
        got = a.series_of(k)
        assert got == [w[k] for w in want], k
        assert all(g["measured"] == 300 for g in got)
    assert a.series_of(0) != a.series_of(1) != a.series_of(2)
    for k in range(3):
        sa, sb = a.get_state_of(k), b.get_state_of(k)
        for name in sa:
            assert_bit_equal(sa[name], sb[name], f"member {k} {name}")


def test_trail_and_series_together(pb, orc):
    over = dict(centroid_int=0.2, centroid_steps=8)
    gates = SR.gate_steps(0.0, DT, INTERVAL, 200, 1e9)
    a, b, c = (light_wave_sim(pb, orc, FORMS["resident"], **over) for _ in range(3))
    for s in (a, b):
        s.set_centroid_trail(True)
    a.set_series(INTERVAL, 16)
    assert a.step(200, dt=DT, sort_interval=SORT) == 200 and b.step(200, dt=DT, sort_interval=SORT) == 200
    (ax, at, ar), (bx, bt, br) = a.centroid_trail(), b.centroid_trail()
    assert ar == br and ar >= 8
    assert_bit_equal(ax, bx, "trail ring")
    assert np.array_equal(at.view(np.uint32), bt.view(np.uint32))
    assert a.series_of(0) == [r[0] for r in reference_rows(c, gates, 200)]
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert_bit_equal(sa[k], sb[k], k)


# ---- the runner ------------------------------------------------------------------------------------------------------

HEADER = ("Time, Step, Measured, SumQx, SumQy, MinQx, MaxQx, MinQy, MaxQy, SumXX, SumYY, SumXY, SumQr, SumRR, SumWx, "
          "SumWy, SumVV")
COLUMNS = ("step", "measured", "sum_qx", "sum_qy", "min_qx", "max_qx", "min_qy", "max_qy", "xx", "yy", "xy", "sum_qr",
           "rr", "sum_wx", "sum_wy", "vv")


def line_of(row):
    return ", ".join(["%.9g" % row["time"]] + [str(row[k]) for k in COLUMNS])


# the example as it is (dump_interval 60: the one row at time 0), and with a dump row every 2.5 s
@pytest.mark.parametrize("extra", [{}, {"dump_interval": "2.5"}], ids=["as_written", "dump_2.5"])
def test_runner_writes_the_series_at_the_dump_interval(tmp_path, extra):
    from particlerobotsimulations_amd import host
    over = dict(max_time="30", **extra)
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--series", "s.csv"], capture_output=True, text=True,
                       timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "s.csv").read().splitlines()
    flat = host.load_config(CFG, **over)
    gates = SR.gate_steps(0.0, flat.timestep, flat.dump_interval, 10000, 30.0)
    assert lines[0] == HEADER and len(lines) == 1 + len(gates) and len(gates) == (12 if extra else 1)
    cells = [[c.strip() for c in l.split(",")] for l in lines[1:]]
    assert all(c[2] == "300" for c in cells)
    # every row's time is one of the CSV's dump times, in order
    main_times = [l.split(",")[0] for l in open(tmp_path / "example_data.csv").read().splitlines()[2:]]
    mine = ["%f" % float(c[0]) for c in cells]
    it = iter(main_times)
    assert all(t in it for t in mine), (mine, main_times)
    assert [int(c[1]) for c in cells] == sorted({int(c[1]) for c in cells})
    # the same rows from the class driven in-process
    h = host.HostSim(CFG, engine="fused", **over)
    h.set_series(flat.dump_interval, 4096)
    assert h.series_info() == {"interval": float(f32(flat.dump_interval)), "capacity": 4096, "records": 0}
    while not h.finished:
        if h.advance(h.steps_until_dump()) == 0:
            break
    want = h.series_rows(0)
    assert lines[1:] == [line_of(w) for w in want]
    assert [(w["step"], w["time"]) for w in want] == gates
    assert want[-1] == h.series_rows(len(want) - 1)[0] and h.moments()[0]["measured"] == 300
    h.close()


def test_runner_loses_no_record_with_a_ring_of_two(tmp_path):
    from particlerobotsimulations_amd import host
    flat = host.load_config(CFG, max_time="0.5")
    gates = SR.gate_steps(0.0, flat.timestep, 0.0, 1000, 0.5)
    r = subprocess.run([RUN, CFG, "--quiet", "--set", "max_time", "0.5", "--series", "s.csv", "--series-capacity", "2",
                        "--series-interval", "0"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "s.csv").read().splitlines()
    assert lines[0] == HEADER
    cells = [[c.strip() for c in l.split(",")] for l in lines[1:]]
    assert [(int(c[1]), c[0]) for c in cells] == [(k, "%.9g" % t) for k, t in gates] and 50 <= len(gates) <= 52
