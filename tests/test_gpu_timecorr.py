"""GPU: the time correlations (pbSimSetTimeCorrelation / pbSimTimeCorrelationRecord / pbSimGetTimeCorrelation,
csrc/pb_timecorr.hip) against tests/timecorr_ref.py on states read back from the device.  Every comparison is exact: a
row holds integers only.  A table recorded while stepping is compared with a twin run that has the correlation off and
is stopped in front of every step the gate names.  tests/test_timecorr_api.py pins the reference to a plain loop and to
known answers on the CPU, and shows that the recipes and shifts used here keep every pair measured."""
import os
import re
import subprocess

import numpy as np
import pytest

import series_ref as SR
import timecorr_ref as TR
from helpers import assert_bit_equal, simparams_from_orc
from test_gpu_series import DT, FORMS, INTERVAL, PUI, SORT, STEPS, layout_of, light_wave_sim, make_batch, sim_with
from test_series_api import CORNER, SIZES, recipe
from test_timecorr_api import (BATCH_BOTS, BATCH_LAGS, BATCH_RADIUS, KNOWN, MANUAL_LAGS, MANUAL_RADIUS, TIES,
                               batch_records, known_answer_records, manual_records, tie_records, unmeasured_records)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
LAGS, RADIUS = 5, 0.015625  # while stepping
OFF = {"interval": 0.0, "lags": 0, "overlap_radius": 0.0, "records": 0}


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def header_constant(name):
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    return int(re.search(r"#define %s (\d+)u" % name, header).group(1))


def record_manually(sim, records, lags, radius):
    """Sets each of `records` (pos, vel[, rad]) and takes a record of it; returns the member's rows and the states read
    back, as (pos, vel)."""
    n = len(records[0][0])
    sim.set_time_correlation(-1.0, lags, radius)
    assert sim.time_correlation_info() == {"interval": -1.0, "lags": lags, "overlap_radius": float(f32(radius)),
                                           "records": 0}
    back = []
    for rec in records:
        rad = rec[2] if len(rec) > 2 else np.full(n, 0.1, f32)
        sim.set_state(pos=rec[0], vel=rec[1], rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
        st = sim.get_state()
        back.append((st["pos"], st["vel"]))
        sim.time_correlation_record()
    assert sim.time_correlation_info()["records"] == len(records)
    return sim.time_correlation()[0], back


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- manual records on set states ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", ["origin", "corner"])
def test_manual_records_around_the_wave_and_the_workgroup(pb, orc, n, where):
    recs = manual_records(n, CORNER if where == "corner" else (0.0, 0.0))
    sim = sim_with(pb, orc, *recs[0])
    rows, back = record_manually(sim, recs, MANUAL_LAGS, MANUAL_RADIUS)
    for (p, v), rec in zip(back, recs):
        assert same_bits(p, rec[0]) and same_bits(v, rec[1])
    want = TR.table(back, [0] * 4, MANUAL_LAGS, MANUAL_RADIUS)
    print(n, where, rows)
    assert rows == want, (n, where, rows, want)
    assert [r["origins"] for r in rows] == [4, 3, 2] and [r["samples"] for r in rows] == [4 * n, 3 * n, 2 * n]
    assert [r["sum_steps"] for r in rows] == [0, 0, 0] and rows[0]["msd"] == 0 and rows[1]["msd"] > 0


def test_more_bots_than_one_pass_covers(pb, orc):
    n = header_constant("PB_TCORR_BLOCKS") * 256 + 321  # the grid-stride loop runs twice for 321 lanes
    assert n == 65857
    recs = manual_records(n, (-300.0, 700.0), records=3)
    sim = sim_with(pb, orc, *recs[0])
    rows, back = record_manually(sim, recs, 2, MANUAL_RADIUS)
    want = TR.table(back, [0] * 3, 2, MANUAL_RADIUS)
    assert rows == want
    assert [r["samples"] for r in rows] == [3 * n, 2 * n] and rows[1]["msd"] > 1 << 48


def test_known_answers_ties_and_unmeasured_pairs(pb, orc):
    for name, recs, lags, radius, known in (("three bots", known_answer_records(), 3, 0.75, KNOWN),
                                            ("ties", tie_records(), 2, 2.5 * 2.0 ** -20, TIES)):
        sim = sim_with(pb, orc, recs[0][0], recs[0][1], np.full(3, 0.1, f32))
        rows, back = record_manually(sim, recs, lags, radius)
        for (p, v), rec in zip(back, recs):
            assert same_bits(p, rec[0]) and same_bits(v, rec[1]), name
        assert rows == TR.table(back, [0] * len(recs), lags, radius), name
        assert rows == [dict(k, sum_steps=0) for k in known], (name, rows)  # (no step ran between the records)
    assert rows[1]["sum_qx"] == 4 and rows[1]["msd"] == 28 and rows[1]["vacf"] == 28  # the ties went to even here too
    recs, bad1, bad0 = unmeasured_records()
    sim = sim_with(pb, orc, recs[0][0], recs[0][1], np.full(257, 0.1, f32))
    rows, back = record_manually(sim, recs, 2, 0.6)
    for (p, v), rec in zip(back, recs):
        for got, put in ((p, rec[0]), (v, rec[1])):
            nan = np.isnan(put)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], put[~nan])
    assert rows == TR.table(back, [0, 0], 2, 0.6)
    top = (1 << 31) - 128
    assert rows[1]["samples"] == 257 - len(bad1) and rows[0]["samples"] == 2 * 257 - 26 and rows[1]["max_q2"] == top * top
    # no measured pair: an all-zero table
    pos, vel, rad = recipe(65)
    bad = np.full_like(vel, np.inf)
    sim = sim_with(pb, orc, pos, bad, rad)
    rows, _ = record_manually(sim, [(pos, bad, rad), (pos, bad, rad)], 2, 0.5)
    assert rows == [dict(dict.fromkeys(TR.FIELDS, 0), lag=0, origins=2), dict(dict.fromkeys(TR.FIELDS, 0), lag=1, origins=1)]


def test_batch_of_three_members_do_not_leak_into_each_other(pb, orc):
    n, recs = BATCH_BOTS, batch_records()
    ens = make_batch(pb, orc, 3, n)
    ens.set_time_correlation(-1.0, BATCH_LAGS, BATCH_RADIUS)
    back = [[] for _ in range(3)]
    for r in range(4):
        for k in range(3):
            pos, vel, rad = recs[k][r]
            ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
            st = ens.get_state_of(k)
            assert same_bits(st["pos"], pos) and same_bits(st["vel"], vel)
            back[k].append((st["pos"], st["vel"]))
        ens.time_correlation_record()
    rows = ens.time_correlation()
    assert len(rows) == 3 and all(len(r) == BATCH_LAGS for r in rows)
    for k in range(3):
        assert rows[k] == TR.table(back[k], [0] * 4, BATCH_LAGS, BATCH_RADIUS), k
        assert [r["samples"] for r in rows[k]] == [4 * n, 3 * n, 2 * n]
    assert rows[0][1] != rows[1][1] != rows[2][1] and rows[0][1]["msd"] < rows[2][1]["msd"]
    assert rows[0][1]["vacf"] > 0 > rows[2][1]["vacf"]
    assert ens.time_correlation() == rows  # twice: the same rows


# ---- recorded while stepping -----------------------------------------------------------------------------------------

def twin_states(twin, gates, nsteps, state_of=None, sort_interval=SORT):
    """Steps the twin (correlation off) in pieces that stop in front of every step `gates` names; the (pos, vel) read
    back at each stop, per member.  Runs the twin to nsteps."""
    state_of = state_of or (lambda: [twin.get_state()])
    out, at = None, 0
    for k, t in gates:
        if k > at:
            assert twin.step(k - at, dt=DT, sort_interval=sort_interval) == k - at
            at = k
        assert f32(twin.time) == f32(t), (k, twin.time, t)
        states = state_of()
        out = out or [[] for _ in states]
        for m, s in enumerate(states):
            out[m].append((s["pos"], s["vel"]))
    if nsteps > at:
        twin.step(nsteps - at, dt=DT, sort_interval=sort_interval)
    return out


@pytest.mark.parametrize("name", list(FORMS))
def test_recorded_table_equals_a_twin_stopped_in_front_of_every_gate_step(pb, orc, name):
    form = FORMS[name]
    interval, steps = (0.0, 120) if name == "every_step" else (INTERVAL, STEPS)
    gates = SR.gate_steps(0.0, DT, interval, steps, 1e9)
    rec = [k for k, _ in gates]
    sorts = [k for k, _ in SR.gate_steps(0.0, DT, SORT, steps, 1e9)]
    phases = [k for k, _ in SR.gate_steps(0.0, DT, PUI, steps, 1e9)]
    assert len(rec) > LAGS  # the ring wraps
    assert set(sorts[1:]) & set(rec) and set(phases[1:]) & set(rec)  # a re-sort and a phase update on a record's step
    if interval:
        assert set(sorts) - set(rec) and set(phases) - set(rec)      # and one of each between records
    a = light_wave_sim(pb, orc, form)
    assert a.config()["resident"] == (1 if name == "resident" else 0)
    a.set_time_correlation(interval, LAGS, RADIUS)
    assert a.time_correlation_info() == {"interval": float(f32(interval)), "lags": LAGS, "overlap_radius": RADIUS,
                                         "records": 0}
    assert a.step(steps, dt=DT, sort_interval=SORT) == steps  # one call
    assert a.time_correlation_info()["records"] == len(rec)
    got = a.time_correlation()[0]
    b = light_wave_sim(pb, orc, form)
    want = TR.table(twin_states(b, gates, steps)[0], rec, LAGS, RADIUS)
    print(name, got)
    assert got == want, (name, got, want)
    assert [g["origins"] for g in got] == [len(rec) - l for l in range(LAGS)]
    assert all(g["samples"] == 300 * g["origins"] for g in got) and got[1]["msd"] > 0 and got[1]["vacf"] != 0
    assert 0 < got[1]["overlap"] < got[1]["samples"]  # bots on both sides of the overlap radius
    lay = layout_of(a)
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(300))  # sorted: the slots are not in original order
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
    s = pb.time_correlation_summary(got[LAGS - 1], got[0])
    assert s["msd"] > 0.0 and s["mean_lag_steps"] == got[LAGS - 1]["sum_steps"] / got[LAGS - 1]["origins"]
    n, ms = a.time_correlation_times()
    assert n == len(rec) and ms > 0.0


def test_batch_of_three_members_records_each_against_its_own_twin(pb, orc):
    steps = 150
    gates = SR.gate_steps(0.0, DT, INTERVAL, steps, 1e9)
    rec = [k for k, _ in gates]
    a = make_batch(pb, orc, 3, 300, control=0, phase_update_interval=PUI)
    b = make_batch(pb, orc, 3, 300, control=0, phase_update_interval=PUI)
    a.set_time_correlation(INTERVAL, 4, RADIUS)
    assert a.step(steps, dt=DT, sort_interval=SORT) == steps
    states = twin_states(b, gates, steps, state_of=lambda: [b.get_state_of(k) for k in range(3)])
    got = a.time_correlation()
    for k in range(3):
        assert got[k] == TR.table(states[k], rec, 4, RADIUS), k
        assert all(g["samples"] == 300 * g["origins"] for g in got[k])
    assert got[0][1] != got[1][1] != got[2][1]
    for k in range(3):
        sa, sb = a.get_state_of(k), b.get_state_of(k)
        for name in sa:
            assert_bit_equal(sa[name], sb[name], f"member {k} {name}")


def test_series_trail_and_correlation_together(pb, orc):
    over = dict(centroid_int=0.2, centroid_steps=8)
    tci = 0.15  # another interval than the series': either gate ends a stretch
    a, b, c = (light_wave_sim(pb, orc, FORMS["resident"], **over) for _ in range(3))
    for s in (a, b):
        s.set_centroid_trail(True)
        s.set_series(INTERVAL, 16)
    for s in (a, c):
        s.set_time_correlation(tci, LAGS, RADIUS)
    for s in (a, b, c):
        assert s.step(200, dt=DT, sort_interval=SORT) == 200
    (ax, at, ar), (bx, bt, br) = a.centroid_trail(), b.centroid_trail()
    assert ar == br and ar >= 8
    assert_bit_equal(ax, bx, "trail ring")
    assert np.array_equal(at.view(np.uint32), bt.view(np.uint32))
    assert a.series_of(0) == b.series_of(0) and len(a.series_of(0)) == len(SR.gate_steps(0.0, DT, INTERVAL, 200, 1e9))
    ta, tc = a.time_correlation(), c.time_correlation()
    assert ta == tc and ta[0][0]["origins"] == len(SR.gate_steps(0.0, DT, tci, 200, 1e9)) > LAGS
    sa, sb, sc = a.get_state(), b.get_state(), c.get_state()
    for k in sa:
        assert_bit_equal(sa[k], sb[k], k)
        assert_bit_equal(sa[k], sc[k], k)


def test_reading_and_recording_change_nothing(pb, orc):
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, phase_update_interval=0.3)
    sim.set_series(0.1, 8)
    sim.set_time_correlation(-1.0, 3, RADIUS)
    assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    assert sim.time_correlation_info()["records"] == 0  # manual only
    before, stats, lay, t, series = sim.get_state(), sim.stats(), layout_of(sim), sim.time, sim.series_of(0)
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(300))
    sim.time_correlation_record()
    sim.time_correlation_record()
    first = sim.time_correlation()
    assert first == sim.time_correlation()
    assert first[0] == TR.table([(before["pos"], before["vel"])] * 2, [60, 60], 3, RADIUS)
    after = sim.get_state()
    for k in before:
        assert_bit_equal(before[k], after[k], k)
    assert sim.stats() == stats and sim.time == t and sim.series_of(0) == series
    for a, b in zip(lay, layout_of(sim)):
        assert np.array_equal(a, b)
    # a later step and a set_state leave the ring alone: the next record pairs with the two it holds
    assert sim.step(7, dt=DT, sort_interval=0.2) == 7
    now = sim.get_state()
    sim.set_state(pos=now["pos"], vel=now["vel"], rad=now["rad"], phase=now["phase"], dead=now["dead"])
    sim.time_correlation_record()
    snaps = [(before["pos"], before["vel"])] * 2 + [(now["pos"], now["vel"])]
    assert sim.time_correlation()[0] == TR.table(snaps, [60, 60, 67], 3, RADIUS)
    n, ms = sim.time_correlation_times()
    assert n == 3 and ms > 0.0


def test_restart_switch_off_and_argument_errors(pb, orc):
    a = light_wave_sim(pb, orc, FORMS["fused"])
    assert a.time_correlation_info() == OFF and a.time_correlation_times() == (0, 0.0)
    for call in (a.time_correlation_record, a.time_correlation):
        with pytest.raises(RuntimeError, match="code 2.*the correlation is off"):
            call()
    for bad, word in (((-0.5, 4, 0.1), "interval"), ((float("nan"), 4, 0.1), "interval"), ((float("inf"), 4, 0.1), "interval"),
                      ((0.0, 65, 0.1), "lags"), ((0.0, 4, 2048.0), "overlapRadius"), ((0.0, 4, -0.1), "overlapRadius"),
                      ((0.0, 4, float("nan")), "overlapRadius")):
        with pytest.raises(RuntimeError, match="code 2.*pbSimSetTimeCorrelation.*" + word):
            a.set_time_correlation(*bad)
    assert a.time_correlation_info() == OFF
    a.set_time_correlation(0.0, 4, RADIUS)
    assert a.step(20, dt=DT, sort_interval=SORT) == 20 and a.time_correlation_info()["records"] == 20
    rows = a.time_correlation()[0]
    assert [r["origins"] for r in rows] == [20, 19, 18, 17] and [r["sum_steps"] for r in rows] == [0, 19, 36, 51]
    # again: restarts at record 0 with a zeroed table
    a.set_time_correlation(0.05, 64, RADIUS)
    assert a.time_correlation_info() == {"interval": float(f32(0.05)), "lags": 64, "overlap_radius": RADIUS, "records": 0}
    zero = a.time_correlation()[0]
    assert len(zero) == 64 and zero == [dict(dict.fromkeys(TR.FIELDS, 0), lag=l) for l in range(64)]
    gates = SR.gate_steps(a.time, DT, 0.05, 30, 1e9)
    assert a.step(30, dt=DT, sort_interval=SORT) == 30
    rows = a.time_correlation()[0]
    assert a.time_correlation_info()["records"] == len(gates) and 5 <= len(gates) <= 7
    assert [r["origins"] for r in rows] == [max(len(gates) - l, 0) for l in range(64)]
    assert rows[1]["sum_steps"] == gates[-1][0] - gates[0][0]
    # lags 0 frees: later steps record nothing and are fused again
    a.set_time_correlation(0.05, 0, 0.0)
    assert a.time_correlation_info() == OFF
    stats = a.stats()
    assert a.step(30, dt=DT, sort_interval=SORT) == 30 and a.time_correlation_info() == OFF
    assert a.stats()["fused_launches"] == stats["fused_launches"] + 29  # every step but the call's last is fused again
    with pytest.raises(RuntimeError, match="code 2.*the correlation is off"):
        a.time_correlation()
    assert a.time_correlation_times() == (0, 0.0)


def test_no_record_for_the_step_that_max_time_stops(pb, orc):
    gates = SR.gate_steps(0.0, DT, 0.0, 50, 0.1)
    a = light_wave_sim(pb, orc, FORMS["fused"], max_time=0.1)
    a.set_time_correlation(0.0, 4, RADIUS)
    done = a.step(50, dt=DT, sort_interval=SORT)
    assert done == len(gates) and 10 <= done <= 12
    assert a.time_correlation_info()["records"] == done and a.step(5, dt=DT, sort_interval=SORT) == 0
    assert a.time_correlation_info()["records"] == done
    assert [r["origins"] for r in a.time_correlation()[0]] == [done - l for l in range(4)]


# ---- the refusals that need a live batch -----------------------------------------------------------------------------
# Not run here: a batch of 2^28 bots or more (its state alone is tens of gigabytes, tests/soak_huge_arena.py) and a batch
# of more than 65535 members (65536 parameter blocks and cell lists to build): neither fits a test of a few seconds.
# They are two comparisons in front of the ring-size test below, in pbSimSetTimeCorrelation.

def test_a_ring_above_2_33_bytes_is_refused_before_anything_is_allocated(pb, orc):
    n = (1 << 23) + 1  # 64 lags x n x 16 bytes = 2^33 + 1024
    P = orc.default_params(nCells=n, nDead=0, seed=3, max_time=1e9)
    sp, keep = simparams_from_orc(P)
    sim = pb.Sim(sp, wall_half=4.0e6, keepalive=keep)
    with pytest.raises(RuntimeError, match="code 2.*pbSimSetTimeCorrelation.*2\\^33 bytes"):
        sim.set_time_correlation(-1.0, 64, 0.1)
    assert sim.time_correlation_info() == OFF
    with pytest.raises(RuntimeError, match="code 2.*the correlation is off"):
        sim.time_correlation_record()
    sim.set_time_correlation(-1.0, 1, 0.1)  # the same batch with a ring that fits
    sim.time_correlation_record()
    assert sim.time_correlation()[0][0]["origins"] == 1 and sim.time_correlation_info()["records"] == 1
    sim.close()


def test_a_lag_with_2_31_samples_is_refused_and_a_restart_recovers(pb, orc):
    from particlerobotsimulations_amd import _capi
    n = 1 << 20  # 2048 records of 2^20 bots are 2^31 samples in lag 0; 2047 are not
    rng = np.random.default_rng(31)
    g = np.arange(1024, dtype=f32) * f32(0.25) - f32(128.0)
    pos = np.stack(np.meshgrid(g, g), -1).reshape(n, 2).astype(f32)
    vel = (rng.integers(-512, 513, size=(n, 2)).astype(f32) / f32(4096.0)).astype(f32)
    sim = sim_with(pb, orc, pos, vel, np.full(n, 0.1, f32))
    st = sim.get_state()
    w = np.rint(st["vel"].astype(np.float64) * 2.0 ** 20).astype(np.int64)  # multiples of 2^-12: exact
    w2 = int((w * w).sum())                                               # below 2^20 x 2 x 2^34: int64 holds it
    sim.set_time_correlation(-1.0, 1, 0.5)
    for _ in range(2047):
        sim.time_correlation_record()
    row = sim.time_correlation()[0][0]
    assert row == {"lag": 0, "origins": 2047, "sum_steps": 0, "samples": 2047 << 20, "sum_qx": 0, "sum_qy": 0, "msd": 0,
                   "vacf": 2047 * w2, "overlap": 2047 << 20, "max_q2": 0}
    assert row["samples"] == (1 << 31) - (1 << 20) and row["vacf"] > 1 << 63
    sim.time_correlation_record()
    rows = (_capi.pbTimeCorrelationRow * 1)(_capi.pbTimeCorrelationRow(lag=7, samples=7))
    assert _capi.lib().pbSimGetTimeCorrelation(sim._h, rows) == 2  # PB_ERR_ARG
    assert b"a lag holds 2^31 samples or more: restart the correlation" in _capi.lib().pbGetLastErrorString()
    assert (rows[0].lag, rows[0].samples, rows[0].origins) == (7, 7, 0)  # no row was written
    with pytest.raises(RuntimeError, match="code 2.*pbSimGetTimeCorrelation.*2\\^31 samples"):
        sim.time_correlation()
    assert sim.time_correlation_info()["records"] == 2048
    sim.set_time_correlation(-1.0, 1, 0.5)  # the restart
    assert sim.time_correlation_info()["records"] == 0
    sim.time_correlation_record()
    assert sim.time_correlation()[0][0] == dict(row, origins=1, samples=n, vacf=w2, overlap=n)
    sim.close()


# ---- the runner ------------------------------------------------------------------------------------------------------

HEADER = "Lag, Origins, SumSteps, Samples, SumQx, SumQy, SumQ2, SumWW, Overlap, MaxQ2"
COLUMNS = ("lag", "origins", "sum_steps", "samples", "sum_qx", "sum_qy", "msd", "vacf", "overlap", "max_q2")


def test_runner_writes_the_table_at_the_end_of_the_run(tmp_path):
    from particlerobotsimulations_amd import host
    over = dict(max_time="30", dump_interval="2.5")
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--timecorr", "t.csv", "--timecorr-lags", "4"],
                       capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "t.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 5
    cells = [[int(c) for c in l.split(", ")] for l in lines[1:]]
    assert [c[0] for c in cells] == [0, 1, 2, 3] and [c[1] for c in cells] == [12, 11, 10, 9]
    assert all(c[3] == 300 * c[1] for c in cells)
    # the same rows from the class driven in-process, with the runner's defaults
    flat = host.load_config(CFG, **over)
    h = host.HostSim(CFG, engine="fused", **over)
    h.set_time_correlation(flat.dump_interval, 4, flat.min_radius)
    assert h.time_correlation_info() == {"interval": float(f32(flat.dump_interval)), "lags": 4,
                                         "overlap_radius": float(f32(flat.min_radius)), "records": 0}
    while not h.finished:
        if h.advance(h.steps_until_dump()) == 0:
            break
    want = h.time_correlation()[0]
    assert lines[1:] == [", ".join(str(w[k]) for k in COLUMNS) for w in want]
    assert h.time_correlation_info()["records"] == 12
    h.time_correlation_record()
    assert h.time_correlation_info()["records"] == 13
    h.close()


def test_runner_refuses_a_run_whose_table_cannot_fit(tmp_path):
    # 300 bots, a record every 0.01 s up to 10^5 s: 10^7 records, 3 x 10^9 samples in lag 0
    r = subprocess.run([RUN, CFG, "--quiet", "--set", "max_time", "100000", "--timecorr", "t.csv", "--timecorr-interval",
                        "0.01"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 2 and r.stdout == ""
    assert r.stderr == ("--timecorr: about 10000002 records of 300 bots would pass 2^31 samples per lag: raise "
                        "--timecorr-interval or lower max_time\n")
    assert not os.path.exists(tmp_path / "t.csv")
