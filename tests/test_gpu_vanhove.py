"""GPU: the self van Hove function (pbSimSetVanHove / pbSimVanHoveRecord / pbSimGetVanHove, csrc/pb_vanhove.hip) against
tests/vanhove_ref.py on states read back from the device.  Every comparison is exact: a row and its histograms hold
integers only.  A table recorded while stepping is compared with a twin run that has the analysis off and is stopped in
front of every step the gate names.  tests/test_vanhove_api.py pins the reference to a plain loop and to known answers
on the CPU, and shows that the recipe used here fills a histogram.

Not run here, as in tests/test_gpu_timecorr.py: the refusals that need a batch of 2^28 bots, of more than 65535 members,
a ring above 2^33 bytes (2^24 bots at 64 lags) or a table above 2^31 bytes (more than 800 members at 64 lags and 1024
bins), and a cell with 2^31 samples: none fits a test of a few seconds.  They are comparisons in front of the allocation
in pbSimSetVanHove, and pbLagFetch's in front of the rows in pbSimGetVanHove."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import series_ref as SR
import timecorr_ref as TR
import vanhove_ref as VR
from helpers import assert_bit_equal
from test_gpu_scatter import stepping_sim
from test_gpu_series import DT, FORMS, INTERVAL, PUI, SORT, STEPS, layout_of, make_batch, sim_with
from test_gpu_sfactor import live_memory
from test_gpu_timecorr import same_bits, twin_states
from test_series_api import CORNER, recipe
from test_timecorr_api import BATCH_BOTS, batch_records
from test_vanhove_api import (KNOWN_BINS, KNOWN_WIDTH, MANUAL_LAGS, MANUAL_RECORDS, TOP, known_answer_records,
                              known_answer_rows, unmeasured_positions, vanhove_records)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
SHAPES = [(0.125, 64), (0.3, 1024), (2.0 ** -20, 1), (2047.5, 2), (0.125, 16)]  # (width, bins), cycled over the sizes
LAGS, BINS = 5, 64  # while stepping
OFF = {"interval": 0.0, "lags": 0, "width": 0.0, "bins": 0, "records": 0}


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def header_constant(name):
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    return int(re.search(r"#define %s (\d+)u" % name, header).group(1))


def record_manually(sim, records, lags, width, bins):
    """Sets each of `records` (positions) and takes a record of it; returns the member's rows and the positions read
    back."""
    n = len(records[0])
    sim.set_van_hove(-1.0, lags, width, bins)
    assert sim.van_hove_info() == {"interval": -1.0, "lags": lags, "width": float(f32(width)), "bins": bins, "records": 0}
    back = []
    zeros = np.zeros((n, 2), f32)
    for pos in records:
        sim.set_state(pos=pos, vel=zeros, rad=np.full(n, 0.1, f32), phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
        back.append(sim.get_state()["pos"])
        sim.van_hove_record()
    assert sim.van_hove_info()["records"] == len(records)
    return sim.van_hove()[0], back


def fresh_sim(pb, orc, n):
    return sim_with(pb, orc, np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.full(n, 0.1, f32))


# ---- manual records on set states ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", ["origin", "corner"])
def test_manual_records_around_the_wave_and_the_workgroup(pb, orc, n, where):
    width, bins = SHAPES[(SIZES.index(n) + (where == "corner")) % len(SHAPES)]
    recs = [r[0] for r in vanhove_records(n, center=CORNER if where == "corner" else (0.0, 0.0))]
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, MANUAL_LAGS, width, bins)
    for p, rec in zip(back, recs):
        assert same_bits(p, rec)
    want = VR.table(back, [0] * MANUAL_RECORDS, MANUAL_LAGS, width, bins)
    print(n, where, width, bins, {k: rows[1][k] for k in VR.FIELDS})
    assert rows == want, (n, where, width, bins)
    assert all(VR.identities_hold(r) for r in rows)
    assert [r["origins"] for r in rows] == [7, 6, 5] and [r["samples"] for r in rows] == [7 * n, 6 * n, 5 * n]
    assert rows[0]["msd"] == 0 and rows[0]["radial"][0] == 7 * n and rows[0]["x"][bins] == 7 * n == rows[0]["y"][bins]
    assert rows[1]["msd"] > 0 and rows[1]["q4"] > 0
    sim.close()


def test_more_bots_than_one_pass_covers(pb, orc):
    n = header_constant("PB_VANHOVE_BLOCKS") * 256 + 321  # the grid-stride loop runs twice for 321 lanes
    assert n == 65857
    recs = [r[0] for r in vanhove_records(n, records=3, center=(-300.0, 700.0))]
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, 2, 0.125, 64)
    want = VR.table(back, [0] * 3, 2, 0.125, 64)
    assert rows == want
    assert all(VR.identities_hold(r) for r in rows)
    assert [r["samples"] for r in rows] == [3 * n, 2 * n] and rows[1]["msd"] > 1 << 56 and rows[1]["q4"] > 1 << 100
    assert sum(1 for c in rows[1]["radial"] if c) >= 32
    sim.close()


def test_known_answers_and_unmeasured_pairs(pb, orc):
    recs = known_answer_records()
    sim = fresh_sim(pb, orc, 8)
    rows, back = record_manually(sim, recs, 2, KNOWN_WIDTH, KNOWN_BINS)
    for p, rec in zip(back, recs):
        assert same_bits(p, rec)
    assert rows == VR.table(back, [0, 0], 2, KNOWN_WIDTH, KNOWN_BINS)
    assert rows == [dict(k, sum_steps=0) for k in known_answer_rows()]  # (no step ran between the records)
    sim.close()
    p, bad1, bad0 = unmeasured_positions()
    sim = fresh_sim(pb, orc, 257)
    rows, back = record_manually(sim, p, 2, 64.0, 32)
    for got, put in zip(back, p):
        nan = np.isnan(put)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], put[~nan])
    assert rows == VR.table(back, [0, 0], 2, 64.0, 32)
    assert all(VR.identities_hold(r) for r in rows)
    assert rows[1]["samples"] == 257 - len(bad1) == 243 and rows[0]["samples"] == 2 * 257 - 12
    assert rows[1]["radial"][31] == 2 and rows[1]["x"][63] == 1 and rows[1]["y"][0] == 1 and rows[1]["q4"] >= 2 * TOP ** 4
    sim.close()
    # no measured pair: an all-zero table
    bad = np.full((65, 2), np.nan, f32)
    sim = fresh_sim(pb, orc, 65)
    rows, _ = record_manually(sim, [bad, bad], 2, 0.5, 4)
    assert rows == [dict(VR.empty_row(0, 4), origins=2), dict(VR.empty_row(1, 4), origins=1)]
    sim.close()


def test_batch_of_three_members_do_not_leak_into_each_other(pb, orc):
    n, recs = BATCH_BOTS, batch_records()
    ens = make_batch(pb, orc, 3, n)
    ens.set_van_hove(-1.0, 3, 0.25, 32)
    back = [[] for _ in range(3)]
    for r in range(4):
        for k in range(3):
            pos, vel, rad = recs[k][r]
            ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
            st = ens.get_state_of(k)
            assert same_bits(st["pos"], pos)
            back[k].append(st["pos"])
        ens.van_hove_record()
    rows = ens.van_hove()
    assert len(rows) == 3 and all(len(r) == 3 for r in rows)
    for k in range(3):
        assert rows[k] == VR.table(back[k], [0] * 4, 3, 0.25, 32), k
        assert [r["samples"] for r in rows[k]] == [4 * n, 3 * n, 2 * n] and all(VR.identities_hold(r) for r in rows[k])
    assert rows[0][1] != rows[1][1] != rows[2][1] and rows[0][1]["msd"] < rows[2][1]["msd"]
    assert ens.van_hove() == rows  # twice: the same rows
    ens.close()


# ---- recorded while stepping -----------------------------------------------------------------------------------------

def width_for(states, rec):
    """The smallest power of two w such that BINS bins of w hold every displacement of the twin's records at every lag."""
    most = 0
    for r in range(len(states)):
        for l in range(min(r, LAGS - 1) + 1):
            most = max([most] + [qx * qx + qy * qy for qx, qy in VR.quantised_pairs(states[r], states[r - l])])
    e = -20
    while (BINS << (20 + e)) ** 2 <= most:
        e += 1
    return 2.0 ** e


@pytest.mark.parametrize("wave", [True, False], ids=["wave", "no_wave"])
@pytest.mark.parametrize("name", list(FORMS))
def test_recorded_table_equals_a_twin_and_leaves_the_run_and_the_other_recorders_alone(pb, orc, name, wave):
    form = FORMS[name]
    interval, steps = (0.0, 120) if name == "every_step" else (INTERVAL, STEPS)
    gates = SR.gate_steps(0.0, DT, interval, steps, 1e9)
    rec = [k for k, _ in gates]
    sorts = [k for k, _ in SR.gate_steps(0.0, DT, SORT, steps, 1e9)]
    phases = [k for k, _ in SR.gate_steps(0.0, DT, PUI, steps, 1e9)] if wave else []
    assert len(rec) > LAGS  # the ring wraps
    # b: the twin, everything off, run first: its states choose the width
    b = stepping_sim(pb, orc, form, wave)
    states = twin_states(b, gates, steps)[0]
    positions = [p for p, _ in states]
    width = width_for(positions, rec)
    want = VR.table(positions, rec, LAGS, width, BINS)
    assert sum(1 for c in want[LAGS - 1]["radial"] if c) >= 4 and all(w["beyond_r"] == 0 for w in want), width
    # a: the van Hove function alone; c: all four recorders; d: the time correlation alone; e: the series alone;
    # g: the scattering alone
    a, c, d, e, g = (stepping_sim(pb, orc, form, wave) for _ in range(5))
    assert a.config()["resident"] == (1 if name == "resident" else 0)
    vectors = pb.half_plane_vectors(2)
    for s in (a, c):
        s.set_van_hove(interval, LAGS, width, BINS)
    for s in (c, d):
        s.set_time_correlation(interval, LAGS, 0.015625)
    for s in (c, e):
        s.set_series(interval, 512)
    for s in (c, g):
        s.set_scattering(interval, LAGS, 3, vectors)
    assert a.van_hove_info() == {"interval": float(f32(interval)), "lags": LAGS, "width": width, "bins": BINS, "records": 0}
    for s in (a, c, d, e, g):
        assert s.step(steps, dt=DT, sort_interval=SORT) == steps  # one call
    assert a.van_hove_info()["records"] == c.van_hove_info()["records"] == len(rec)
    got = a.van_hove()[0]
    print(name, wave, width, {k: got[LAGS - 1][k] for k in VR.FIELDS})
    assert got == want, (name, wave)
    assert all(VR.identities_hold(r) for r in got)
    assert [r["origins"] for r in got] == [len(rec) - l for l in range(LAGS)]
    assert all(r["samples"] == 300 * r["origins"] for r in got)
    lay = layout_of(a)
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(300))  # sorted: the slots are not in original order
    # the final state is the twin's, bit for bit, whichever recorders ran
    sb = b.get_state()
    for s in (a, c, d, e, g):
        st = s.get_state()
        for k in sb:
            assert_bit_equal(st[k], sb[k], f"{name} {k}")
        assert s.time == b.time
    # each recorder gives what it gives alone
    assert c.van_hove()[0] == got
    tc = c.time_correlation()
    assert tc == d.time_correlation() and tc[0] == TR.table(states, rec, LAGS, 0.015625)
    assert c.series_of(0) == e.series_of(0) and len(e.series_of(0)) == len(rec)
    assert c.scattering() == g.scattering()
    # the histogram is the distribution whose second moment the time correlation's msd is
    assert [(r["msd"], r["samples"]) for r in got] == [(t["msd"], t["samples"]) for t in tc[0]]
    # the launches are those of a run with only the time correlation on at that interval
    assert a.stats() == d.stats() == c.stats() == e.stats() == g.stats()
    assert a.stats()["steps"] == steps and a.stats()["resorts"] == len(sorts) and a.stats()["phase_updates"] == len(phases)
    if name == "resident":
        assert a.stats()["resident_launches"] > 0
    if name == "every_step":
        assert a.stats()["fused_launches"] == 0  # interval 0 costs the fusion
    elif name != "resident":
        assert a.stats()["fused_launches"] > 0
    s = pb.van_hove_summary(got[LAGS - 1], width)
    assert s["msd"] > 0.0 and s["alpha2"] > -1.0 and s["mean_lag_steps"] == got[LAGS - 1]["sum_steps"] / got[LAGS - 1]["origins"]
    n, ms = a.van_hove_times()
    assert n == len(rec) and ms > 0.0
    for s in (a, b, c, d, e, g):
        s.close()


def test_reading_and_recording_change_nothing(pb, orc):
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, phase_update_interval=0.3)
    vectors = pb.half_plane_vectors(1)
    sim.set_series(0.1, 8)
    sim.set_time_correlation(0.1, 3, 0.5)
    sim.set_scattering(0.1, 3, 3, vectors)
    sim.set_van_hove(-1.0, 3, 0.03125, 32)
    assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    assert sim.van_hove_info()["records"] == 0  # manual only
    before, stats, lay, t = sim.get_state(), sim.stats(), layout_of(sim), sim.time
    series, corr, scat = sim.series_of(0), sim.time_correlation(), sim.scattering()
    sim.van_hove_record()
    sim.van_hove_record()
    first = sim.van_hove()
    assert first == sim.van_hove()
    assert first[0] == VR.table([before["pos"]] * 2, [60, 60], 3, 0.03125, 32)
    after = sim.get_state()
    for k in before:
        assert_bit_equal(before[k], after[k], k)
    assert sim.stats() == stats and sim.time == t
    assert sim.series_of(0) == series and sim.time_correlation() == corr and sim.scattering() == scat
    for x, y in zip(lay, layout_of(sim)):
        assert np.array_equal(x, y)
    # a later step and a set_state leave the ring alone: the next record pairs with the two it holds
    assert sim.step(7, dt=DT, sort_interval=0.2) == 7
    now = sim.get_state()
    sim.set_state(pos=now["pos"], vel=now["vel"], rad=now["rad"], phase=now["phase"], dead=now["dead"])
    sim.van_hove_record()
    rows = sim.van_hove()[0]
    assert rows == VR.table([before["pos"]] * 2 + [now["pos"]], [60, 60, 67], 3, 0.03125, 32)
    assert rows[1]["sum_steps"] == 7 and rows[2]["sum_steps"] == 7 and rows[1]["msd"] > 0
    assert sim.van_hove_times()[0] == 3 and sim.van_hove_times()[1] > 0.0
    sim.close()


# ---- life cycle --------------------------------------------------------------------------------------------------------

def test_restart_switch_off_and_argument_errors(pb, orc):
    start = live_memory()
    pos, vel, rad = recipe(300)
    a = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0, phase_update_interval=PUI)
    a.set_resident(1)
    made = live_memory()
    assert a.van_hove_info() == OFF and a.van_hove_times() == (0, 0.0)
    for call in (a.van_hove_record, a.van_hove):
        with pytest.raises(RuntimeError, match="code 2.*the van Hove function is off"):
            call()
    for bad, word in (((-0.5, 4, 0.125, 64), "interval"), ((float("nan"), 4, 0.125, 64), "interval"),
                      ((0.0, 65, 0.125, 64), "lags"), ((0.0, 4, 0.125, 0), "bins"), ((0.0, 4, 0.125, 1025), "bins"),
                      ((0.0, 4, 0.0, 64), "binWidth"), ((0.0, 4, 2048.0, 64), "binWidth"),
                      ((0.0, 4, float("nan"), 64), "binWidth"), ((0.0, 4, 2.0 ** -22, 64), "quantum")):
        with pytest.raises(RuntimeError, match="code 2.*pbSimSetVanHove.*" + word):
            a.set_van_hove(*bad)
    assert a.van_hove_info() == OFF and live_memory() == made
    a.set_van_hove(0.0, 4, 0.125, 48)
    # the ring, the table (ten moments and 5 x 48 counters per lag) and the 49 edges
    assert live_memory() == (made[0] + 3, made[1] + 4 * 300 * 8 + 4 * (10 + 5 * 48) * 8 + 49 * 8)
    assert a.step(20, dt=DT, sort_interval=SORT) == 20 and a.van_hove_info()["records"] == 20
    rows = a.van_hove()[0]
    assert [r["origins"] for r in rows] == [20, 19, 18, 17] and [r["sum_steps"] for r in rows] == [0, 19, 36, 51]
    assert all(VR.identities_hold(r) and r["samples"] == 300 * r["origins"] for r in rows)
    # again: restarts at record 0 with a zeroed table
    a.set_van_hove(0.05, 64, 0.5, 7)
    assert a.van_hove_info() == {"interval": float(f32(0.05)), "lags": 64, "width": 0.5, "bins": 7, "records": 0}
    zero = a.van_hove()[0]
    assert zero == [VR.empty_row(l, 7) for l in range(64)]
    gates = SR.gate_steps(a.time, DT, 0.05, 30, 1e9)
    assert a.step(30, dt=DT, sort_interval=SORT) == 30
    rows = a.van_hove()[0]
    assert a.van_hove_info()["records"] == len(gates) and 5 <= len(gates) <= 7
    assert [r["origins"] for r in rows] == [max(len(gates) - l, 0) for l in range(64)]
    assert rows[1]["sum_steps"] == gates[-1][0] - gates[0][0]
    # lags 0 frees: the memory is back, later steps record nothing and are fused again
    a.set_van_hove(0.05, 0, 0.0, 0)
    assert a.van_hove_info() == OFF and live_memory() == made
    stats = a.stats()
    assert a.step(30, dt=DT, sort_interval=SORT) == 30 and a.van_hove_info() == OFF
    assert a.stats()["fused_launches"] == stats["fused_launches"] + 29  # every step but the call's last is fused again
    with pytest.raises(RuntimeError, match="code 2.*the van Hove function is off"):
        a.van_hove()
    assert a.van_hove_times() == (0, 0.0)
    # destroyed with the ring live: nothing stays
    a.set_van_hove(-1.0, 2, 1.0, 1)
    a.van_hove_record()
    assert live_memory()[0] == made[0] + 3
    a.close()
    assert live_memory() == start


# ---- the runner ------------------------------------------------------------------------------------------------------

HEADER = "Lag, Origins, SumSteps, Samples, SumQ2, SumQ4, Alpha2, Axis, Bin, Lower, Count"


def expected_lines(pb, rows, width, bins):
    """The file of --vanhove from the rows of van_hove(): the integers as text, the two floats as numbers."""
    qw = VR.qw_of(width) / 2.0 ** 20
    out = []
    for row in rows:
        lead = [str(row[k]) for k in ("lag", "origins", "sum_steps", "samples", "msd", "q4")]
        alpha2 = pb.van_hove_summary(row, width)["alpha2"]
        for axis, key, first, end in (("r", "radial", 0, bins * qw), ("x", "x", -bins, math.nan), ("y", "y", -bins, math.nan)):
            for j, count in enumerate(row[key]):
                out.append((lead, alpha2, axis, j, (first + j) * qw, count))
            out.append((lead, alpha2, axis, -1, end, row["beyond_" + ("r" if axis == "r" else axis)]))
    return out


def same_number(text, value):
    got = float(text)
    return (math.isnan(got) and math.isnan(value)) or got == pytest.approx(value, rel=1e-8, abs=0.0)


def test_runner_writes_the_table_at_the_end_of_the_run(pb, tmp_path):
    from particlerobotsimulations_amd import host
    over = dict(max_time="30", dump_interval="2.5")
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--vanhove", "g.csv", "--vanhove-lags", "4", "--vanhove-bins", "16",
                                                      "--vanhove-width", "0.03125"],
                       capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "g.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 4 * (5 * 16 + 3)
    cells = [l.split(", ") for l in lines[1:]]
    # the same rows from the class driven in-process
    h = host.HostSim(CFG, engine="fused", **over)
    flat = host.load_config(CFG, **over)
    h.set_van_hove(flat.dump_interval, 4, 0.03125, 16)
    assert h.van_hove_info() == {"interval": float(f32(flat.dump_interval)), "lags": 4, "width": 0.03125, "bins": 16,
                                 "records": 0}
    while not h.finished:
        if h.advance(h.steps_until_dump()) == 0:
            break
    rows = h.van_hove()[0]
    assert [r["origins"] for r in rows] == [12, 11, 10, 9] and all(r["samples"] == 300 * r["origins"] for r in rows)
    assert all(VR.identities_hold(r) for r in rows) and rows[3]["msd"] > 0
    want = expected_lines(pb, rows, 0.03125, 16)
    assert len(want) == len(cells)
    for c, (lead, alpha2, axis, j, lower, count) in zip(cells, want):
        assert c[:6] == lead and c[7:9] == [axis, str(j)] and c[10] == str(count), (c, lead, axis, j)
        assert same_number(c[6], alpha2) and same_number(c[9], lower), (c, alpha2, lower)
    assert h.van_hove_info()["records"] == 12
    h.van_hove_record()
    assert h.van_hove_info()["records"] == 13
    h.close()
    # the defaults: 32 lags of 64 bins, an eighth of min_radius wide
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--vanhove", "d.csv"], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "d.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 32 * (5 * 64 + 3)
    cells = [l.split(", ") for l in lines[1:]]
    assert [int(c[0]) for c in cells[::323]] == list(range(32)) and [c[7] for c in cells[:323:1]].count("r") == 65
    eighth = VR.qw_of(f32(0.125) * f32(flat.min_radius)) / 2.0 ** 20
    assert same_number(cells[1][9], eighth) and same_number(cells[64][9], 64 * eighth) and cells[64][8] == "-1"


def test_runner_refuses_a_run_whose_table_cannot_fit(tmp_path):
    # 300 bots, a record every 0.01 s up to 10^5 s: 10^7 records, 3 x 10^9 samples in lag 0
    r = subprocess.run([RUN, CFG, "--quiet", "--set", "max_time", "100000", "--vanhove", "g.csv", "--vanhove-interval",
                        "0.01"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 2 and r.stdout == ""
    assert r.stderr == ("--vanhove: about 10000002 records of 300 bots would pass 2^31 samples per lag: raise "
                        "--vanhove-interval or lower max_time\n")
    assert not os.path.exists(tmp_path / "g.csv")
