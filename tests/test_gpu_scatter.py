"""GPU: the self-intermediate scattering function (pbSimSetScattering / pbSimScatteringRecord / pbSimGetScattering,
csrc/pb_scatter.hip) against tests/scatter_ref.py on states read back from the device.  Every comparison is exact: a row
holds integers only.  A table recorded while stepping is compared with a twin run that has the scattering off and is
stopped in front of every step the gate names.  tests/test_scatter_api.py pins the reference to a plain loop and to known
answers on the CPU, and shows that the recipes used here keep every pair measured.

Not run here, as in tests/test_gpu_timecorr.py: the refusals that need a batch of 2^28 bots, of more than 65535 members,
a ring above 2^33 bytes (2^24 bots at 64 lags) or a table above 2^31 bytes (more than 8192 members at 64 lags and 256
vectors), and a cell with 2^31 samples: none fits a test of a few seconds.  They are comparisons in front of the
allocation in pbSimSetScattering and one in front of the rows in pbSimGetScattering."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import scatter_ref as XR
import series_ref as SR
import timecorr_ref as TR
from helpers import assert_bit_equal
from test_gpu_series import DT, FORMS, INTERVAL, PUI, SORT, STEPS, layout_of, make_batch, sim_with
from test_gpu_sfactor import live_memory
from test_gpu_timecorr import same_bits, twin_states
from test_scatter_api import (BATCH_LAGS, BOXES, L_LOG2, MANUAL_LAGS, MANUAL_RECORDS, NVECS, SIZES, dyadic_positions,
                              float64_records, known_cases, phase_bound, positions, unmeasured_records,
                              unmeasured_samples, vector_list)
from test_series_api import CORNER, recipe
from test_timecorr_api import BATCH_BOTS, batch_records, manual_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
LAGS, BOX = 5, 3  # while stepping
OFF = {"interval": 0.0, "lags": 0, "box_log2": 0, "nvec": 0, "records": 0}


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def header_constant(name):
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    return int(re.search(r"#define %s (\d+)u" % name, header).group(1))


def record_manually(sim, records, lags, box_log2, vectors):
    """Sets each of `records` (positions) and takes a record of it; returns the member's rows and the positions read
    back."""
    n = len(records[0])
    sim.set_scattering(-1.0, lags, box_log2, vectors)
    assert sim.scattering_info() == {"interval": -1.0, "lags": lags, "box_log2": box_log2, "nvec": len(vectors),
                                     "records": 0}
    back = []
    zeros = np.zeros((n, 2), f32)
    for pos in records:
        sim.set_state(pos=pos, vel=zeros, rad=np.full(n, 0.1, f32), phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
        back.append(sim.get_state()["pos"])
        sim.scattering_record()
    assert sim.scattering_info()["records"] == len(records)
    return sim.scattering()[0], back


def fresh_sim(pb, orc, n):
    return sim_with(pb, orc, np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.full(n, 0.1, f32))


# ---- manual records on set states ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", ["origin", "corner"])
def test_manual_records_around_the_wave_and_the_workgroup(pb, orc, n, where):
    k = SIZES.index(n) + (len(SIZES) if where == "corner" else 0)
    nvec, box = NVECS[k % len(NVECS)], BOXES[k % len(BOXES)]  # (16 cases: every nvec and every box several times)
    vectors = vector_list(nvec)
    recs = positions(manual_records(n, CORNER if where == "corner" else (0.0, 0.0), records=MANUAL_RECORDS))
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, MANUAL_LAGS, box, vectors)
    for got, put in zip(back, recs):
        assert same_bits(got, put)
    want = XR.table(back, [0] * MANUAL_RECORDS, MANUAL_LAGS, vectors, box)
    print(n, where, nvec, box, rows[1][0])
    assert rows == want, (n, where, nvec, box)
    assert [r[0]["origins"] for r in rows] == [7, 6, 5] and [r[-1]["samples"] for r in rows] == [7 * n, 6 * n, 5 * n]
    assert all(r["re"] == 7 * n << 30 and r["im"] == 0 and r["sum_steps"] == 0 for r in rows[0])
    sim.close()


@pytest.mark.parametrize("nvec", NVECS)
@pytest.mark.parametrize("box", BOXES)
def test_every_list_length_in_every_box(pb, orc, nvec, box):
    n = 257
    vectors = vector_list(nvec)
    recs = positions(manual_records(n, (1.5, -2.25), records=MANUAL_RECORDS))
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, MANUAL_LAGS, box, vectors)
    want = XR.table(back, [0] * MANUAL_RECORDS, MANUAL_LAGS, vectors, box)
    assert rows == want, (nvec, box)
    assert [[r["nx"], r["ny"]] for r in rows[2]] == vectors.tolist()
    assert all(r["samples"] == (7 - l) * n for l in range(3) for r in rows[l])
    if nvec >= 3:
        assert rows[1][0] == rows[1][2] and rows[1][0]["re"] != rows[0][0]["re"]  # the repeated vector; a lag that moved
    sim.close()


def test_more_bots_than_one_pass_covers(pb, orc):
    n = header_constant("PB_SCATTER_BLOCKS") * 256 + 321  # the block loop runs twice for 321 lanes
    assert n == 65857
    recs = positions(manual_records(n, (-300.0, 700.0), records=3))
    vectors = vector_list(3)
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, 2, 3, vectors)
    assert rows == XR.table(back, [0] * 3, 2, vectors, 3)
    assert [r[0]["samples"] for r in rows] == [3 * n, 2 * n]
    sim.close()


def test_known_answers_on_dyadic_positions(pb, orc):
    pos = dyadic_positions()
    n = len(pos)
    sim = fresh_sim(pb, orc, n)
    for shift, vec, (re, im) in known_cases():
        moved = (pos + np.array(shift, f32)).astype(f32)
        rows, back = record_manually(sim, [pos, moved], 2, L_LOG2, np.array([vec], np.int32))
        assert same_bits(back[0], pos) and same_bits(back[1], moved)
        assert rows[0][0] == {"lag": 0, "nx": vec[0], "ny": vec[1], "origins": 2, "sum_steps": 0, "samples": 2 * n,
                              "re": (2 * n) << 30, "im": 0}, (shift, vec)
        assert rows[1][0] == {"lag": 1, "nx": vec[0], "ny": vec[1], "origins": 1, "sum_steps": 0, "samples": n,
                              "re": n * re, "im": n * im}, (shift, vec, rows[1][0])
    sim.close()


def test_unmeasured_pairs(pb, orc):
    recs, bad = unmeasured_records()
    vectors = vector_list(3)
    sim = fresh_sim(pb, orc, 257)
    rows, back = record_manually(sim, recs, 3, 3, vectors)
    for got, put in zip(back, recs):
        nan = np.isnan(put)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], put[~nan])
    assert rows == XR.table(back, [0, 0, 0], 3, vectors, 3)
    assert [r[0]["samples"] for r in rows] == unmeasured_samples(257, bad) == [3 * 257 - 36, 2 * 257 - 48, 257 - 24]
    # no measured pair: an all-zero table with the right origins
    far = np.full((65, 2), 3000.0, f32)
    far[::2, 1] = np.inf
    sim = fresh_sim(pb, orc, 65)
    rows, _ = record_manually(sim, [far, far], 2, 3, vectors)
    zero = dict.fromkeys(XR.FIELDS, 0)
    assert rows == [[dict(zero, lag=l, nx=int(nx), ny=int(ny), origins=2 - l) for nx, ny in vectors] for l in range(2)]
    sim.close()


def test_batch_of_three_members_do_not_leak_into_each_other(pb, orc):
    n, recs = BATCH_BOTS, batch_records()
    vectors = vector_list(65)
    ens = make_batch(pb, orc, 3, n)
    ens.set_scattering(-1.0, BATCH_LAGS, 4, vectors)
    back = [[] for _ in range(3)]
    for r in range(4):
        for k in range(3):
            pos, vel, rad = recs[k][r]
            ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
            st = ens.get_state_of(k)
            assert same_bits(st["pos"], pos)
            back[k].append(st["pos"])
        ens.scattering_record()
    rows = ens.scattering()
    assert len(rows) == 3 and all(len(r) == BATCH_LAGS and len(r[0]) == 65 for r in rows)
    for k in range(3):
        assert rows[k] == XR.table(back[k], [0] * 4, BATCH_LAGS, vectors, 4), k
        assert [r[0]["samples"] for r in rows[k]] == [4 * n, 3 * n, 2 * n]
    assert rows[0][1] != rows[1][1] != rows[2][1]
    assert ens.scattering() == rows  # twice: the same rows
    ens.close()


def test_against_float64_within_the_derived_bound(pb, orc):
    recs = float64_records()
    vectors = pb.half_plane_vectors(3)
    sim = fresh_sim(pb, orc, len(recs[0]))
    rows, back = record_manually(sim, recs, 2, 3, vectors)
    dr = back[1].astype(np.float64) - back[0].astype(np.float64)
    for row in rows[1]:
        phase = 2 * np.pi / 8.0 * (row["nx"] * dr[:, 0] + row["ny"] * dr[:, 1])
        bound = phase_bound(row["nx"], row["ny"], 3)
        s = pb.scattering_summary(row)
        print(row["nx"], row["ny"], abs(s["fs_re"] - np.cos(phase).mean()), abs(s["fs_im"] - np.sin(phase).mean()), bound)
        assert row["samples"] == 1000
        assert abs(s["fs_re"] - np.cos(phase).mean()) <= bound and abs(s["fs_im"] - np.sin(phase).mean()) <= bound
    sim.close()


# ---- recorded while stepping -----------------------------------------------------------------------------------------

def stepping_sim(pb, orc, form, wave):
    """tests/test_gpu_series.py's light_wave_sim; wave False: the same blob under a control that is not the light wave
    (no phase updates, no radius wave)."""
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0 if wave else 1, phase_update_interval=PUI)
    sim.set_resident(form["resident"])
    if "lanes" in form:
        sim.set_lanes_per_bot(form["lanes"])
    return sim


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
    vectors = pb.half_plane_vectors(3)
    # a: the scattering alone; b: the twin, everything off; c: all three recorders; d: the time correlation alone;
    # e: the series alone
    a, b, c, d, e = (stepping_sim(pb, orc, form, wave) for _ in range(5))
    assert a.config()["resident"] == (1 if name == "resident" else 0)
    for s in (a, c):
        s.set_scattering(interval, LAGS, BOX, vectors)
    for s in (c, d):
        s.set_time_correlation(interval, LAGS, 0.015625)
    for s in (c, e):
        s.set_series(interval, 512)
    assert a.scattering_info() == {"interval": float(f32(interval)), "lags": LAGS, "box_log2": BOX, "nvec": 24, "records": 0}
    for s in (a, c, d, e):
        assert s.step(steps, dt=DT, sort_interval=SORT) == steps  # one call
    assert a.scattering_info()["records"] == c.scattering_info()["records"] == len(rec)
    got = a.scattering()[0]
    states = twin_states(b, gates, steps)[0]
    want = XR.table([p for p, _ in states], rec, LAGS, vectors, BOX)
    print(name, wave, got[1][0])
    assert got == want, (name, wave)
    assert [g[0]["origins"] for g in got] == [len(rec) - l for l in range(LAGS)]
    assert all(r["samples"] == 300 * r["origins"] for g in got for r in g)
    if interval:  # 25 steps between records: the blob moved, and the longest lag has left the table's step 0
        assert any(r["im"] != 0 for r in got[LAGS - 1]) and all(r["re"] < r["samples"] << 30 for r in got[LAGS - 1][:3])
    lay = layout_of(a)
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(300))  # sorted: the slots are not in original order
    # the final state is the twin's, bit for bit, whichever recorders ran
    sb = b.get_state()
    for s in (a, c, d, e):
        st = s.get_state()
        for k in sb:
            assert_bit_equal(st[k], sb[k], f"{name} {k}")
        assert s.time == b.time
    # each recorder gives what it gives alone
    assert c.scattering()[0] == got
    assert c.time_correlation() == d.time_correlation() and d.time_correlation()[0] == TR.table(states, rec, LAGS, 0.015625)
    assert c.series_of(0) == e.series_of(0) and len(e.series_of(0)) == len(rec)
    # the launches are those of a run with only the time correlation on at that interval
    assert a.stats() == d.stats() == c.stats() == e.stats()
    assert a.stats()["steps"] == steps and a.stats()["resorts"] == len(sorts) and a.stats()["phase_updates"] == len(phases)
    if name == "resident":
        assert a.stats()["resident_launches"] > 0
    if name == "every_step":
        assert a.stats()["fused_launches"] == 0  # interval 0 costs the fusion
    elif name != "resident":
        assert a.stats()["fused_launches"] > 0
    n, ms = a.scattering_times()
    assert n == len(rec) and ms > 0.0
    for s in (a, b, c, d, e):
        s.close()


def test_reading_and_recording_change_nothing(pb, orc):
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, phase_update_interval=0.3)
    vectors = vector_list(3)
    sim.set_series(0.1, 8)
    sim.set_time_correlation(0.1, 3, 0.5)
    sim.set_scattering(-1.0, 3, BOX, vectors)
    assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    assert sim.scattering_info()["records"] == 0  # manual only
    before, stats, lay, t = sim.get_state(), sim.stats(), layout_of(sim), sim.time
    series, corr = sim.series_of(0), sim.time_correlation()
    sim.scattering_record()
    sim.scattering_record()
    first = sim.scattering()
    assert first == sim.scattering()
    assert first[0] == XR.table([before["pos"]] * 2, [60, 60], 3, vectors, BOX)
    after = sim.get_state()
    for k in before:
        assert_bit_equal(before[k], after[k], k)
    assert sim.stats() == stats and sim.time == t and sim.series_of(0) == series and sim.time_correlation() == corr
    for x, y in zip(lay, layout_of(sim)):
        assert np.array_equal(x, y)
    # a later step and a set_state leave the ring alone: the next record pairs with the two it holds
    assert sim.step(7, dt=DT, sort_interval=0.2) == 7
    now = sim.get_state()
    sim.set_state(pos=now["pos"], vel=now["vel"], rad=now["rad"], phase=now["phase"], dead=now["dead"])
    sim.scattering_record()
    assert sim.scattering()[0] == XR.table([before["pos"]] * 2 + [now["pos"]], [60, 60, 67], 3, vectors, BOX)
    assert sim.scattering_times()[0] == 3 and sim.scattering_times()[1] > 0.0
    sim.close()


# ---- life cycle --------------------------------------------------------------------------------------------------------

def test_restart_switch_off_and_argument_errors(pb, orc):
    start = live_memory()
    pos, vel, rad = recipe(300)
    a = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0, phase_update_interval=PUI)
    a.set_resident(1)
    made = live_memory()
    vectors = vector_list(65)
    assert a.scattering_info() == OFF and a.scattering_times() == (0, 0.0)
    for call in (a.scattering_record, a.scattering):
        with pytest.raises(RuntimeError, match="code 2.*the scattering is off"):
            call()
    for bad, word in (((-0.5, 4, 3, vectors), "interval"), ((float("nan"), 4, 3, vectors), "interval"),
                      ((0.0, 65, 3, vectors), "lags"), ((0.0, 4, 13, vectors), "boxLog2"), ((0.0, 4, -9, vectors), "boxLog2"),
                      ((0.0, 4, 3, vector_list(257)), "nvec"), ((0.0, 4, 3, np.zeros((0, 2), np.int32)), "nvec")):
        with pytest.raises(RuntimeError, match="code 2.*pbSimSetScattering.*" + word):
            a.set_scattering(*bad)
    assert a.scattering_info() == OFF and live_memory() == made
    a.set_scattering(0.0, 4, 3, vectors)
    # the ring, the table with its counters, the phasors and the list
    assert live_memory() == (made[0] + 4, made[1] + 4 * 300 * 8 + (4 * 65 * 16 + 4 * 8) + 4096 * 8 + 65 * 8)
    vectors[:] = 0  # the list was copied at the call
    assert a.step(20, dt=DT, sort_interval=SORT) == 20 and a.scattering_info()["records"] == 20
    rows = a.scattering()[0]
    assert [r[0]["origins"] for r in rows] == [20, 19, 18, 17] and [r[64]["sum_steps"] for r in rows] == [0, 19, 36, 51]
    assert [[r["nx"], r["ny"]] for r in rows[0]] == vector_list(65).tolist()
    # again: restarts at record 0 with a zeroed table
    a.set_scattering(0.05, 64, -8, vector_list(3))
    assert a.scattering_info() == {"interval": float(f32(0.05)), "lags": 64, "box_log2": -8, "nvec": 3, "records": 0}
    zero = a.scattering()[0]
    assert len(zero) == 64 and all(len(z) == 3 for z in zero)
    assert all(dict(r, nx=0, ny=0) == dict(dict.fromkeys(XR.FIELDS, 0), lag=l) for l, z in enumerate(zero) for r in z)
    gates = SR.gate_steps(a.time, DT, 0.05, 30, 1e9)
    assert a.step(30, dt=DT, sort_interval=SORT) == 30
    rows = a.scattering()[0]
    assert a.scattering_info()["records"] == len(gates) and 5 <= len(gates) <= 7
    assert [r[0]["origins"] for r in rows] == [max(len(gates) - l, 0) for l in range(64)]
    assert rows[1][2]["sum_steps"] == gates[-1][0] - gates[0][0]
    # lags 0 frees: the memory is back, later steps record nothing and are fused again
    a.set_scattering(0.05, 0, 0, None)
    assert a.scattering_info() == OFF and live_memory() == made
    stats = a.stats()
    assert a.step(30, dt=DT, sort_interval=SORT) == 30 and a.scattering_info() == OFF
    assert a.stats()["fused_launches"] == stats["fused_launches"] + 29  # every step but the call's last is fused again
    with pytest.raises(RuntimeError, match="code 2.*the scattering is off"):
        a.scattering()
    assert a.scattering_times() == (0, 0.0)
    # destroyed with the ring live: nothing stays
    a.set_scattering(-1.0, 2, 3, vector_list(1))
    a.scattering_record()
    assert live_memory()[0] == made[0] + 4
    a.close()
    assert live_memory() == start


# ---- the runner ------------------------------------------------------------------------------------------------------

HEADER = "Lag, Nx, Ny, Origins, SumSteps, Samples, Re, Im, FsRe, FsIm"
COLUMNS = ("lag", "nx", "ny", "origins", "sum_steps", "samples", "re", "im")


def test_runner_writes_the_table_at_the_end_of_the_run(tmp_path):
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import host
    over = dict(max_time="30", dump_interval="2.5")
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--scatter", "f.csv", "--scatter-lags", "4", "--scatter-nmax", "2",
                                                      "--scatter-box-log2", "4"],
                       capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "f.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 4 * 12
    cells = [l.split(", ") for l in lines[1:]]
    assert [int(c[0]) for c in cells] == [l for l in range(4) for _ in range(12)]
    assert [int(c[3]) for c in cells[::12]] == [12, 11, 10, 9] and all(int(c[5]) == 300 * int(c[3]) for c in cells)
    # the same rows from the class driven in-process, with the runner's list
    flat = host.load_config(CFG, **over)
    h = host.HostSim(CFG, engine="fused", **over)
    vectors = pb.half_plane_vectors(2)
    h.set_scattering(flat.dump_interval, 4, 4, vectors)
    assert h.scattering_info() == {"interval": float(f32(flat.dump_interval)), "lags": 4, "box_log2": 4, "nvec": 12,
                                   "records": 0}
    while not h.finished:
        if h.advance(h.steps_until_dump()) == 0:
            break
    want = [w for lag in h.scattering()[0] for w in lag]
    assert [", ".join(c[:8]) for c in cells] == [", ".join(str(w[k]) for k in COLUMNS) for w in want]
    for c, w in zip(cells, want):
        s = pb.scattering_summary(w)
        assert c[8] == "%.9g" % s["fs_re"] and c[9] == "%.9g" % s["fs_im"], (c, s)
    assert h.scattering_info()["records"] == 12
    h.scattering_record()
    assert h.scattering_info()["records"] == 13
    h.close()
    # the defaults: 32 lags, the 24 vectors of the half plane up to 3, the box that holds the walls
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--scatter", "g.csv"], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "g.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 32 * 24
    assert [l.split(", ")[1:3] for l in lines[1:25]] == [[str(x), str(y)] for x, y in pb.half_plane_vectors(3).tolist()]


def test_runner_refuses_a_run_whose_table_cannot_fit(tmp_path):
    # 300 bots, a record every 0.01 s up to 10^5 s: 10^7 records, 3 x 10^9 samples in lag 0
    r = subprocess.run([RUN, CFG, "--quiet", "--set", "max_time", "100000", "--scatter", "f.csv", "--scatter-interval",
                        "0.01"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 2 and r.stdout == ""
    assert r.stderr == ("--scatter: about 10000002 records of 300 bots would pass 2^31 samples per lag: raise "
                        "--scatter-interval or lower max_time\n")
    assert not os.path.exists(tmp_path / "f.csv")
