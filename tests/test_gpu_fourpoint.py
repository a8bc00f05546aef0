"""GPU: the four-point recorder (pbSimSetFourPoint / pbSimFourPointRecord / pbSimGetFourPoint, csrc/pb_fourpoint.hip)
against tests/fourpoint_ref.py on states read back from the device.  Every comparison is exact: a row holds integers
only, overlap2, re, im and power composed from their limbs.  A table recorded while stepping is compared with a twin run
that has the recorder off and is stopped in front of every step the gate names.  tests/test_fourpoint_api.py pins the
reference to a plain double loop and to its identities on the CPU, and shows that the walk used here mixes overlapping
and non-overlapping bots in every wave; tests/test_fourpoint_ref.py holds the limb arithmetic, the third limb of power
included, which no state of a few seconds' size reaches.

Not run here, as in tests/test_gpu_scatter.py: the refusals that need a batch of 2^28 bots, of more than 65535 members,
a ring above 2^33 bytes, a table above 2^31 bytes and a lag with 2^31 origins: none fits a test of a few seconds.  They
are comparisons in front of the allocation in pbSimSetFourPoint and one in front of the read-back in pbSimGetFourPoint."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import coherent_ref as CR
import fourpoint_ref as FR
import series_ref as SR
import sfactor_ref as KR
from helpers import assert_bit_equal
from test_fourpoint_api import RADIUS, dyadic_walk, walk, walk_records
from test_gpu_series import DT, FORMS, INTERVAL, PUI, SORT, STEPS, layout_of, make_batch, sim_with
from test_gpu_sfactor import live_memory
from test_gpu_timecorr import same_bits, twin_states
from test_scatter_api import BOXES, MANUAL_LAGS, MANUAL_RECORDS, NVECS, SIZES, unmeasured_records, vector_list
from test_series_api import CORNER, recipe
from test_timecorr_api import BATCH_BOTS, batch_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
LAGS, BOX, STEP_RADIUS = 5, 3, 0.015625  # while stepping
BELOW = float(np.nextafter(f32(2048.0), f32(0.0)))
OFF = {"interval": 0.0, "lags": 0, "overlap_radius": 0.0, "box_log2": 0, "nvec": 0, "records": 0}


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def header_constant(name):
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    return int(re.search(r"#define %s (\d+)u" % name, header).group(1))


def put(sim, pos):
    n = len(pos)
    zeros = np.zeros((n, 2), f32)
    sim.set_state(pos=pos, vel=zeros, rad=np.full(n, 0.1, f32), phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    return sim.get_state()["pos"]


def record_manually(sim, records, lags, radius, box_log2, vectors, also=None):
    """Sets each of `records` (positions) and takes a record of it (and whatever `also` records of the same state);
    returns the member's rows and the positions read back."""
    sim.set_four_point(-1.0, lags, radius, box_log2, vectors)
    assert sim.four_point_info() == {"interval": -1.0, "lags": lags, "overlap_radius": float(f32(radius)),
                                     "box_log2": box_log2, "nvec": len(vectors), "records": 0}
    back = []
    for pos in records:
        back.append(put(sim, pos))
        sim.four_point_record()
        if also:
            also()
    assert sim.four_point_info()["records"] == len(records)
    return sim.four_point()[0], back


def fresh_sim(pb, orc, n):
    return sim_with(pb, orc, np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.full(n, 0.1, f32))


# ---- manual records on set states ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", ["origin", "corner"])
def test_manual_records_around_the_wave_and_the_workgroup(pb, orc, n, where):
    k = SIZES.index(n) + (len(SIZES) if where == "corner" else 0)
    nvec, box = NVECS[k % len(NVECS)], BOXES[k % len(BOXES)]  # (16 cases: every nvec and every box several times)
    vectors = vector_list(nvec)
    recs = walk_records(n, CORNER if where == "corner" else (0.0, 0.0), records=MANUAL_RECORDS)
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, MANUAL_LAGS, RADIUS, box, vectors)
    for got, want in zip(back, recs):
        assert same_bits(got, want)
    want = FR.table(back, [0] * MANUAL_RECORDS, MANUAL_LAGS, RADIUS, vectors, box)
    print(n, where, nvec, box, rows[1][0])
    assert rows == want, (n, where, nvec, box)
    assert [r[0]["origins"] for r in rows] == [7, 6, 5] and [r[-1]["samples"] for r in rows] == [7 * n, 6 * n, 5 * n]
    assert all(r["sum_steps"] == 0 for lag in rows for r in lag)
    assert rows[0][0]["overlap"] == 7 * n and rows[0][0]["overlap2"] == 7 * n * n  # a bot overlaps itself
    if n >= 63:  # the walk: some bots of every origin stayed, some did not, and their number fluctuates
        o, q, q2 = rows[1][0]["origins"], rows[1][0]["overlap"], rows[1][0]["overlap2"]
        assert 0 < q < rows[1][0]["samples"] and q2 * o - q * q > 0
    sim.close()


@pytest.mark.parametrize("nvec", NVECS)
@pytest.mark.parametrize("box", BOXES)
def test_every_list_length_in_every_box(pb, orc, nvec, box):
    n = 257
    vectors = vector_list(nvec)
    recs = walk_records(n, (1.5, -2.25), records=MANUAL_RECORDS)
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, MANUAL_LAGS, RADIUS, box, vectors)
    want = FR.table(back, [0] * MANUAL_RECORDS, MANUAL_LAGS, RADIUS, vectors, box)
    assert rows == want, (nvec, box)
    assert [[r["nx"], r["ny"]] for r in rows[2]] == vectors.tolist()
    assert all(r["samples"] == (7 - l) * n for l in range(3) for r in rows[l])
    if nvec >= 3:
        assert rows[1][0] == rows[1][2] and rows[1][0]["im"] != 0  # the repeated vector
    if nvec >= 4:  # (0, 0) counts the overlapping bots
        assert all(r[3]["re"] == r[3]["overlap"] << 30 and r[3]["im"] == 0 and r[3]["power"] == r[3]["overlap2"] << 60
                   for r in rows)
    sim.close()


def test_the_dyadic_walk_with_its_exact_ties_and_the_time_correlations_overlap(pb, orc):
    recs = dyadic_walk()
    vectors = vector_list(3)
    sim = fresh_sim(pb, orc, 257)
    sim.set_time_correlation(-1.0, MANUAL_LAGS, RADIUS)
    rows, back = record_manually(sim, recs, MANUAL_LAGS, RADIUS, 3, vectors, also=sim.time_correlation_record)
    for got, want in zip(back, recs):
        assert same_bits(got, want)
    assert rows == FR.table(back, [0] * 7, MANUAL_LAGS, RADIUS, vectors, 3)
    # the fp32 differences are exact on this grid: the time correlation, which quantises the difference, counts the same
    corr = sim.time_correlation()[0]
    assert [r[0]["overlap"] for r in rows] == [c["overlap"] for c in corr]
    assert [r[0]["samples"] for r in rows] == [c["samples"] for c in corr] == [7 * 257, 6 * 257, 5 * 257]
    # the ties (tests/test_fourpoint_api.py counts them: 6 at lag 1, 2 at lag 2) do not overlap; a quantum more and they do
    more, _ = record_manually(sim, recs, MANUAL_LAGS, RADIUS + 2.0 ** -20, 3, vectors)
    assert more == FR.table(back, [0] * 7, MANUAL_LAGS, RADIUS + 2.0 ** -20, vectors, 3)
    assert [m[0]["overlap"] - r[0]["overlap"] for r, m in zip(rows, more)] == [0, 6, 2]
    sim.close()


def test_more_bots_than_one_pass_covers(pb, orc):
    n = header_constant("PB_FOURPOINT_BLOCKS") * 256 + 321  # the block loop runs twice for 321 lanes
    assert n == 65857
    recs = walk(recipe(n, (-300.0, 700.0))[0], 7000 + n, 3)
    vectors = vector_list(3)
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, 2, RADIUS, 3, vectors)
    assert rows == FR.table(back, [0] * 3, 2, RADIUS, vectors, 3)
    assert [r[0]["samples"] for r in rows] == [3 * n, 2 * n] and 0 < rows[1][0]["overlap"] < 2 * n
    sim.close()


def test_unmeasured_records(pb, orc):
    recs, bad = unmeasured_records()
    vectors = vector_list(3)
    sim = fresh_sim(pb, orc, 257)
    rows, back = record_manually(sim, recs, 3, 1.0, 3, vectors)
    for got, want in zip(back, recs):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])
    assert rows == FR.table(back, [0, 0, 0], 3, 1.0, vectors, 3)
    # a bot of every unmeasured kind is missing from exactly the pairs that hold its record
    samples = [sum(257 - len(set(bad[r]) | set(bad[r - l])) for r in range(l, 3)) for l in range(3)]
    assert [r[0]["samples"] for r in rows] == samples == [3 * 245, 2 * 233, 233]
    # against a radius of 1: records 0 -> 1 shift by 0.56 and 0 -> 2 by 0.76 (all overlap but the two bots that stood
    # just inside the range in one of the records), records 1 -> 2 by 1.3 (none does)
    assert [r[0]["overlap"] for r in rows] == [samples[0], 233 - 2, 233 - 2]
    sim.close()
    # no measured bot: an all-zero table with the right origins
    far = np.full((65, 2), 3000.0, f32)
    far[::2, 1] = np.inf
    sim = fresh_sim(pb, orc, 65)
    rows, _ = record_manually(sim, [far, far], 2, 1.0, 3, vectors)
    zero = dict.fromkeys(FR.FIELDS, 0)
    assert rows == [[dict(zero, lag=l, nx=int(nx), ny=int(ny), origins=2 - l) for nx, ny in vectors] for l in range(2)]
    sim.close()


def test_radius_zero_and_the_largest_radius(pb, orc):
    n = 257
    recs = walk_records(n, (1.5, -2.25), records=4)
    vectors = vector_list(65)
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, 3, 0.0, 4, vectors)  # nothing overlaps, lag 0 included; samples are counted
    assert rows == FR.table(back, [0] * 4, 3, 0.0, vectors, 4)
    for l, lag in enumerate(rows):
        assert all((r["samples"], r["overlap"], r["overlap2"], r["re"], r["im"], r["power"]) == ((4 - l) * n, 0, 0, 0, 0, 0)
                   for r in lag)
    # everything measured overlaps: the mode of an origin is the density mode of its earlier state
    sk = []
    for pos in recs:
        put(sim, pos)
        rows_sk = KR.from_device(sim.structure_factor(vectors, 4, "density")[0])
        sk.append([(r["re"], r["im"]) for r in rows_sk])
        assert {r["measured"] for r in rows_sk} == {n}
    rows, back = record_manually(sim, recs, 3, BELOW, 4, vectors)
    assert rows == FR.table(back, [0] * 4, 3, BELOW, vectors, 4)
    for l, lag in enumerate(rows):
        then = range(0, 4 - l)  # the earlier records of lag l's origins
        for k, r in enumerate(lag):
            assert (r["re"], r["im"]) == tuple(sum(sk[t][k][c] for t in then) for c in (0, 1))
            assert r["power"] == sum(sk[t][k][0] ** 2 + sk[t][k][1] ** 2 for t in then)
            assert r["samples"] == r["overlap"] == (4 - l) * n and r["overlap2"] == (4 - l) * n * n
    # lag 0's power is the coherent recorder's lag-0 re for the same list and box
    sim.set_coherent_scattering(-1.0, 3, 4, vectors)
    for pos in recs:
        put(sim, pos)
        sim.coherent_scattering_record()
    coh = sim.coherent_scattering()[0]
    assert [r["power"] for r in rows[0]] == [c["re"] for c in coh[0]]
    # with an unmeasured bot in one record, lag 0 still agrees, and at the default radius too
    recs[2][9, 0] = np.nan
    sim.set_coherent_scattering(-1.0, 3, 4, vectors)
    rows, back = record_manually(sim, recs, 3, RADIUS, 4, vectors, also=sim.coherent_scattering_record)
    assert rows == FR.table(back, [0] * 4, 3, RADIUS, vectors, 4)
    assert [r["power"] for r in rows[0]] == [c["re"] for c in sim.coherent_scattering()[0][0]]
    assert rows[0][0]["samples"] == 4 * n - 1
    sim.close()


def test_batch_of_three_members_each_equals_a_lone_sim(pb, orc):
    n, starts = BATCH_BOTS, [member[0][0] for member in batch_records()]
    # different motion per member: member k walks from the batch's first record with steps k + 1 times as long
    steps = [walk(np.zeros((n, 2), f32), 7100 + k, 4) for k in range(3)]
    recs = [[(starts[k] + steps[k][r] * f32(k + 1)).astype(f32) for r in range(4)] for k in range(3)]
    vectors = vector_list(65)
    ens = make_batch(pb, orc, 3, n)
    ens.set_four_point(-1.0, 3, RADIUS, 4, vectors)
    back = [[] for _ in range(3)]
    for r in range(4):
        for k in range(3):
            ens.set_state_of(k, pos=recs[k][r])
            st = ens.get_state_of(k)
            assert same_bits(st["pos"], recs[k][r])
            back[k].append(st["pos"])
        ens.four_point_record()
    rows = ens.four_point()
    assert len(rows) == 3 and all(len(r) == 3 and len(r[0]) == 65 for r in rows)
    lone = fresh_sim(pb, orc, n)
    for k in range(3):
        assert rows[k] == FR.table(back[k], [0] * 4, 3, RADIUS, vectors, 4), k
        alone, _ = record_manually(lone, recs[k], 3, RADIUS, 4, vectors)
        assert alone == rows[k], k
        assert [r[0]["samples"] for r in rows[k]] == [4 * n, 3 * n, 2 * n]
    assert rows[0][1][0]["overlap"] > rows[1][1][0]["overlap"] > rows[2][1][0]["overlap"]  # the faster member overlaps less
    assert ens.four_point() == rows  # twice: the same rows
    lone.close()
    ens.close()


# ---- recorded while stepping -----------------------------------------------------------------------------------------

WIDTH, BINS = 0.03125, 16


def stepping_sim(pb, orc, form, wave):
    """tests/test_gpu_series.py's light_wave_sim with a centroid trail to switch on; wave False: the same blob under a
    control that is not the light wave (no phase updates, no radius wave)."""
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0 if wave else 1, phase_update_interval=PUI,
                   centroid_steps=16, centroid_int=0.1)
    sim.set_resident(form["resident"])
    if "lanes" in form:
        sim.set_lanes_per_bot(form["lanes"])
    return sim


@pytest.mark.parametrize("wave", [True, False], ids=["wave", "no_wave"])
@pytest.mark.parametrize("name", list(FORMS))
def test_recorded_table_equals_a_twin_and_leaves_the_run_alone(pb, orc, name, wave):
    form = FORMS[name]
    interval, steps = (0.0, 120) if name == "every_step" else (INTERVAL, STEPS)
    gates = SR.gate_steps(0.0, DT, interval, steps, 1e9)
    rec = [k for k, _ in gates]
    sorts = [k for k, _ in SR.gate_steps(0.0, DT, SORT, steps, 1e9)]
    phases = [k for k, _ in SR.gate_steps(0.0, DT, PUI, steps, 1e9)] if wave else []
    assert len(rec) > LAGS  # the ring wraps
    vectors = np.concatenate([pb.half_plane_vectors(3), np.zeros((1, 2), np.int32)])
    # a: the recorder alone; b: the twin, everything off; d: the time correlation alone, whose launches' count it shares
    a, b, d = (stepping_sim(pb, orc, form, wave) for _ in range(3))
    assert a.config()["resident"] == (1 if name == "resident" else 0)
    a.set_four_point(interval, LAGS, STEP_RADIUS, BOX, vectors)
    d.set_time_correlation(interval, LAGS, STEP_RADIUS)
    assert a.four_point_info() == {"interval": float(f32(interval)), "lags": LAGS, "overlap_radius": STEP_RADIUS,
                                   "box_log2": BOX, "nvec": 25, "records": 0}
    for s in (a, d):
        assert s.step(steps, dt=DT, sort_interval=SORT) == steps  # one call
    assert a.four_point_info()["records"] == len(rec)
    got = a.four_point()[0]
    states = twin_states(b, gates, steps)[0]
    want = FR.table([p for p, _ in states], rec, LAGS, STEP_RADIUS, vectors, BOX)
    print(name, wave, got[1][0], got[LAGS - 1][24])
    assert got == want, (name, wave)
    assert [g[0]["origins"] for g in got] == [len(rec) - l for l in range(LAGS)]
    assert all(r["samples"] == 300 * r["origins"] for g in got for r in g)
    assert all(r["overlap"] == r["samples"] for r in got[0])
    lay = layout_of(a)
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(300))  # sorted: the slots are not in original order
    # the final state is the twin's, bit for bit
    sb = b.get_state()
    for s in (a, d):
        st = s.get_state()
        for k in sb:
            assert_bit_equal(st[k], sb[k], f"{name} {k}")
        assert s.time == b.time
    # the launches are those of a run with only the time correlation on at that interval
    assert a.stats() == d.stats()
    assert a.stats()["steps"] == steps and a.stats()["resorts"] == len(sorts) and a.stats()["phase_updates"] == len(phases)
    if name == "resident":
        assert a.stats()["resident_launches"] > 0
    if name == "every_step":
        assert a.stats()["fused_launches"] == 0  # interval 0 costs the fusion
    elif name != "resident":
        assert a.stats()["fused_launches"] > 0
    n, ms = a.four_point_times()
    assert n == len(rec) and ms > 0.0
    for s in (a, b, d):
        s.close()


def test_all_seven_recorders_at_once_each_gives_what_it_gives_alone(pb, orc):
    form, steps = FORMS["fused"], STEPS
    vectors = pb.half_plane_vectors(3)
    switches = {
        "series": lambda s: s.set_series(INTERVAL, 512),
        "time_correlation": lambda s: s.set_time_correlation(INTERVAL, LAGS, STEP_RADIUS),
        "scattering": lambda s: s.set_scattering(INTERVAL, LAGS, BOX, vectors),
        "van_hove": lambda s: s.set_van_hove(INTERVAL, LAGS, WIDTH, BINS),
        "van_hove_distinct": lambda s: s.set_van_hove_distinct(INTERVAL, LAGS, WIDTH, BINS),
        "coherent_scattering": lambda s: s.set_coherent_scattering(INTERVAL, LAGS, BOX, vectors),
        "four_point": lambda s: s.set_four_point(INTERVAL, LAGS, STEP_RADIUS, BOX, vectors),
    }
    read = lambda s, name: s.series_of(0) if name == "series" else getattr(s, name)()
    every = stepping_sim(pb, orc, form, True)
    every.set_centroid_trail(True)
    for on in switches.values():
        on(every)
    assert every.step(steps, dt=DT, sort_interval=SORT) == steps
    final = every.get_state()
    for name, on in switches.items():
        alone = stepping_sim(pb, orc, form, True)
        on(alone)
        assert alone.step(steps, dt=DT, sort_interval=SORT) == steps
        assert read(alone, name) == read(every, name), name
        st = alone.get_state()
        for k in final:
            assert_bit_equal(st[k], final[k], f"{name} {k}")
        alone.close()
    assert every.four_point_info()["records"] == every.coherent_scattering_info()["records"] == len(every.series_of(0))
    every.close()
    # the order in which stepMany fires them is the header's sentence
    header = re.sub(r"\s*\n \* ", " ", open(os.path.join(ROOT, "include", "particlebot_hip.h")).read())
    assert ("the order is: series, time correlation, scattering, van Hove, distinct van Hove, coherent scattering, "
            "four-point; then the centroid trail and the phase update") in header
    engine = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_engine.hip")).read()
    body = engine.split("PbHostEvent events[")[1]
    fired = [body.index(word) for word in ("pbSeriesRecord}", "pbTimeCorrRecord(B)", "pbScatteringRecord(B)",
                                           "pbVanHoveRecord(B)", "pbVanHoveDistinctRecord(B)", "pbCoherentRecord(B)",
                                           "pbFourPointRecord(B)", "trailRecord}", "phaseUpdate(B)")]
    assert fired == sorted(fired)


def test_reading_and_recording_change_nothing(pb, orc):
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, phase_update_interval=0.3)
    vectors = vector_list(3)
    sim.set_series(0.1, 8)
    sim.set_time_correlation(0.1, 3, 0.5)
    sim.set_scattering(0.1, 3, BOX, vectors)
    sim.set_four_point(-1.0, 3, 0.5, BOX, vectors)
    assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    assert sim.four_point_info()["records"] == 0  # manual only
    before, stats, lay, t = sim.get_state(), sim.stats(), layout_of(sim), sim.time
    series, corr, scat = sim.series_of(0), sim.time_correlation(), sim.scattering()
    sim.four_point_record()
    sim.four_point_record()
    first = sim.four_point()
    assert first == sim.four_point()
    assert first[0] == FR.table([before["pos"]] * 2, [60, 60], 3, 0.5, vectors, BOX)
    after = sim.get_state()
    for k in before:
        assert_bit_equal(before[k], after[k], k)
    assert sim.stats() == stats and sim.time == t and sim.series_of(0) == series and sim.time_correlation() == corr
    assert sim.scattering() == scat
    for x, y in zip(lay, layout_of(sim)):
        assert np.array_equal(x, y)
    # a later step and a set_state leave the ring alone: the next record pairs with the two it holds
    assert sim.step(7, dt=DT, sort_interval=0.2) == 7
    now = sim.get_state()
    sim.set_state(pos=now["pos"], vel=now["vel"], rad=now["rad"], phase=now["phase"], dead=now["dead"])
    sim.four_point_record()
    assert sim.four_point()[0] == FR.table([before["pos"]] * 2 + [now["pos"]], [60, 60, 67], 3, 0.5, vectors, BOX)
    assert sim.four_point_times()[0] == 3 and sim.four_point_times()[1] > 0.0
    sim.close()


# ---- life cycle --------------------------------------------------------------------------------------------------------

def test_restart_switch_off_and_argument_errors(pb, orc):
    start = live_memory()
    pos, vel, rad = recipe(300)
    a = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0, phase_update_interval=PUI)
    a.set_resident(1)
    made = live_memory()
    vectors = vector_list(65)
    assert a.four_point_info() == OFF and a.four_point_times() == (0, 0.0)
    for call in (a.four_point_record, a.four_point):
        with pytest.raises(RuntimeError, match="code 2.*the four-point recorder is off"):
            call()
    for bad, word in (((-0.5, 4, 0.5, 3, vectors), "interval"), ((float("nan"), 4, 0.5, 3, vectors), "interval"),
                      ((0.0, 65, 0.5, 3, vectors), "lags"), ((0.0, 4, -0.5, 3, vectors), "overlapRadius"),
                      ((0.0, 4, 2048.0, 3, vectors), "overlapRadius"), ((0.0, 4, float("nan"), 3, vectors), "overlapRadius"),
                      ((0.0, 4, 0.5, 13, vectors), "boxLog2"), ((0.0, 4, 0.5, -9, vectors), "boxLog2"),
                      ((0.0, 4, 0.5, 3, vector_list(257)), "nvec"), ((0.0, 4, 0.5, 3, np.zeros((0, 2), np.int32)), "nvec")):
        with pytest.raises(RuntimeError, match="code 2.*pbSimSetFourPoint.*" + word):
            a.set_four_point(*bad)
    assert a.four_point_info() == OFF and live_memory() == made
    a.set_four_point(0.0, 4, 0.5, 3, vectors)
    # the ring of positions, the cells with the (member, lag) words, the record's scratch, the phasors and the list
    assert live_memory() == (made[0] + 5, made[1] + 4 * 300 * 8 + 4 * (65 * 64 + 32) + 4 * (65 * 16 + 16) + 4096 * 8 + 65 * 8)
    vectors[:] = 0  # the list was copied at the call
    assert a.step(20, dt=DT, sort_interval=SORT) == 20 and a.four_point_info()["records"] == 20
    rows = a.four_point()[0]
    assert [r[0]["origins"] for r in rows] == [20, 19, 18, 17] and [r[64]["sum_steps"] for r in rows] == [0, 19, 36, 51]
    assert [[r["nx"], r["ny"]] for r in rows[0]] == vector_list(65).tolist()
    # again: restarts at record 0 with a zeroed table
    a.set_four_point(0.05, 64, 0.25, -8, vector_list(3))
    assert a.four_point_info() == {"interval": float(f32(0.05)), "lags": 64, "overlap_radius": 0.25, "box_log2": -8,
                                   "nvec": 3, "records": 0}
    zero = a.four_point()[0]
    assert len(zero) == 64 and all(len(z) == 3 for z in zero)
    assert all(dict(r, nx=0, ny=0) == dict(dict.fromkeys(FR.FIELDS, 0), lag=l) for l, z in enumerate(zero) for r in z)
    gates = SR.gate_steps(a.time, DT, 0.05, 30, 1e9)
    assert a.step(30, dt=DT, sort_interval=SORT) == 30
    rows = a.four_point()[0]
    assert a.four_point_info()["records"] == len(gates) and 5 <= len(gates) <= 7
    assert [r[0]["origins"] for r in rows] == [max(len(gates) - l, 0) for l in range(64)]
    assert rows[1][2]["sum_steps"] == gates[-1][0] - gates[0][0]
    # lags 0 frees: the memory is back, later steps record nothing and are fused again
    a.set_four_point(0.05, 0, 0.0, 0, None)
    assert a.four_point_info() == OFF and live_memory() == made
    stats = a.stats()
    assert a.step(30, dt=DT, sort_interval=SORT) == 30 and a.four_point_info() == OFF
    assert a.stats()["fused_launches"] == stats["fused_launches"] + 29  # every step but the call's last is fused again
    with pytest.raises(RuntimeError, match="code 2.*the four-point recorder is off"):
        a.four_point()
    with pytest.raises(RuntimeError, match="code 2.*the four-point recorder is off"):
        a.four_point_record()
    assert a.four_point_times() == (0, 0.0)
    # destroyed with the ring live: nothing stays
    a.set_four_point(-1.0, 2, 0.25, 3, vector_list(1))
    a.four_point_record()
    assert live_memory()[0] == made[0] + 5
    a.close()
    assert live_memory() == start


def test_legacy_engine_refuses(capfd):
    from particlerobotsimulations_amd import host
    h = host.HostSim(CFG, engine="legacy")
    capfd.readouterr()
    lib, vec = host.lib(), (C.c_int * 2)(1, 0)
    assert lib.pbHostSetFourPoint(h._h, -1.0, 2, 0.25, 3, vec, 1) == -1
    assert capfd.readouterr() == ("", "Particlebot::setFourPoint: the four-point recorder needs the fused engine\n")
    assert lib.pbHostFourPointRecord(h._h) == -1
    assert capfd.readouterr() == ("", "Particlebot::fourPointRecord: the four-point recorder needs the fused engine\n")
    h.close()


# ---- the runner ------------------------------------------------------------------------------------------------------

HEADER = "Lag, Nx, Ny, Origins, SumSteps, Samples, Overlap, Overlap2, Re, Im, Power, Chi4, S4"
COLUMNS = ("lag", "nx", "ny", "origins", "sum_steps", "samples", "overlap", "overlap2", "re", "im", "power")


def test_runner_writes_the_table_at_the_end_of_the_run(tmp_path):
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import _analysis, _capi, host
    over = dict(max_time="30", dump_interval="2.5")
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--fourpoint", "f.csv", "--fourpoint-lags", "4", "--fourpoint-nmax",
                                                      "2", "--fourpoint-box-log2", "4", "--fourpoint-overlap", "0.05"],
                       capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "f.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 4 * 13
    cells = [l.split(", ") for l in lines[1:]]
    assert [int(c[0]) for c in cells] == [l for l in range(4) for _ in range(13)]
    assert [int(c[3]) for c in cells[::13]] == [12, 11, 10, 9] and all(int(c[5]) == 300 * int(c[3]) for c in cells)
    assert [c[1:3] for c in cells[12::13]] == [["0", "0"]] * 4  # (0, 0) is the list's last
    # the same rows from the class driven in-process through the host library's wrappers, with the runner's list
    flat = host.load_config(CFG, **over)
    h = host.HostSim(CFG, engine="fused", **over)
    lib = host.lib()
    vectors = np.ascontiguousarray(np.concatenate([pb.half_plane_vectors(2), np.zeros((1, 2), np.int32)]), np.int32)
    assert lib.pbHostSetFourPoint(h._h, flat.dump_interval, 4, 0.05, 4, _capi.np_ptr(vectors), len(vectors)) == 0

    def info():
        return _analysis.read_info(_analysis.FOUR_POINT_INFO, lambda *q: lib.pbHostFourPointInfo(h._h, *q))
    assert info() == {"interval": float(f32(flat.dump_interval)), "lags": 4, "overlap_radius": float(f32(0.05)),
                      "box_log2": 4, "nvec": 13, "records": 0}
    while not h.finished:
        if h.advance(h.steps_until_dump()) == 0:
            break
    rows, count = (_capi.pbFourPointRow * 52)(), C.c_ulonglong(0)
    assert lib.pbHostFourPointRows(h._h, rows, 51, C.byref(count)) == -1 and count.value == 52  # too little room
    assert lib.pbHostFourPointRows(h._h, rows, 52, C.byref(count)) == 0 and count.value == 52
    want = [_capi.four_point_row(r) for r in rows]
    assert [", ".join(c[:11]) for c in cells] == [", ".join(str(w[k]) for k in COLUMNS) for w in want]
    for lag in range(4):
        s = pb.four_point_summary(want[13 * lag:13 * lag + 13])
        for c, s4 in zip(cells[13 * lag:13 * lag + 13], s["s4"]):
            assert c[11] == "%.9g" % s["chi4"], (c, s)
            assert float(c[12]) == pytest.approx(s4, rel=1e-6, abs=1e-9), (c, s4)  # (long double against an exact fraction)
    assert info()["records"] == 12
    assert lib.pbHostFourPointRecord(h._h) == 0 and info()["records"] == 13
    assert lib.pbHostSetFourPoint(h._h, 0.0, 0, 0.0, 0, None, 0) == 0 and info()["lags"] == 0  # off
    assert lib.pbHostFourPointRecord(h._h) == -1
    h.close()
    # the defaults: 32 lags, the 24 vectors of the half plane up to 3 and (0, 0), the box that holds the walls
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--fourpoint", "g.csv"], capture_output=True, text=True,
                       timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "g.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 32 * 25
    assert [l.split(", ")[1:3] for l in lines[1:26]] == [[str(x), str(y)] for x, y in pb.half_plane_vectors(3).tolist()] + [["0", "0"]]


def test_runner_refuses_a_run_whose_records_cannot_fit(tmp_path):
    # the one cap is 2^31 origins per lag, whatever the bots: a record every 0.01 s up to 10^8 s is 10^10 records
    r = subprocess.run([RUN, CFG, "--quiet", "--set", "max_time", "100000000", "--fourpoint", "f.csv",
                        "--fourpoint-interval", "0.01"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    records = float(f32(1.0e8)) / float(f32(0.01)) + 2.0
    assert records >= 2.0 ** 31
    assert (r.returncode, r.stdout) == (2, "")
    assert r.stderr == ("--fourpoint: about %.0f records would pass 2^31 origins per lag: raise --fourpoint-interval or "
                        "lower max_time\n" % records)
    assert not os.path.exists(tmp_path / "f.csv")
