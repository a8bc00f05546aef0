"""GPU: the coherent intermediate scattering function (pbSimSetCoherent / pbSimCoherentRecord / pbSimGetCoherent,
csrc/pb_coherent.hip) against tests/coherent_ref.py on states read back from the device.  Every comparison is exact: a
row holds integers only, re and im composed from their 192 bits.  A table recorded while stepping is compared with a twin
run that has the recorder off and is stopped in front of every step the gate names.  tests/test_coherent_api.py pins the
reference to a plain double loop and to known answers on the CPU; tests/test_coherent_ref.py holds the 192-bit
arithmetic, the positive third limb included, which no state of a few seconds' size reaches.

Not run here, as in tests/test_gpu_scatter.py: the refusals that need a batch of 2^28 bots, of more than 65535 members,
a ring plus table above 2^31 bytes (more than 2048 members at 64 lags and 256 vectors), and a lag with 2^31 origins: none
fits a test of a few seconds.  They are comparisons in front of the allocation in pbSimSetCoherent and one in front of
the read-back in pbSimGetCoherent.

The wide batches compare every member with a lone Sim given that member's states: one lone Sim per shape, restarted for
every member, since the recorder reads positions alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import coherent_ref as CR
import series_ref as SR
import sfactor_ref as KR
import timecorr_ref as TR
import wide_batch_cases as W
from helpers import assert_bit_equal, simparams_from_orc
from test_coherent_api import UNIT, float64_products, product_bound
from test_gpu_series import DT, FORMS, INTERVAL, PUI, SORT, STEPS, layout_of, make_batch, sim_with
from test_gpu_sfactor import live_memory
from test_gpu_timecorr import same_bits, twin_states
from test_scatter_api import (BATCH_LAGS, BOXES, L, L_LOG2, MANUAL_LAGS, MANUAL_RECORDS, NVECS, SIZES, dyadic_positions,
                              float64_records, positions, unmeasured_records, vector_list)
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


def put(sim, pos):
    n = len(pos)
    zeros = np.zeros((n, 2), f32)
    sim.set_state(pos=pos, vel=zeros, rad=np.full(n, 0.1, f32), phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    return sim.get_state()["pos"]


def record_manually(sim, records, lags, box_log2, vectors):
    """Sets each of `records` (positions) and takes a record of it; returns the member's rows and the positions read
    back."""
    sim.set_coherent_scattering(-1.0, lags, box_log2, vectors)
    assert sim.coherent_scattering_info() == {"interval": -1.0, "lags": lags, "box_log2": box_log2,
                                              "nvec": len(vectors), "records": 0}
    back = []
    for pos in records:
        back.append(put(sim, pos))
        sim.coherent_scattering_record()
    assert sim.coherent_scattering_info()["records"] == len(records)
    return sim.coherent_scattering()[0], back


def fresh_sim(pb, orc, n):
    return sim_with(pb, orc, np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.full(n, 0.1, f32))


def lag_zero_identities(rows, back, vectors, box):
    """Lag 0 has no imaginary part and holds the summed squares of the records' modes."""
    modes = [CR.modes(p, vectors, box) for p in back]
    for k, row in enumerate(rows[0]):
        assert row["im"] == 0 and row["re"] == sum(m[1][k][0] ** 2 + m[1][k][1] ** 2 for m in modes), k
        assert row["bots_now"] == row["bots_then"] == sum(m[0] for m in modes)


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
    for got, want in zip(back, recs):
        assert same_bits(got, want)
    want = CR.table(back, [0] * MANUAL_RECORDS, MANUAL_LAGS, vectors, box)
    print(n, where, nvec, box, rows[1][0])
    assert rows == want, (n, where, nvec, box)
    assert [r[0]["origins"] for r in rows] == [7, 6, 5] and [r[-1]["bots_then"] for r in rows] == [7 * n, 6 * n, 5 * n]
    assert all(r["sum_steps"] == 0 for lag in rows for r in lag)
    lag_zero_identities(rows, back, vectors, box)
    sim.close()


@pytest.mark.parametrize("nvec", NVECS)
@pytest.mark.parametrize("box", BOXES)
def test_every_list_length_in_every_box(pb, orc, nvec, box):
    n = 257
    vectors = vector_list(nvec)
    recs = positions(manual_records(n, (1.5, -2.25), records=MANUAL_RECORDS))
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, MANUAL_LAGS, box, vectors)
    want = CR.table(back, [0] * MANUAL_RECORDS, MANUAL_LAGS, vectors, box)
    assert rows == want, (nvec, box)
    assert [[r["nx"], r["ny"]] for r in rows[2]] == vectors.tolist()
    assert all(r["bots_now"] == r["bots_then"] == (7 - l) * n for l in range(3) for r in rows[l])
    lag_zero_identities(rows, back, vectors, box)
    if nvec >= 3:
        assert rows[1][0] == rows[1][2] and rows[1][0]["im"] != 0  # the repeated vector; a lag that moved
    sim.close()


def test_more_bots_than_one_pass_covers(pb, orc):
    n = header_constant("PB_COHERENT_BLOCKS") * 256 + 321  # the block loop runs twice for 321 lanes
    assert n == 65857
    recs = positions(manual_records(n, (-300.0, 700.0), records=3))
    vectors = vector_list(3)
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, 2, 3, vectors)
    assert rows == CR.table(back, [0] * 3, 2, vectors, 3)
    assert [r[0]["bots_then"] for r in rows] == [3 * n, 2 * n]
    lag_zero_identities(rows, back, vectors, 3)
    sim.close()


def test_known_answers_on_dyadic_positions(pb, orc):
    n = 70
    point = np.zeros((n, 2), f32)
    moved = (point + np.array([L / 4, 0.0], f32)).astype(f32)
    sim = fresh_sim(pb, orc, n)
    vectors = np.array([(1, 0), (0, 1), (4, 9), (2, 0)], np.int32)
    rows, back = record_manually(sim, [point, point], 2, L_LOG2, vectors)  # all n bots on one point
    assert same_bits(back[0], point)
    for row in rows[0] + rows[1]:
        assert row["re"] == row["origins"] * n * n * UNIT and row["im"] == 0 and row["bots_then"] == row["origins"] * n
    rows, back = record_manually(sim, [point, moved], 2, L_LOG2, vectors)  # then moved a quarter box along x
    assert same_bits(back[1], moved)
    assert [(r["re"], r["im"]) for r in rows[1]] == [(0, n * n * UNIT), (n * n * UNIT, 0), (n * n * UNIT, 0),
                                                     (-n * n * UNIT, 0)]
    assert all(r["re"] == 2 * n * n * UNIT and r["im"] == 0 for r in rows[0])
    # a rigid quarter-box shift of a blob: F(lag 1) = i S(k)
    pos = dyadic_positions()
    rows, back = record_manually(sim, [pos, (pos + np.array([L / 4, 0.0], f32)).astype(f32)], 2, L_LOG2, vectors[:1])
    (_, [(c, s)]) = CR.modes(pos, [(1, 0)], L_LOG2)
    assert rows[1][0]["re"] == 0 and rows[1][0]["im"] == c * c + s * s > 0
    sim.close()


def test_unmeasured_records(pb, orc):
    recs, bad = unmeasured_records()
    vectors = vector_list(3)
    sim = fresh_sim(pb, orc, 257)
    rows, back = record_manually(sim, recs, 3, 3, vectors)
    for got, want in zip(back, recs):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])
    assert rows == CR.table(back, [0, 0, 0], 3, vectors, 3)
    m = [257 - len(b) for b in bad]
    assert [r[0]["bots_now"] for r in rows] == [sum(m), m[1] + m[2], m[2]] == [3 * 245, 2 * 245, 245]
    assert [r[0]["bots_then"] for r in rows] == [sum(m), m[0] + m[1], m[0]]
    # a record with fewer measured bots than the others shows in bots_now and bots_then apart
    fewer = recs[1].copy()
    fewer[200:, 0] = np.inf
    rows, back = record_manually(sim, [recs[0], fewer], 2, 3, vectors)
    assert rows == CR.table(back, [0, 0], 2, vectors, 3)
    assert (rows[1][0]["bots_now"], rows[1][0]["bots_then"]) == (245 - 57, 245)
    sim.close()
    # no measured bot: an all-zero table with the right origins
    far = np.full((65, 2), 3000.0, f32)
    far[::2, 1] = np.inf
    sim = fresh_sim(pb, orc, 65)
    rows, _ = record_manually(sim, [far, far], 2, 3, vectors)
    zero = dict.fromkeys(CR.FIELDS, 0)
    assert rows == [[dict(zero, lag=l, nx=int(nx), ny=int(ny), origins=2 - l) for nx, ny in vectors] for l in range(2)]
    sim.close()


def test_batch_of_three_members_do_not_leak_into_each_other(pb, orc):
    n, recs = BATCH_BOTS, batch_records()
    vectors = vector_list(65)
    ens = make_batch(pb, orc, 3, n)
    ens.set_coherent_scattering(-1.0, BATCH_LAGS, 4, vectors)
    back = [[] for _ in range(3)]
    for r in range(4):
        for k in range(3):
            pos, vel, rad = recs[k][r]
            ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
            st = ens.get_state_of(k)
            assert same_bits(st["pos"], pos)
            back[k].append(st["pos"])
        ens.coherent_scattering_record()
    rows = ens.coherent_scattering()
    assert len(rows) == 3 and all(len(r) == BATCH_LAGS and len(r[0]) == 65 for r in rows)
    for k in range(3):
        assert rows[k] == CR.table(back[k], [0] * 4, BATCH_LAGS, vectors, 4), k
        assert [r[0]["bots_then"] for r in rows[k]] == [4 * n, 3 * n, 2 * n]
    assert rows[0][1] != rows[1][1] != rows[2][1]
    assert ens.coherent_scattering() == rows  # twice: the same rows
    ens.close()


def test_device_against_device_modes_of_the_structure_factor(pb, orc):
    recs, _ = unmeasured_records()
    recs = recs + positions(manual_records(257, (1.5, -2.25), records=2))
    vectors = vector_list(65)
    sim = fresh_sim(pb, orc, 257)
    modes = []
    for pos in recs:  # each record alone: its modes through the structure factor, their square through lag 0
        put(sim, pos)
        sk = KR.from_device(sim.structure_factor(vectors, 4, "density")[0])
        modes.append((sk[0]["measured"], [(r["re"], r["im"]) for r in sk]))
        sim.set_coherent_scattering(-1.0, 1, 4, vectors)
        sim.coherent_scattering_record()
        for row, (c, s) in zip(sim.coherent_scattering()[0][0], modes[-1][1]):
            assert (row["re"], row["im"], row["bots_now"], row["bots_then"]) == (c * c + s * s, 0, modes[-1][0], modes[-1][0])
    rows, _ = record_manually(sim, recs, 3, 4, vectors)
    assert rows == CR.table_of_modes(modes, [0] * len(recs), 3, vectors)  # multiplied in Python
    assert {m[0] for m in modes} == {245, 257}
    sim.close()


def test_against_float64_within_the_derived_bound(pb, orc):
    recs = float64_records()
    vectors = pb.half_plane_vectors(3)
    sim = fresh_sim(pb, orc, len(recs[0]))
    rows, back = record_manually(sim, recs, 2, 3, vectors)
    for row, want in zip(rows[1], float64_products(back, vectors, 3)):
        bound = product_bound(row["nx"], row["ny"], 3, row["bots_now"], row["bots_then"])
        err_re, err_im = abs(row["re"] / 2.0 ** 60 - want.real), abs(row["im"] / 2.0 ** 60 - want.imag)
        print(row["nx"], row["ny"], err_re, err_im, bound)
        assert row["bots_now"] == row["bots_then"] == 1000
        assert err_re <= bound and err_im <= bound
    sim.close()


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


def six_recorders_on(sim, interval, vectors):
    sim.set_series(interval, 512)
    sim.set_time_correlation(interval, LAGS, 0.015625)
    sim.set_scattering(interval, LAGS, BOX, vectors)
    sim.set_van_hove(interval, LAGS, WIDTH, BINS)
    sim.set_van_hove_distinct(interval, LAGS, WIDTH, BINS)
    sim.set_centroid_trail(True)


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
    # a: the recorder alone; b: the twin, everything off; c: the six existing recorders and this one; o: the six without
    # it; d: the time correlation alone
    a, b, c, o, d = (stepping_sim(pb, orc, form, wave) for _ in range(5))
    assert a.config()["resident"] == (1 if name == "resident" else 0)
    for s in (c, o):
        six_recorders_on(s, interval, vectors)
    for s in (a, c):
        s.set_coherent_scattering(interval, LAGS, BOX, vectors)
    d.set_time_correlation(interval, LAGS, 0.015625)
    assert a.coherent_scattering_info() == {"interval": float(f32(interval)), "lags": LAGS, "box_log2": BOX, "nvec": 24,
                                            "records": 0}
    for s in (a, c, o, d):
        assert s.step(steps, dt=DT, sort_interval=SORT) == steps  # one call
    assert a.coherent_scattering_info()["records"] == c.coherent_scattering_info()["records"] == len(rec)
    got = a.coherent_scattering()[0]
    states = twin_states(b, gates, steps)[0]
    want = CR.table([p for p, _ in states], rec, LAGS, vectors, BOX)
    print(name, wave, got[1][0])
    assert got == want, (name, wave)
    assert [g[0]["origins"] for g in got] == [len(rec) - l for l in range(LAGS)]
    assert all(r["bots_now"] == r["bots_then"] == 300 * r["origins"] for g in got for r in g)
    assert all(r["im"] == 0 for r in got[0])
    if interval:  # 25 steps between records: the blob moved, and the density waves with it
        assert any(r["im"] != 0 for r in got[LAGS - 1])
    lay = layout_of(a)
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(300))  # sorted: the slots are not in original order
    # the final state is the twin's, bit for bit, whichever recorders ran
    sb = b.get_state()
    for s in (a, c, o, d):
        st = s.get_state()
        for k in sb:
            assert_bit_equal(st[k], sb[k], f"{name} {k}")
        assert s.time == b.time
    # beside the six: the same table, and each of them gives what it gives without this one
    assert c.coherent_scattering()[0] == got
    assert c.time_correlation() == o.time_correlation() == d.time_correlation()
    assert d.time_correlation()[0] == TR.table(states, rec, LAGS, 0.015625)
    assert c.series_of(0) == o.series_of(0) and len(o.series_of(0)) == len(rec)
    assert c.scattering() == o.scattering() and c.van_hove() == o.van_hove()
    assert c.van_hove_distinct() == o.van_hove_distinct()
    (cxy, ct, cn), (oxy, ot, on) = c.centroid_trail(), o.centroid_trail()
    assert_bit_equal(cxy, oxy, f"{name} trail")
    assert_bit_equal(ct, ot, f"{name} trail times")
    assert cn == on > 0
    # the launches are those of a run with only the time correlation on at that interval
    assert a.stats() == d.stats() and c.stats() == o.stats()
    assert a.stats()["steps"] == steps and a.stats()["resorts"] == len(sorts) and a.stats()["phase_updates"] == len(phases)
    if name == "resident":
        assert a.stats()["resident_launches"] > 0
    if name == "every_step":
        assert a.stats()["fused_launches"] == 0  # interval 0 costs the fusion
    elif name != "resident":
        assert a.stats()["fused_launches"] > 0
    n, ms = a.coherent_scattering_times()
    assert n == len(rec) and ms > 0.0
    for s in (a, b, c, o, d):
        s.close()


def test_reading_and_recording_change_nothing(pb, orc):
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, phase_update_interval=0.3)
    vectors = vector_list(3)
    sim.set_series(0.1, 8)
    sim.set_time_correlation(0.1, 3, 0.5)
    sim.set_scattering(0.1, 3, BOX, vectors)
    sim.set_coherent_scattering(-1.0, 3, BOX, vectors)
    assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    assert sim.coherent_scattering_info()["records"] == 0  # manual only
    before, stats, lay, t = sim.get_state(), sim.stats(), layout_of(sim), sim.time
    series, corr, scat = sim.series_of(0), sim.time_correlation(), sim.scattering()
    sim.coherent_scattering_record()
    sim.coherent_scattering_record()
    first = sim.coherent_scattering()
    assert first == sim.coherent_scattering()
    assert first[0] == CR.table([before["pos"]] * 2, [60, 60], 3, vectors, BOX)
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
    sim.coherent_scattering_record()
    assert sim.coherent_scattering()[0] == CR.table([before["pos"]] * 2 + [now["pos"]], [60, 60, 67], 3, vectors, BOX)
    assert sim.coherent_scattering_times()[0] == 3 and sim.coherent_scattering_times()[1] > 0.0
    sim.close()


# ---- life cycle --------------------------------------------------------------------------------------------------------

def test_restart_switch_off_and_argument_errors(pb, orc):
    start = live_memory()
    pos, vel, rad = recipe(300)
    a = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0, phase_update_interval=PUI)
    a.set_resident(1)
    made = live_memory()
    vectors = vector_list(65)
    assert a.coherent_scattering_info() == OFF and a.coherent_scattering_times() == (0, 0.0)
    for call in (a.coherent_scattering_record, a.coherent_scattering):
        with pytest.raises(RuntimeError, match="code 2.*the coherent scattering is off"):
            call()
    for bad, word in (((-0.5, 4, 3, vectors), "interval"), ((float("nan"), 4, 3, vectors), "interval"),
                      ((0.0, 65, 3, vectors), "lags"), ((0.0, 4, 13, vectors), "boxLog2"), ((0.0, 4, -9, vectors), "boxLog2"),
                      ((0.0, 4, 3, vector_list(257)), "nvec"), ((0.0, 4, 3, np.zeros((0, 2), np.int32)), "nvec")):
        with pytest.raises(RuntimeError, match="code 2.*pbSimSetCoherent.*" + word):
            a.set_coherent_scattering(*bad)
    assert a.coherent_scattering_info() == OFF and live_memory() == made
    a.set_coherent_scattering(0.0, 4, 3, vectors)
    # the ring of modes, the cells, the measured counts, the phasors and the list
    assert live_memory() == (made[0] + 5, made[1] + 4 * 65 * 16 + 4 * 65 * 64 + 4 * 4 + 4096 * 8 + 65 * 8)
    vectors[:] = 0  # the list was copied at the call
    assert a.step(20, dt=DT, sort_interval=SORT) == 20 and a.coherent_scattering_info()["records"] == 20
    rows = a.coherent_scattering()[0]
    assert [r[0]["origins"] for r in rows] == [20, 19, 18, 17] and [r[64]["sum_steps"] for r in rows] == [0, 19, 36, 51]
    assert [[r["nx"], r["ny"]] for r in rows[0]] == vector_list(65).tolist()
    # again: restarts at record 0 with a zeroed table
    a.set_coherent_scattering(0.05, 64, -8, vector_list(3))
    assert a.coherent_scattering_info() == {"interval": float(f32(0.05)), "lags": 64, "box_log2": -8, "nvec": 3,
                                            "records": 0}
    zero = a.coherent_scattering()[0]
    assert len(zero) == 64 and all(len(z) == 3 for z in zero)
    assert all(dict(r, nx=0, ny=0) == dict(dict.fromkeys(CR.FIELDS, 0), lag=l) for l, z in enumerate(zero) for r in z)
    gates = SR.gate_steps(a.time, DT, 0.05, 30, 1e9)
    assert a.step(30, dt=DT, sort_interval=SORT) == 30
    rows = a.coherent_scattering()[0]
    assert a.coherent_scattering_info()["records"] == len(gates) and 5 <= len(gates) <= 7
    assert [r[0]["origins"] for r in rows] == [max(len(gates) - l, 0) for l in range(64)]
    assert rows[1][2]["sum_steps"] == gates[-1][0] - gates[0][0]
    # lags 0 frees: the memory is back, later steps record nothing and are fused again
    a.set_coherent_scattering(0.05, 0, 0, None)
    assert a.coherent_scattering_info() == OFF and live_memory() == made
    stats = a.stats()
    assert a.step(30, dt=DT, sort_interval=SORT) == 30 and a.coherent_scattering_info() == OFF
    assert a.stats()["fused_launches"] == stats["fused_launches"] + 29  # every step but the call's last is fused again
    with pytest.raises(RuntimeError, match="code 2.*the coherent scattering is off"):
        a.coherent_scattering()
    assert a.coherent_scattering_times() == (0, 0.0)
    # destroyed with the ring live: nothing stays
    a.set_coherent_scattering(-1.0, 2, 3, vector_list(1))
    a.coherent_scattering_record()
    assert live_memory()[0] == made[0] + 5
    a.close()
    assert live_memory() == start


def test_legacy_engine_refuses(capfd):
    from particlerobotsimulations_amd import host
    h = host.HostSim(CFG, engine="legacy")
    capfd.readouterr()
    lib, vec = host.lib(), (C.c_int * 2)(1, 0)
    assert lib.pbHostSetCoherent(h._h, -1.0, 2, 3, vec, 1) == -1
    assert capfd.readouterr() == ("", "Particlebot::setCoherent: the coherent scattering needs the fused engine\n")
    assert lib.pbHostCoherentRecord(h._h) == -1
    assert capfd.readouterr() == ("", "Particlebot::coherentRecord: the coherent scattering needs the fused engine\n")
    h.close()


# ---- wide batches ------------------------------------------------------------------------------------------------------

WIDE_LAGS, WIDE_BOX = 3, 4


def wide_records(st, m):
    """Four records of member m: its marked and its present positions (the plants and the empty members included), and
    both again shifted by dyadic steps."""
    a, b = st.marked[m]["pos"], st.final[m]["pos"]
    return [a, b, (a + np.array([0.25, -0.125], f32)).astype(f32), (b + np.array([-0.5, 0.375], f32)).astype(f32)]


@pytest.mark.parametrize("name", W.MAIN)
def test_wide_batches_every_member_equals_the_restatement_and_a_lone_sim(pb, orc, name):
    st = W.state(name)
    vectors = vector_list(3)
    recs = [wide_records(st, m) for m in range(st.nsims)]
    sps = [simparams_from_orc(P) for P in st.params]
    ens = pb.Ensemble([sp for sp, _ in sps], wall_half=st.wall_half, keepalive=[k for _, k in sps])
    for m in range(st.nsims):
        ens.set_state_of(m, **st.marked[m])
    ens.set_coherent_scattering(-1.0, WIDE_LAGS, WIDE_BOX, vectors)
    for r in range(4):
        for m in range(st.nsims):
            ens.set_state_of(m, pos=recs[m][r])
        ens.coherent_scattering_record()
    got = ens.coherent_scattering()
    assert len(got) == st.nsims and ens.coherent_scattering_info()["records"] == 4 > WIDE_LAGS  # the ring wrapped
    want = [CR.table(recs[m], [0] * 4, WIDE_LAGS, vectors, WIDE_BOX) for m in range(st.nsims)]

    def check(m):
        assert got[m] == want[m], (got[m][1], want[m][1])
    assert W.every_member(st, "coherent scattering", check) == st.nsims
    # members differ, the empty last member holds zeros, a planted member shows fewer bots in its second record
    assert len({repr(r) for r in want}) >= st.nsims - 1
    assert all(r["re"] == r["bots_now"] == 0 for lag in got[st.nsims - 1] for r in lag)
    assert got[0][0][0]["bots_now"] == 4 * st.n - 2 * 3 and got[1][0][0]["bots_now"] == 4 * st.n
    # a lone Sim given the member's states
    sp, keep = simparams_from_orc(st.params[0])
    lone = pb.Sim(sp, wall_half=st.wall_half, keepalive=keep)
    lone.set_state(**st.marked[0])

    def check_alone(m):
        lone.set_coherent_scattering(-1.0, WIDE_LAGS, WIDE_BOX, vectors)
        for pos in recs[m]:
            lone.set_state(pos=pos)
            lone.coherent_scattering_record()
        assert lone.coherent_scattering()[0] == got[m], m
    assert W.every_member(st, "lone Sim", check_alone) == st.nsims
    lone.close()
    ens.close()


# ---- the runner ------------------------------------------------------------------------------------------------------

HEADER = "Lag, Nx, Ny, Origins, SumSteps, BotsNow, BotsThen, Re, Im, FRe, FIm"
COLUMNS = ("lag", "nx", "ny", "origins", "sum_steps", "bots_now", "bots_then", "re", "im")


def test_runner_writes_the_table_at_the_end_of_the_run(tmp_path):
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import _analysis, _capi, host
    over = dict(max_time="30", dump_interval="2.5")
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--coherent", "f.csv", "--coherent-lags", "4", "--coherent-nmax",
                                                      "2", "--coherent-box-log2", "4"],
                       capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "f.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 4 * 12
    cells = [l.split(", ") for l in lines[1:]]
    assert [int(c[0]) for c in cells] == [l for l in range(4) for _ in range(12)]
    assert [int(c[3]) for c in cells[::12]] == [12, 11, 10, 9] and all(int(c[6]) == 300 * int(c[3]) for c in cells)
    # the same rows from the class driven in-process through the host library's wrappers, with the runner's list
    flat = host.load_config(CFG, **over)
    h = host.HostSim(CFG, engine="fused", **over)
    lib = host.lib()
    vectors = np.ascontiguousarray(pb.half_plane_vectors(2), np.int32)
    assert lib.pbHostSetCoherent(h._h, flat.dump_interval, 4, 4, _capi.np_ptr(vectors), len(vectors)) == 0

    def info():
        return _analysis.read_info(_analysis.COHERENT_INFO, lambda *q: lib.pbHostCoherentInfo(h._h, *q))
    assert info() == {"interval": float(f32(flat.dump_interval)), "lags": 4, "box_log2": 4, "nvec": 12, "records": 0}
    while not h.finished:
        if h.advance(h.steps_until_dump()) == 0:
            break
    rows, count = (_capi.pbCoherentRow * 48)(), C.c_ulonglong(0)
    assert lib.pbHostCoherentRows(h._h, rows, 47, C.byref(count)) == -1 and count.value == 48  # too little room
    assert lib.pbHostCoherentRows(h._h, rows, 48, C.byref(count)) == 0 and count.value == 48
    want = [_capi.coherent_row(r) for r in rows]
    assert [", ".join(c[:9]) for c in cells] == [", ".join(str(w[k]) for k in COLUMNS) for w in want]
    for c, w in zip(cells, want):
        s = pb.coherent_scattering_summary(w)
        assert c[9] == "%.9g" % s["f_re"] and c[10] == "%.9g" % s["f_im"], (c, s)
    assert info()["records"] == 12
    assert lib.pbHostCoherentRecord(h._h) == 0 and info()["records"] == 13
    assert lib.pbHostSetCoherent(h._h, 0.0, 0, 0, None, 0) == 0 and info()["lags"] == 0  # off
    assert lib.pbHostCoherentRecord(h._h) == -1
    h.close()
    # the defaults: 32 lags, the 24 vectors of the half plane up to 3, the box that holds the walls
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--coherent", "g.csv"], capture_output=True, text=True,
                       timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "g.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 32 * 24
    assert [l.split(", ")[1:3] for l in lines[1:25]] == [[str(x), str(y)] for x, y in pb.half_plane_vectors(3).tolist()]


def test_runner_refuses_a_run_whose_table_cannot_fit(tmp_path):
    # the one cap is 2^31 origins per lag, whatever the bots: a record every 0.01 s up to 10^8 s is 10^10 records
    r = subprocess.run([RUN, CFG, "--quiet", "--set", "max_time", "100000000", "--coherent", "f.csv",
                        "--coherent-interval", "0.01"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    records = float(f32(1.0e8)) / float(f32(0.01)) + 2.0
    assert records >= 2.0 ** 31
    assert (r.returncode, r.stdout) == (2, "")
    assert r.stderr == ("--coherent: about %.0f records would pass 2^31 origins per lag: raise --coherent-interval or "
                        "lower max_time\n" % records)
    assert not os.path.exists(tmp_path / "f.csv")
    # 3 x 10^9 (bot, record) pairs, which the per-bot recorders refuse, are no obstacle here: the run starts (and is
    # ended by its first checkpoint step, as a killed process would be)
    r = subprocess.run([RUN, CFG, "--quiet", "--set", "max_time", "100000", "--coherent", "f.csv", "--coherent-interval",
                        "0.01", "--stop-after-steps", "3"], capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 9 and "would pass" not in r.stderr
