"""GPU: the distinct van Hove function (pbSimSetVanHoveDistinct / pbSimVanHoveDistinctRecord / pbSimGetVanHoveDistinct,
csrc/pb_vanhove_distinct.hip) against tests/vanhove_distinct_ref.py on states read back from the device.  Every
comparison is exact: a row and its counters hold integers only, and the reference is an all-pairs loop that knows nothing
of cells.  A table recorded while stepping is compared with a twin run that has the analysis off and is stopped in front
of every step the gate names.  tests/test_vanhove_distinct_ref.py pins the reference to a plain loop and to known
answers on the CPU, and shows that the recipe used here fills every bin and moves bots out of their cells.

Not run here, as in tests/test_gpu_vanhove.py: the refusals that need a batch of 2^28 bots, of more than 65535 members, a
ring above 2^33 bytes or a table above 2^31 bytes, and a lag with 2^31 centres: none fits a test of a few seconds.  They
are comparisons in front of the allocation in pbSimSetVanHoveDistinct, and pbLagFetch's in front of the rows."""
import os
import subprocess

import numpy as np
import pytest

import series_ref as SR
import timecorr_ref as TR
import vanhove_distinct_ref as DR
import vanhove_ref as VR
from helpers import assert_bit_equal
from test_gpu_scatter import stepping_sim
from test_gpu_series import DT, FORMS, INTERVAL, PUI, SORT, STEPS, layout_of, make_batch, sim_with
from test_gpu_sfactor import live_memory
from test_gpu_timecorr import same_bits, twin_states
from test_series_api import CORNER, recipe
from test_timecorr_api import BATCH_BOTS, batch_records
from test_vanhove_api import MANUAL_LAGS, MANUAL_RECORDS, vanhove_records
from test_vanhove_distinct_ref import KNOWN_BINS, KNOWN_WIDTH, SHAPES, absent_cases, known_answer_records, known_answer_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000]
LAGS, WIDTH, BINS = 5, 1.0 / 32, 32  # while stepping: rMax = 1 inside a blob a few units across
OFF = {"interval": 0.0, "lags": 0, "width": 0.0, "bins": 0, "records": 0}


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def same_values(got, put):
    """Bit-equal where `put` is a number, NaN where it is NaN."""
    got, put = np.asarray(got, f32), np.asarray(put, f32)
    nan = np.isnan(put)
    return np.array_equal(np.isnan(got), nan) and same_bits(got[~nan], put[~nan])


def record_manually(sim, records, lags, width, bins):
    """Sets each of `records` ((pos, rad)) and takes a record of it; returns the member's rows and the (pos, rad) read
    back."""
    n = len(records[0][0])
    sim.set_van_hove_distinct(-1.0, lags, width, bins)
    assert sim.van_hove_distinct_info() == {"interval": -1.0, "lags": lags, "width": float(f32(width)), "bins": bins,
                                            "records": 0}
    back = []
    zeros = np.zeros((n, 2), f32)
    for pos, rad in records:
        sim.set_state(pos=pos, vel=zeros, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
        st = sim.get_state()
        back.append((st["pos"], st["rad"]))
        sim.van_hove_distinct_record()
    assert sim.van_hove_distinct_info()["records"] == len(records)
    return sim.van_hove_distinct()[0], back


def fresh_sim(pb, orc, n):
    return sim_with(pb, orc, np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.full(n, 0.1, f32))


def with_rad(positions, rad=0.1):
    return [(p, np.full(len(p), rad, f32)) for p in positions]


def shape_of(n, where):
    return SHAPES[(SIZES.index(n) + (where == "corner")) % len(SHAPES)]


def manual_records_of(n, where):
    return with_rad([r[0] for r in vanhove_records(n, center=CORNER if where == "corner" else (0.0, 0.0))])


# ---- manual records on set states ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", ["origin", "corner"])
def test_manual_records_around_the_wave_and_the_workgroup(pb, orc, n, where):
    width, bins = shape_of(n, where)
    recs = manual_records_of(n, where)
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, MANUAL_LAGS, width, bins)
    for (p, r), rec in zip(back, recs):
        assert same_bits(p, rec[0]) and same_bits(r, rec[1])
    want = DR.table(back, [0] * MANUAL_RECORDS, MANUAL_LAGS, width, bins)
    print(n, where, width, bins, {k: rows[1][k] for k in DR.FIELDS})
    assert rows == want, (n, where, width, bins)
    assert [r["origins"] for r in rows] == [7, 6, 5]
    assert [r["centres"] for r in rows] == [7 * n, 6 * n, 5 * n] == [r["partners"] for r in rows]
    assert all(r["pairs"] == sum(r["counts"]) for r in rows) and all(c % 2 == 0 for c in rows[0]["counts"])
    if n >= 63:
        assert rows[1]["pairs"] > 0 and rows[0]["pairs"] > 0
    if n == 1:
        assert all(r["pairs"] == 0 for r in rows)  # a lone bot has no other bot
    sim.close()


@pytest.mark.parametrize("n", [n for n in SIZES if n >= 63])
def test_the_recipe_needs_the_walk_around_the_earlier_position(n):
    """Conditions on the inputs of the test above, computed in the reference alone: at every size at least one of the two
    shapes has counted pairs at lag 1 whose partner is outside the nine cells around the centre bot's CURRENT position:
    a sweep centred there would get the table above wrong.  (n = 1 has no other bot, and the two bots of n = 2 are counted
    at the corner only, 8 pairs, none of them outside the nine cells: no shape can show it at those two sizes.)"""
    missed = []
    for where in ("origin", "corner"):
        width, bins = shape_of(n, where)
        recs = manual_records_of(n, where)
        missed.append(sum(DR.missed_around_the_current_position(recs[r], recs[r - 1], width, bins) for r in (1, 2)))
    print(n, missed)
    assert max(missed) > 0, (n, missed)


def test_more_than_sixteen_workgroups_off_the_origin(pb, orc):
    n = 4097  # 17 workgroups of 256 lanes, a grid of 128 x 64 cells
    recs = with_rad([r[0] for r in vanhove_records(n, records=2, center=(-300.0, 700.0))])
    sim = fresh_sim(pb, orc, n)
    rows, back = record_manually(sim, recs, 2, 1.0 / 16, 64)
    want = DR.table(back, [0, 0], 2, 1.0 / 16, 64)
    assert rows == want
    assert [r["centres"] for r in rows] == [2 * n, n] and rows[1]["pairs"] > n and min(rows[1]["counts"][1:]) > 0
    assert DR.grid_of(n, 1.0 / 16, 64)[1:] == (128, 64)
    sim.close()


def test_known_answers_and_absent_bots(pb, orc):
    sim = fresh_sim(pb, orc, 5)
    recs = known_answer_records()
    rows, back = record_manually(sim, recs, 2, KNOWN_WIDTH, KNOWN_BINS)
    for (p, r), rec in zip(back, recs):
        assert same_bits(p, rec[0]) and same_bits(r, rec[1])
    assert rows == [dict(k, sum_steps=0) for k in known_answer_rows()]  # (no step ran between the records)
    for name, recs, lag1 in absent_cases():
        rows, back = record_manually(sim, recs, 2, KNOWN_WIDTH, KNOWN_BINS)  # (the setter restarts at record 0)
        for (p, r), rec in zip(back, recs):
            assert same_values(p, rec[0]) and same_values(r, rec[1]), name
        assert rows[1] == dict(lag1, sum_steps=0), name
        assert rows == DR.table(back, [0, 0], 2, KNOWN_WIDTH, KNOWN_BINS), name
    sim.close()
    # nobody present: an all-zero table with the origins counted
    bad = np.full((65, 2), np.nan, f32)
    sim = fresh_sim(pb, orc, 65)
    rows, _ = record_manually(sim, with_rad([bad, bad]), 2, 0.5, 4)
    assert rows == [dict(DR.empty_row(0, 4), origins=2), dict(DR.empty_row(1, 4), origins=1)]
    sim.close()


def test_batch_of_three_members_do_not_leak_into_each_other(pb, orc):
    n, recs = BATCH_BOTS, batch_records()
    ens = make_batch(pb, orc, 3, n)
    ens.set_van_hove_distinct(-1.0, 3, 0.25, 32)
    back = [[] for _ in range(3)]
    for r in range(4):
        for k in range(3):
            pos, vel, rad = recs[k][r]
            ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
            st = ens.get_state_of(k)
            assert same_bits(st["pos"], pos)
            back[k].append((st["pos"], st["rad"]))
        ens.van_hove_distinct_record()
    rows = ens.van_hove_distinct()
    assert len(rows) == 3 and all(len(r) == 3 for r in rows)
    for k in range(3):
        assert rows[k] == DR.table(back[k], [0] * 4, 3, 0.25, 32), k
        assert [r["centres"] for r in rows[k]] == [4 * n, 3 * n, 2 * n] and rows[k][1]["pairs"] > 0
    assert rows[0][1]["counts"] != rows[1][1]["counts"] != rows[2][1]["counts"]
    assert ens.van_hove_distinct() == rows  # twice: the same rows
    ens.close()


# ---- recorded while stepping -----------------------------------------------------------------------------------------

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
    # b: the twin, everything off
    b = stepping_sim(pb, orc, form, wave)
    states = twin_states(b, gates, steps)[0]
    assert np.isfinite(b.get_state()["rad"]).all()  # (every bot is present throughout: the radii stay finite)
    want = DR.table(with_rad([p for p, _ in states]), rec, LAGS, WIDTH, BINS)
    # a broad histogram, and a range that leaves most pairs out: the cell rejection has work to do
    assert sum(1 for c in want[LAGS - 1]["counts"] if c) >= BINS // 2
    assert 0 < 2 * want[LAGS - 1]["pairs"] < want[LAGS - 1]["centres"] * 299
    # a: the distinct part alone; c: all five recorders; d: the time correlation alone; e: the series alone;
    # g: the scattering alone; h: the self part alone
    a, c, d, e, g, h = (stepping_sim(pb, orc, form, wave) for _ in range(6))
    assert a.config()["resident"] == (1 if name == "resident" else 0)
    vectors = pb.half_plane_vectors(2)
    for s in (a, c):
        s.set_van_hove_distinct(interval, LAGS, WIDTH, BINS)
    for s in (c, d):
        s.set_time_correlation(interval, LAGS, 0.015625)
    for s in (c, e):
        s.set_series(interval, 512)
    for s in (c, g):
        s.set_scattering(interval, LAGS, 3, vectors)
    for s in (c, h):
        s.set_van_hove(interval, LAGS, WIDTH, BINS)
    assert a.van_hove_distinct_info() == {"interval": float(f32(interval)), "lags": LAGS, "width": WIDTH, "bins": BINS,
                                          "records": 0}
    for s in (a, c, d, e, g, h):
        assert s.step(steps, dt=DT, sort_interval=SORT) == steps  # one call
    assert a.van_hove_distinct_info()["records"] == c.van_hove_distinct_info()["records"] == len(rec)
    got = a.van_hove_distinct()[0]
    print(name, wave, {k: got[LAGS - 1][k] for k in DR.FIELDS})
    assert got == want, (name, wave)
    assert [r["origins"] for r in got] == [len(rec) - l for l in range(LAGS)]
    assert all(r["centres"] == 300 * r["origins"] == r["partners"] for r in got)
    lay = layout_of(a)
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(300))  # sorted: the slots are not in original order
    # the final state is the twin's, bit for bit, whichever recorders ran
    sb = b.get_state()
    for s in (a, c, d, e, g, h):
        st = s.get_state()
        for k in sb:
            assert_bit_equal(st[k], sb[k], f"{name} {k}")
        assert s.time == b.time
    # each recorder gives what it gives alone
    assert c.van_hove_distinct()[0] == got
    tc = c.time_correlation()
    assert tc == d.time_correlation() and tc[0] == TR.table(states, rec, LAGS, 0.015625)
    assert c.series_of(0) == e.series_of(0) and len(e.series_of(0)) == len(rec)
    assert c.scattering() == g.scattering()
    assert c.van_hove() == h.van_hove() and c.van_hove()[0] == VR.table([p for p, _ in states], rec, LAGS, WIDTH, BINS)
    # the launches are those of a run with only the time correlation on at that interval
    assert a.stats() == d.stats() == c.stats() == e.stats() == g.stats() == h.stats()
    assert a.stats()["steps"] == steps and a.stats()["resorts"] == len(sorts) and a.stats()["phase_updates"] == len(phases)
    if name == "resident":
        assert a.stats()["resident_launches"] > 0
    if name == "every_step":
        assert a.stats()["fused_launches"] == 0  # interval 0 costs the fusion
    elif name != "resident":
        assert a.stats()["fused_launches"] > 0
    n, ms = a.van_hove_distinct_times()
    assert n == len(rec) and ms > 0.0
    for s in (a, b, c, d, e, g, h):
        s.close()


# ---- the scratch it shares with the on-demand analyses -------------------------------------------------------------------

def on_demand_session(pb, orc, with_records):
    """mark; radial counts; record; cluster stats; record; contacts; pair correlation; rearrangement compare, on a state
    that moves between the mark and the rest.  Returns every result and every run counter."""
    recs = [r for r in vanhove_records(300, records=3)]
    sim = sim_with(pb, orc, *recs[0])
    out = {}
    if with_records:
        sim.set_van_hove_distinct(-1.0, 2, 0.125, 16)
    sim.mark_reference(0.05)
    n = 300
    sim.set_state(pos=recs[1][0], vel=recs[1][1], rad=recs[1][2], phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    out["radial"] = sim.radial_counts(2.0, 32).tolist()
    if with_records:
        sim.van_hove_distinct_record()
    out["clusters"] = sim.clusters(0.05)
    if with_records:
        sim.van_hove_distinct_record()
    contacts = sim.contacts(0.05)
    out["contacts"] = {k: v.tobytes() for k, v in contacts.items()}
    rows, totals = sim.pair_correlation("velocity", 2.0, 16)
    out["correlation"] = (rows.tobytes(), totals)
    out["rearrangement"] = sim.rearrangement()
    out["rearrangement_of"] = {k: v.tobytes() for k, v in sim.rearrangement_of(0).items()}
    out["reference"] = sim.reference_info()
    out["runs"] = [f()[0] for f in (sim.cluster_times, sim.contact_times, sim.structure_times, sim.rearrangement_times,
                                    sim.correlation_times)]
    table = sim.van_hove_distinct()[0] if with_records else None
    state = (recs[1][0], recs[1][2])
    sim.close()
    return out, table, state


def test_records_between_on_demand_analyses_change_none_of_them(pb, orc):
    mixed, table, state = on_demand_session(pb, orc, True)
    fresh, _, _ = on_demand_session(pb, orc, False)
    assert mixed == fresh
    assert min(fresh["runs"]) >= 1 and fresh["reference"]["marked"] and sum(fresh["radial"][0]) > 0
    # the table is that of a session that ran nothing else
    sim = fresh_sim(pb, orc, 300)
    alone, _ = record_manually(sim, [state, state], 2, 0.125, 16)
    sim.close()
    assert table == alone == DR.table([state, state], [0, 0], 2, 0.125, 16) and table[1]["pairs"] > 0


def test_reading_and_recording_change_nothing(pb, orc):
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, phase_update_interval=0.3)
    sim.set_series(0.1, 8)
    sim.set_time_correlation(0.1, 3, 0.5)
    sim.set_van_hove(0.1, 3, 0.03125, 32)
    sim.set_van_hove_distinct(-1.0, 3, 0.03125, 32)
    assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    assert sim.van_hove_distinct_info()["records"] == 0  # manual only
    before, stats, lay, t = sim.get_state(), sim.stats(), layout_of(sim), sim.time
    series, corr, vh = sim.series_of(0), sim.time_correlation(), sim.van_hove()
    sim.van_hove_distinct_record()
    sim.van_hove_distinct_record()
    first = sim.van_hove_distinct()
    assert first == sim.van_hove_distinct()
    here = (before["pos"], before["rad"])
    assert first[0] == DR.table([here] * 2, [60, 60], 3, 0.03125, 32)
    after = sim.get_state()
    for k in before:
        assert_bit_equal(before[k], after[k], k)
    assert sim.stats() == stats and sim.time == t
    assert sim.series_of(0) == series and sim.time_correlation() == corr and sim.van_hove() == vh
    for x, y in zip(lay, layout_of(sim)):
        assert np.array_equal(x, y)
    # a later step and a set_state leave the ring alone: the next record pairs with the two it holds
    assert sim.step(7, dt=DT, sort_interval=0.2) == 7
    now = sim.get_state()
    sim.set_state(pos=now["pos"], vel=now["vel"], rad=now["rad"], phase=now["phase"], dead=now["dead"])
    sim.van_hove_distinct_record()
    rows = sim.van_hove_distinct()[0]
    assert rows == DR.table([here] * 2 + [(now["pos"], now["rad"])], [60, 60, 67], 3, 0.03125, 32)
    assert rows[1]["sum_steps"] == 7 and rows[2]["sum_steps"] == 7 and rows[1]["pairs"] > 0
    assert sim.van_hove_distinct_times()[0] == 3 and sim.van_hove_distinct_times()[1] > 0.0
    sim.close()


# ---- life cycle --------------------------------------------------------------------------------------------------------

def test_restart_switch_off_and_argument_errors(pb, orc):
    start = live_memory()
    pos, vel, rad = recipe(300)
    a = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0, phase_update_interval=PUI)
    a.set_resident(1)
    bare = live_memory()
    assert a.van_hove_distinct_info() == OFF and a.van_hove_distinct_times() == (0, 0.0)
    for call in (a.van_hove_distinct_record, a.van_hove_distinct):
        with pytest.raises(RuntimeError, match="code 2.*the distinct van Hove function is off"):
            call()
    for bad, word in (((-0.5, 4, 0.125, 64), "interval"), ((float("nan"), 4, 0.125, 64), "interval"),
                      ((0.0, 65, 0.125, 64), "lags"), ((0.0, 4, 0.125, 0), "bins"), ((0.0, 4, 0.125, 1025), "bins"),
                      ((0.0, 4, 0.0, 64), "binWidth"), ((0.0, 4, 2048.0, 64), "binWidth"),
                      ((0.0, 4, float("nan"), 64), "binWidth"), ((0.0, 4, 2.0 ** -22, 64), "quantum"),
                      ((0.0, 4, 32.0, 64), "below 2048"), ((0.0, 4, 2.0, 1024), "below 2048")):
        with pytest.raises(RuntimeError, match="code 2.*pbSimSetVanHoveDistinct.*" + word):
            a.set_van_hove_distinct(*bad)
    assert a.van_hove_distinct_info() == OFF and live_memory() == bare  # nothing was allocated, the scratch included
    # the shared scratch is the analysis layer's: made by whoever needs it first, kept until the batch goes
    a.radial_counts(1.0, 8)
    made = live_memory()
    a.set_van_hove_distinct(0.0, 4, 0.125, 48)
    # the ring, the table (two words and 48 counters per lag) and the 49 edges
    assert live_memory() == (made[0] + 3, made[1] + 4 * 300 * 8 + 4 * (2 + 48) * 8 + 49 * 8)
    assert a.step(20, dt=DT, sort_interval=SORT) == 20 and a.van_hove_distinct_info()["records"] == 20
    assert live_memory() == (made[0] + 3, made[1] + 4 * 300 * 8 + 4 * (2 + 48) * 8 + 49 * 8)  # no record allocates
    rows = a.van_hove_distinct()[0]
    assert [r["origins"] for r in rows] == [20, 19, 18, 17] and [r["sum_steps"] for r in rows] == [0, 19, 36, 51]
    assert all(r["centres"] == 300 * r["origins"] == r["partners"] and r["pairs"] == sum(r["counts"]) for r in rows)
    # again: restarts at record 0 with a zeroed table
    a.set_van_hove_distinct(0.05, 64, 0.5, 7)
    assert a.van_hove_distinct_info() == {"interval": float(f32(0.05)), "lags": 64, "width": 0.5, "bins": 7, "records": 0}
    assert a.van_hove_distinct()[0] == [DR.empty_row(l, 7) for l in range(64)]
    gates = SR.gate_steps(a.time, DT, 0.05, 30, 1e9)
    assert a.step(30, dt=DT, sort_interval=SORT) == 30
    rows = a.van_hove_distinct()[0]
    assert a.van_hove_distinct_info()["records"] == len(gates) and 5 <= len(gates) <= 7
    assert [r["origins"] for r in rows] == [max(len(gates) - l, 0) for l in range(64)]
    assert rows[1]["sum_steps"] == gates[-1][0] - gates[0][0]
    # lags 0 frees the ring, the table and the edges: later steps record nothing and are fused again
    a.set_van_hove_distinct(0.05, 0, 0.0, 0)
    assert a.van_hove_distinct_info() == OFF and live_memory() == made
    stats = a.stats()
    assert a.step(30, dt=DT, sort_interval=SORT) == 30 and a.van_hove_distinct_info() == OFF
    assert a.stats()["fused_launches"] == stats["fused_launches"] + 29  # every step but the call's last is fused again
    with pytest.raises(RuntimeError, match="code 2.*the distinct van Hove function is off"):
        a.van_hove_distinct()
    assert a.van_hove_distinct_times() == (0, 0.0)
    # a session that never filed: the setter makes the scratch, so that no record has to
    c = sim_with(pb, orc, pos, vel, rad)
    none = live_memory()
    c.set_van_hove_distinct(-1.0, 2, 1.0, 1)
    held = live_memory()
    assert held[0] > none[0] + 3
    c.van_hove_distinct_record()
    c.van_hove_distinct_record()
    assert live_memory() == held
    c.set_van_hove_distinct(-1.0, 0, 0.0, 0)
    assert live_memory() == (held[0] - 3, held[1] - (2 * 300 * 8 + 2 * 3 * 8 + 2 * 8))
    c.close()
    # destroyed with the ring live: nothing stays
    a.set_van_hove_distinct(-1.0, 2, 1.0, 1)
    a.van_hove_distinct_record()
    assert live_memory()[0] == made[0] + 3
    a.close()
    assert live_memory() == start


# ---- the runner ------------------------------------------------------------------------------------------------------

HEADER = "Lag, Origins, SumSteps, Centres, Partners, Pairs, Bin, Lower, Count"


def test_runner_writes_the_table_at_the_end_of_the_run(pb, tmp_path):
    from particlerobotsimulations_amd import host
    over = dict(max_time="30", dump_interval="2.5")
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--vanhove-distinct", "g.csv", "--vanhove-distinct-lags", "4",
                                                      "--vanhove-distinct-bins", "16", "--vanhove-distinct-width",
                                                      "0.03125"],
                       capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "g.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 4 * 16
    cells = [l.split(", ") for l in lines[1:]]
    # the same rows from the class driven in-process
    h = host.HostSim(CFG, engine="fused", **over)
    flat = host.load_config(CFG, **over)
    h.set_van_hove_distinct(flat.dump_interval, 4, 0.03125, 16)
    assert h.van_hove_distinct_info() == {"interval": float(f32(flat.dump_interval)), "lags": 4, "width": 0.03125,
                                          "bins": 16, "records": 0}
    while not h.finished:
        if h.advance(h.steps_until_dump()) == 0:
            break
    rows = h.van_hove_distinct()[0]
    assert [r["origins"] for r in rows] == [12, 11, 10, 9] and all(r["centres"] == 300 * r["origins"] for r in rows)
    assert all(r["pairs"] == sum(r["counts"]) for r in rows) and rows[3]["pairs"] > 0
    at = 0
    for row in rows:
        for j, count in enumerate(row["counts"]):
            lead = [str(row[k]) for k in ("lag", "origins", "sum_steps", "centres", "partners", "pairs")]
            assert cells[at][:6] == lead and cells[at][6] == str(j) and cells[at][8] == str(count), (cells[at], lead, j)
            assert float(cells[at][7]) == pytest.approx(j * 0.03125, rel=1e-8, abs=0.0)
            at += 1
    assert at == len(cells)
    assert h.van_hove_distinct_info()["records"] == 12
    h.van_hove_distinct_record()
    assert h.van_hove_distinct_info()["records"] == 13
    h.close()
    # the defaults: 32 lags of 64 bins, an eighth of min_radius wide
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--vanhove-distinct", "d.csv"], capture_output=True, text=True,
                       timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "d.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 32 * 64
    cells = [l.split(", ") for l in lines[1:]]
    assert [int(c[0]) for c in cells[::64]] == list(range(32)) and [int(c[6]) for c in cells[:64]] == list(range(64))
    eighth = VR.qw_of(f32(0.125) * f32(flat.min_radius)) / 2.0 ** 20
    assert float(cells[1][7]) == pytest.approx(eighth, rel=1e-8) and float(cells[63][7]) == pytest.approx(63 * eighth, rel=1e-8)
