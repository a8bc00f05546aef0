"""GPU: the recorders on a batch of 257 members (wide_batch_cases.FINITE: 257 x 40, finite states, nothing planted):
the time correlation, the scattering function and both van Hove functions take manual records of states written with
set_state_of, and all five recorders, the series included, are fired by one step() call; EVERY member's rows are
compared with the recorder's restatement (tests/series_ref.py, timecorr_ref.py, scatter_ref.py, vanhove_ref.py,
vanhove_distinct_ref.py) exactly, as the recorder's own test file compares them.  The four lagged tables are
member-major; a stride or a division that is off by one lag or one block stays inside the table of three members and
shows as a shifted member here.

The series takes no manual records (pbSimSetSeries refuses the interval -1), so it runs in the stepping test only; its
row writer is the one moments() uses, which tests/test_gpu_wide_batches.py compares on every member."""
import time

import numpy as np
import pytest

import analysis_session_cases as AC
import scatter_ref as XR
import series_ref as MR
import timecorr_ref as TR
import vanhove_distinct_ref as DR
import vanhove_ref as VR
import wide_batch_cases as W
from helpers import assert_bit_equal, simparams_from_orc

pytestmark = pytest.mark.gpu
f32 = np.float32
DT, SORT = 0.01, 0.5
LAGS, CAPACITY = 4, 8
RADIUS = 0.0625                     # the overlap function's a
BOX = 4
BINS = 8
MANUAL_RECORDS = 6
MANUAL_DRIFT = 0.04                 # per record and axis: one lag moves a bot 0.057, three lags 0.17
MANUAL_SELF_WIDTH = 0.02            # 8 bins reach 0.16: lag 1 falls inside, lag 3 beyond
MANUAL_DISTINCT_WIDTH = 0.05        # 8 bins reach 0.4: the neighbours at 0.19 inside, the far side of the blob beyond
INTERVAL, STEPS = 0.05, 40
STEP_SELF_WIDTH, STEP_DISTINCT_WIDTH = 0.002, 0.05


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def make(pb, st):
    sps = [simparams_from_orc(P) for P in st.params]
    sim = pb.Ensemble([sp for sp, _ in sps], wall_half=st.wall_half, keepalive=[k for _, k in sps])
    for k in range(st.nsims):
        sim.set_state_of(k, **st.marked[k])
    return sim


def switch_on(sim, interval, self_width, distinct_width, series):
    if series:
        sim.set_series(interval, CAPACITY)
    sim.set_time_correlation(interval, LAGS, RADIUS)
    sim.set_scattering(interval, LAGS, BOX, AC.sk_vectors(W.SK_COUNT))
    sim.set_van_hove(interval, LAGS, self_width, BINS)
    sim.set_van_hove_distinct(interval, LAGS, distinct_width, BINS)


def manual_records(st):
    """Per member the (pos, vel) of every record: a drift of MANUAL_DRIFT per record with dynamics_ref.perturbed's noise,
    the velocities fading, each member from its own seed."""
    out = []
    for k in range(st.nsims):
        rng = np.random.default_rng(52000 + k)
        pos, vel = st.marked[k]["pos"], st.marked[k]["vel"]
        recs = []
        for r in range(MANUAL_RECORDS):
            recs.append((pos, (vel * f32(1.0 - 0.1 * r)).astype(f32)))
            pos = W.YR.perturbed(pos, rng, shift=MANUAL_DRIFT)
        out.append(recs)
    return out


def check_tables(st, sim, states, steps, self_width, distinct_width):
    """Every member's rows of the four lagged tables against the restatements on `states` (per member the (pos, vel)
    of every record) taken at `steps`.  Returns the references, per table the list over members."""
    vectors = AC.sk_vectors(W.SK_COUNT)
    got = {"time correlation": sim.time_correlation(), "scattering": sim.scattering(), "van Hove": sim.van_hove(),
           "distinct van Hove": sim.van_hove_distinct()}
    rad = [st.marked[m]["rad"] for m in range(st.nsims)]
    want = {
        "time correlation": [TR.table(states[m], steps, LAGS, RADIUS) for m in range(st.nsims)],
        "scattering": [XR.table([p for p, _ in states[m]], steps, LAGS, vectors, BOX) for m in range(st.nsims)],
        "van Hove": [VR.table([p for p, _ in states[m]], steps, LAGS, self_width, BINS) for m in range(st.nsims)],
        "distinct van Hove": [DR.table([(p, rad[m]) for p, _ in states[m]], steps, LAGS, distinct_width, BINS)
                              for m in range(st.nsims)],
    }
    counts = {}
    for name in got:
        assert len(got[name]) == st.nsims and all(len(rows) == LAGS for rows in got[name]), name

        def check(m, name=name):
            assert got[name][m] == want[name][m], (got[name][m][1], want[name][m][1])
        counts[name] = W.every_member(st, name, check)
    return want, counts


def test_manual_records_every_member(pb, orc):
    st = W.state(W.FINITE)
    recs = manual_records(st)
    t0 = time.perf_counter()
    sim = make(pb, st)
    switch_on(sim, -1.0, MANUAL_SELF_WIDTH, MANUAL_DISTINCT_WIDTH, series=False)
    for r in range(MANUAL_RECORDS):
        for k in range(st.nsims):
            sim.set_state_of(k, pos=recs[k][r][0], vel=recs[k][r][1])
        sim.time_correlation_record()
        sim.scattering_record()
        sim.van_hove_record()
        sim.van_hove_distinct_record()
    for info in (sim.time_correlation_info(), sim.scattering_info(), sim.van_hove_info(), sim.van_hove_distinct_info()):
        assert info["records"] == MANUAL_RECORDS > LAGS and info["lags"] == LAGS  # the ring wrapped
    for m in (0, 128, st.nsims - 1):  # what was written is what the device holds
        back = sim.get_state_of(m)
        assert_bit_equal(back["pos"], recs[m][-1][0], f"member {m} pos")
        assert_bit_equal(back["vel"], recs[m][-1][1], f"member {m} vel")
    want, counts = check_tables(st, sim, recs, [0] * MANUAL_RECORDS, MANUAL_SELF_WIDTH, MANUAL_DISTINCT_WIDTH)
    seconds = time.perf_counter() - t0
    # from the references: in every member displacements and pair distances fall inside the bins at one lag and beyond
    # them at another, bots lie on both sides of the overlap radius, and no two members have equal rows
    for m in range(st.nsims):
        self_rows, pair_rows, tc = want["van Hove"][m], want["distinct van Hove"][m], want["time correlation"][m]
        assert all(VR.identities_hold(r) for r in self_rows)
        assert any(sum(r["radial"]) > 0 for r in self_rows[1:]) and any(r["beyond_r"] > 0 for r in self_rows[1:]), m
        assert all(0 < r["pairs"] < r["origins"] * st.n * (st.n - 1) for r in pair_rows), m
        assert [r["samples"] for r in tc] == [st.n * (MANUAL_RECORDS - l) for l in range(LAGS)]
        assert 0 < tc[1]["overlap"] and tc[LAGS - 1]["overlap"] < tc[LAGS - 1]["samples"], m
    for name, rows in want.items():
        assert len({repr(r) for r in rows}) == st.nsims, name
    assert set(counts.values()) == {st.nsims}
    print(f"manual records: {seconds:.2f} s with the references; members compared {counts}")


def test_records_fired_by_one_step_call_equal_a_twin_stopped_at_every_gate(pb, orc):
    st = W.state(W.FINITE)
    gates = MR.gate_steps(0.0, DT, INTERVAL, STEPS, 1e9)
    rec = [k for k, _ in gates]
    # eight records in the fp32 clock (the series' ring fills, the lag rings wrap), unevenly spaced: sum_steps tells lags apart
    assert rec == [0, 6, 11, 16, 20, 25, 31, 36] and len(rec) == CAPACITY > LAGS
    t0 = time.perf_counter()
    a, b = make(pb, st), make(pb, st)
    switch_on(a, INTERVAL, STEP_SELF_WIDTH, STEP_DISTINCT_WIDTH, series=True)
    assert a.step(STEPS, dt=DT, sort_interval=SORT) == STEPS  # one call
    # the twin: no recorder, stopped in front of every step the gate names, every member read back
    full, at = [[] for _ in range(st.nsims)], 0
    for k, t in gates:
        if k > at:
            assert b.step(k - at, dt=DT, sort_interval=SORT) == k - at
            at = k
        assert f32(b.time) == f32(t), (k, b.time, t)
        for m in range(st.nsims):
            full[m].append(b.get_state_of(m))
    assert b.step(STEPS - at, dt=DT, sort_interval=SORT) == STEPS - at
    states = [[(s["pos"], s["vel"]) for s in full[m]] for m in range(st.nsims)]
    assert all(np.isfinite(s[k]).all() for m in (0, st.nsims - 1) for s in full[m] for k in ("pos", "vel", "rad"))
    assert a.stats()["resorts"] == b.stats()["resorts"] >= 1 and a.stats()["steps"] == b.stats()["steps"] == STEPS
    for info in (a.time_correlation_info(), a.scattering_info(), a.van_hove_info(), a.van_hove_distinct_info(),
                 a.series_info()):
        assert info["records"] == len(rec)
    # the radii move while stepping: the distinct part files the radii of the record itself
    vectors = AC.sk_vectors(W.SK_COUNT)
    got = {"time correlation": a.time_correlation(), "scattering": a.scattering(), "van Hove": a.van_hove(),
           "distinct van Hove": a.van_hove_distinct()}
    want = {
        "time correlation": lambda m: TR.table(states[m], rec, LAGS, RADIUS),
        "scattering": lambda m: XR.table([p for p, _ in states[m]], rec, LAGS, vectors, BOX),
        "van Hove": lambda m: VR.table([p for p, _ in states[m]], rec, LAGS, STEP_SELF_WIDTH, BINS),
        "distinct van Hove": lambda m: DR.table([(s["pos"], s["rad"]) for s in full[m]], rec, LAGS, STEP_DISTINCT_WIDTH,
                                                BINS),
    }
    counts = {}
    for name in got:
        assert len(got[name]) == st.nsims

        def check(m, name=name):
            assert got[name][m] == want[name](m), m
        counts[name] = W.every_member(st, name, check)

    def check_series(m):
        rows = a.series_of(m)
        assert len(rows) == len(rec)
        for row, (k, t), s in zip(rows, gates, full[m]):
            assert row["step"] == k and f32(row["time"]) == f32(t), (row["step"], k)
            assert {key: row[key] for key in MR.FIELDS} == MR.moments(s["pos"], s["vel"], s["rad"]), k
    counts["series"] = W.every_member(st, "series", check_series)
    moved = sum(not np.array_equal(full[m][0]["pos"], full[m][-1]["pos"]) for m in range(st.nsims))
    assert moved == st.nsims  # every member moved between its first and its last record
    # reading back and recording changed nothing: every member's final state is the twin's
    def check_state(m):
        sa, sb = a.get_state_of(m), b.get_state_of(m)
        for key in sa:
            assert_bit_equal(sa[key], sb[key], f"member {m} {key}")
    counts["final state"] = W.every_member(st, "final state", check_state)
    assert a.time == b.time and set(counts.values()) == {st.nsims}
    print(f"records fired by step(): {time.perf_counter() - t0:.2f} s with the references; members compared {counts}")
