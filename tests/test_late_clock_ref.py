"""The fp32 clock late in a run, on the CPU: series_ref's replay of `time = time + dt` and of the schedule's gate
against the oracle, from start times just below the powers of two at which the size of the clock's step changes, up to
the one at which it stands still.  tests/test_gpu_late_clock.py runs the engine from the same start times with the same
window and intervals; the conditions on those inputs (a boundary crossed at once, gates that fire on consecutive steps,
a standing clock) are asserted here, so that no case over there is trivial.  Every comparison is exact."""
import numpy as np
import pytest

import series_ref as SR

f32 = np.float32
DT = 0.01
STEPS = 400                      # the window: steps from every start time
MARKS = (1, 7, 230, 400)         # where the GPU tests compare
PUI, SORT, REC = 2.0, 0.5, 0.05  # phase-update, re-sort and record intervals
LATE = (4095.9, 16383.9, 32767.9, 65535.9, 131071.9, 262143.9)
NEGATIVE = -0.055
STARTS = LATE + (NEGATIVE,)
PAIRED = (4095.9, 16383.9, 65535.9)  # where a gate fires on two consecutive steps
STANDING = 262143.9
# replayed (firings, consecutive firings) of the intervals 2.0 / 0.5 / 0.05 in the window, per start time
FIRINGS = {
    4095.9: ((3, 1), (10, 2), (83, 5)),
    16383.9: ((3, 1), (9, 1), (94, 16)),
    32767.9: ((3, 0), (10, 0), (96, 2)),
    65535.9: ((4, 2), (14, 7), (125, 62)),
    131071.9: ((4, 0), (13, 0), (125, 2)),
    262143.9: ((394, 393), (394, 393), (396, 393)),
    -0.055: ((2, 0), (8, 0), (80, 0)),
}
# what one step adds to the clock behind the boundary that each positive start time crosses
STEP_BEHIND = {4095.9: 0.009765625, 16383.9: 0.009765625, 32767.9: 0.01171875, 65535.9: 0.0078125,
               131071.9: 0.015625, 262143.9: 0.0}
CROSSES_AT = {4095.9: 10, 16383.9: 11, 32767.9: 11, 65535.9: 9, 131071.9: 13, 262143.9: 6}  # first step behind it
STOP_T0, STOP_MAX_TIME = 16383.9, 16386.0         # a run that max_time ends inside the window
STANDING_STEPS, STANDING_MAX_TIME = 60, 262150.0  # a call on the standing clock, which max_time can never end


def clock(t0, nsteps, max_time=1e9):
    """The fp32 start times of those of the steps 0 ... nsteps - 1 from t0 that run (series_ref.gate_steps at interval
    0), and the time that the last of them leaves behind."""
    t = [f32(t) for _, t in SR.gate_steps(t0, DT, 0.0, nsteps, max_time)]
    return t + [f32(t[-1] + f32(DT))] if t else [f32(t0)]


def firing(t0, interval, nsteps=STEPS, max_time=1e9):
    """The steps of the window whose start time passes the gate at `interval`."""
    return [k for k, _ in SR.gate_steps(t0, DT, interval, nsteps, max_time)]


def consecutive(steps):
    return sum(1 for a, b in zip(steps, steps[1:]) if b == a + 1)


def steps_run(t0, nsteps, max_time):
    """How many of nsteps steps from t0 run before the clock exceeds max_time."""
    return len(SR.gate_steps(t0, DT, 0.0, nsteps, max_time))


def trail_slots(t0, interval, slots, nsteps, max_time=1e9):
    """(k, t, slot) of the steps in front of which the centroid trail records: calcCOG's (int)(t / interval) % slots with
    C's truncation and remainder, so a slot below 0 (nothing is written) comes with a quotient of -1 or less."""
    import display_ref
    return [(k, f32(t), display_ref.ring_slot(t, interval, slots)) for k, t in SR.gate_steps(t0, DT, interval, nsteps, max_time)]


def dump_due(t, interval):
    """dumpParticlebot's own test, which is not the gate: a row unless t - interval floorf(t / interval) > 0.01f."""
    t, interval = f32(t), f32(interval)
    return not bool(f32(t - f32(interval * np.floor(f32(t / interval)))) > f32(0.01))


# the lagged recorders of the late records test: the lags, the scattering's own interval (no multiple of REC: its gate
# steps are not the others'), the trail, and the shapes of the two van Hove functions, picked from the oracle's states
# (test_van_hove_shapes_hold_counts_late asserts what they are picked for).  Static friction holds most of the 300 bots
# between two records; those that move cover 0.0004 (the 90th percentile) to 0.02 in one record and up to 0.033 in seven,
# so 16 bins of 2^-9 reach 0.031.  The nearest bots are 0.11 apart, a tenth of the pairs within 0.6: 8 bins of 1/16.
RECORD_LAGS, SCAT = 8, 0.07
RECORD_TRAIL = dict(centroid_int=0.2, centroid_steps=8)
RECORD_T0 = (16383.9, 65535.9)
VAN_HOVE_SELF = (2.0 ** -9, 16)       # (width, bins), on the REC gate
VAN_HOVE_DISTINCT = (1.0 / 16, 8)     # on the SCAT gate
NEG_TRAIL = dict(centroid_int=0.02, centroid_steps=8)  # the trail of the negative clock's case
DEAD_AT = 16384.5                                      # time_to_dead of the case whose bots die late


def dead_steps(t0, time_to_dead, nsteps):
    """The steps whose start time lies in the dead-bot window [time_to_dead, time_to_dead + dt), all in fp32."""
    lo = f32(time_to_dead)
    hi = f32(lo + f32(DT))
    return [k for k, t in SR.gate_steps(t0, DT, 0.0, nsteps, 1e9) if lo <= f32(t) < hi]


def late_params(orc,n=300, seed=11, **over):
    kw = dict(nCells=n, nDead=0, seed=seed, phase_std=0.6, phase_update_interval=PUI, max_time=1e9, light_x=-2.0,
              light_y=4.0)
    kw.update(over)
    return orc.default_params(**kw)


def late_oracle(orc, P, t0):
    """The oracle placed as at time 0 and then moved to t0.  The engine sorts in its first step whatever the clock says;
    the reference would step on its all-zero cell lists until the next re-sort gate (oracle/pb_oracle.c,
    orc_sim_force_sort_once), so the oracle is told to sort once as well."""
    osim = orc.Sim(P, reset=True)
    osim.time = t0
    osim.force_sort_once()
    return osim


def bits(x):
    return int(np.asarray(x, f32).view(np.uint32))


# ---- the replay itself -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t0", STARTS)
def test_replayed_firing_counts(t0):
    got = tuple((len(g), consecutive(g)) for g in (firing(t0, iv) for iv in (PUI, SORT, REC)))
    assert got == FIRINGS[t0], (t0, got)


@pytest.mark.parametrize("t0", LATE)
def test_window_crosses_its_power_of_two_at_once_and_steps_unevenly_behind_it(t0):
    t = clock(t0, STEPS)
    assert len(t) == STEPS + 1
    boundary = f32(2.0 ** np.ceil(np.log2(t0)))
    assert t[0] < boundary and boundary in (4096, 16384, 32768, 65536, 131072, 262144)
    behind = [k for k in range(STEPS) if t[k] >= boundary]
    # within the first 12 steps; from 131071.9 (0.1015625 below 2^17 in fp32, 0.0078125 a step) it takes exactly 13
    assert behind[0] == CROSSES_AT[t0] and (behind[0] <= 12 or t0 == 131071.9) and behind[0] < MARKS[2]
    assert {float(t[k + 1] - t[k]) for k in behind} == {STEP_BEHIND[t0]}
    assert STEP_BEHIND[t0] != float(f32(DT))
    # a clock computed as t0 + k dt instead of accumulated is another float at every mark behind the boundary
    for mark in MARKS[2:]:
        assert bits(f32(f32(t0) + f32(f32(mark) * f32(DT)))) != bits(t[mark]) != bits(f32(t0 + mark * DT))
    assert len(firing(t0, PUI)) >= 1 and min(firing(t0, PUI)) < MARKS[2]  # a phase update in front of the third mark


@pytest.mark.parametrize("t0", PAIRED)
def test_phase_update_and_resort_gates_fire_on_consecutive_steps(t0):
    for iv in (PUI, SORT, REC):
        assert consecutive(firing(t0, iv)) >= 1, (t0, iv)
    # a pair of phase updates lies between two marks, so that a mark never hides one of its two draws
    g = firing(t0, PUI)
    assert any(b == a + 1 and MARKS[1] <= a and b < MARKS[3] for a, b in zip(g, g[1:]))


def test_clock_stands_still_at_two_to_the_eighteenth():
    t = clock(STANDING, STEPS)
    still = [k for k in range(STEPS) if t[k + 1] == t[k]]
    assert still and still == list(range(still[0], STEPS)) and still[0] <= 12
    assert t[-1] == f32(262144.0) and f32(t[-1] + f32(DT)) == t[-1]
    # on the standing clock every gate fires on every step, and no max_time above it ends the run
    for iv in (PUI, SORT, REC):
        assert firing(STANDING, iv)[-(STEPS - still[0]):] == still
    assert steps_run(STANDING, STANDING_STEPS, STANDING_MAX_TIME) == STANDING_STEPS
    assert clock(STANDING, STANDING_STEPS, STANDING_MAX_TIME)[-1] == f32(262144.0)
    assert len(firing(STANDING, PUI, STANDING_STEPS)) >= STANDING_STEPS - 12


def test_negative_clock_reaches_zero_inside_its_window():
    t = clock(NEGATIVE, 20)
    first = next(k for k in range(20) if t[k] >= 0)
    assert 0 < first < 12 and t[first - 1] < 0
    assert first in firing(NEGATIVE, PUI, 20)  # the first step at t >= 0 also updates the phases
    assert all(not SR.gate(t[k], PUI, DT) for k in range(first))


def test_negative_clock_has_a_dropped_trail_record_and_one_written_at_a_negative_time():
    recs = trail_slots(NEGATIVE, NEG_TRAIL["centroid_int"], NEG_TRAIL["centroid_steps"], 20)
    assert [s for _, t, s in recs if t < 0] == [-2, -1, 0]  # two records fall in front of the ring, one into slot 0
    assert [s for _, t, s in recs if t >= 0][:3] == [0, 1, 2] and len(recs) == 10


def test_late_trail_and_dump_rows_fall_on_consecutive_steps():
    for t0 in (16383.9, 65535.9):
        recs = trail_slots(t0, 0.2, 8, STEPS)
        assert any(b[0] == a[0] + 1 and a[2] == b[2] >= 0 for a, b in zip(recs, recs[1:])), t0  # a pair into one slot
        assert len({s for _, _, s in recs}) == 8                                                # and the ring wraps
    t = clock(16383.9, 300)
    due = [k for k in range(301) if dump_due(t[k], 0.5)]
    assert due == [11, 62, 113, 164, 215, 216, 267]
    assert dead_steps(16383.9, DEAD_AT, STEPS) == [62]


def test_max_time_stops_between_the_two_steps_of_a_pair():
    k = steps_run(STOP_T0, STEPS, STOP_MAX_TIME)
    assert 0 < k < STEPS
    g = firing(STOP_T0, PUI)
    assert k - 1 in g and k in g  # the last step that runs and the first that does not would both update the phases
    assert firing(STOP_T0, PUI, STEPS, STOP_MAX_TIME) == [s for s in g if s < k]
    assert clock(STOP_T0, STEPS, STOP_MAX_TIME)[-1] > f32(STOP_MAX_TIME) and len(clock(STOP_T0, STEPS, STOP_MAX_TIME)) == k + 1


# ---- the oracle against the replay -----------------------------------------------------------------------------------

@pytest.mark.parametrize("t0", STARTS)
def test_oracle_clock_and_phase_updates_follow_the_replay(orc, t0):
    want_t, want_updates = clock(t0, STEPS), firing(t0, PUI)
    osim = late_oracle(orc, late_params(orc), t0)
    assert bits(osim.time) == bits(want_t[0])
    phase, changed = osim.get("phase"), []
    for k in range(STEPS):
        assert osim.update(DT, SORT) == 0
        assert bits(osim.time) == bits(want_t[k + 1]), (t0, k, osim.time, want_t[k + 1])
        now = osim.get("phase")
        if not np.array_equal(now.view(np.uint32), phase.view(np.uint32)):
            changed.append(k)
        phase = now
    assert changed == want_updates, (t0, changed, want_updates)
    assert osim._L.orc_sim_phase_draws(osim._h) == len(want_updates)
    assert np.isfinite(osim.get("pos")).all() and np.isfinite(osim.get("vel")).all()


def test_oracle_stops_where_the_replay_says(orc):
    osim = late_oracle(orc, late_params(orc, max_time=STOP_MAX_TIME), STOP_T0)
    done = 0
    while done < STEPS and osim.update(DT, SORT) == 0:
        done += 1
    assert done == steps_run(STOP_T0, STEPS, STOP_MAX_TIME)
    assert bits(osim.time) == bits(clock(STOP_T0, STEPS, STOP_MAX_TIME)[-1])


# ---- the van Hove shapes of the late records test -------------------------------------------------------------------

def oracle_records(orc, t0, steps_wanted):
    """The oracle's (pos, rad) in front of each of the steps named, from t0 with the late records test's parameters."""
    osim = late_oracle(orc, late_params(orc, **RECORD_TRAIL), t0)
    wanted, at = set(steps_wanted), {}
    for k in range(STEPS):
        if k in wanted:
            at[k] = (osim.get("pos"), osim.get("rad"))
        assert osim.update(DT, SORT) == 0
    osim.close()
    return at


@pytest.mark.parametrize("t0", RECORD_T0)
def test_van_hove_shapes_hold_counts_late(orc, t0):
    """Both tables of the late records test, from the oracle's states at the gates' steps: counts in at least two bins
    at lag 1 and at the last lag, displacements and pairs beyond the last edge as well, and radii that stay finite (the
    distinct part counts a bot as present by them)."""
    import vanhove_distinct_ref as DR
    import vanhove_ref as VR
    rec, srec = firing(t0, REC), firing(t0, SCAT)
    assert len(rec) > RECORD_LAGS and len(srec) > RECORD_LAGS and consecutive(rec) >= 16
    at = oracle_records(orc, t0, rec + srec)
    assert all(np.isfinite(p).all() and np.isfinite(r).all() for p, r in at.values())
    self_rows = VR.table([at[k][0] for k in rec], rec, RECORD_LAGS, *VAN_HOVE_SELF)
    pair_rows = DR.table([at[k] for k in srec], srec, RECORD_LAGS, *VAN_HOVE_DISTINCT)
    for lag in (1, RECORD_LAGS - 1):
        row, pairs = self_rows[lag], pair_rows[lag]
        print(t0, lag, row["radial"], row["beyond_r"], pairs["counts"], pairs["pairs"])
        assert VR.identities_hold(row) and row["origins"] == len(rec) - lag and row["samples"] == 300 * row["origins"]
        assert sum(1 for c in row["radial"] if c) >= 2 and sum(row["radial"][1:]) > 0, (t0, lag, row)
        assert sum(1 for c in pairs["counts"] if c) >= 2 and pairs["origins"] == len(srec) - lag, (t0, lag, pairs)
        assert 0 < pairs["pairs"] < pairs["centres"] * 299  # the range leaves most pairs out
    assert self_rows[RECORD_LAGS - 1]["beyond_r"] > 0
