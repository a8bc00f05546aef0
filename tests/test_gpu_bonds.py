"""GPU: the bond recorder (pbSimSetBondDynamics / pbSimBondDynamicsRecord / pbSimGetBondDynamics, csrc/pb_bonds.hip)
against tests/bonds_ref.py on states read back from the device.  Every comparison is exact: a row holds integers only,
the 128-bit sums composed from their words.  A table recorded while stepping is compared with a twin run that has the
recorder off and is stopped in front of every step the gate names.  tests/test_bonds_api.py pins the reference to a plain
loop over sets, to its identities and to hand-built answers on the CPU, and shows that the recipe used here leaves few
bots out, breaks some bonds and reaches every k; tests/test_bonds_ref.py holds the arithmetic at its bounds, which no
state of a few seconds' size reaches.

Not run here, as in the sibling tests: the refusals that need a batch of 2^28 bots, of more than 65535 members, a ring
above 2^33 bytes and a cell with 2^31 samples: none fits a test of a few seconds.  They are comparisons in front of the
allocation in pbSimSetBondDynamics and one behind the read-back in pbSimGetBondDynamics."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bonds_ref as BR
import series_ref as SR
from helpers import assert_bit_equal
from test_bonds_api import (GAP, INSIDE_RADIUS, LAGS, MAX_RADIUS, OVERLAP, PINNED, RECORDS, SIZES, dyadic_records, rosette,
                            tie_records, walk_records)
from test_gpu_series import DT, FORMS, INTERVAL, PUI, SORT, STEPS, layout_of, make_batch, sim_with
from test_gpu_sfactor import live_memory
from test_gpu_timecorr import same_bits, twin_states
from test_series_api import CORNER, recipe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
STEP_LAGS, STEP_GAP, STEP_RADIUS, STEP_OVERLAP = 5, 0.004, 0.125, 0.015625  # while stepping
OFF = {"interval": 0.0, "lags": 0, "link_gap": 0.0, "max_radius": 0.0, "overlap_radius": 0.0, "records": 0}


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def header_constant(name):
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    return int(re.search(r"#define %s (\d+)u" % name, header).group(1))


def put(sim, pos, rad):
    n = len(pos)
    sim.set_state(pos=pos, vel=np.zeros((n, 2), f32), rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    st = sim.get_state()
    return st["pos"], st["rad"]


def record_manually(sim, records, rad, lags, gap, max_radius, overlap, also=None):
    """Sets each of `records` (positions; `rad` one array or one per record) and takes a record of it (and whatever
    `also` records of the same state); returns the member's rows and the positions and radii read back."""
    sim.set_bond_dynamics(-1.0, lags, gap, max_radius, overlap)
    assert sim.bond_dynamics_info() == {"interval": -1.0, "lags": lags, "link_gap": float(f32(gap)),
                                        "max_radius": float(f32(max_radius)), "overlap_radius": float(f32(overlap)),
                                        "records": 0}
    back, radii = [], []
    for r, pos in enumerate(records):
        p, q = put(sim, pos, rad[r] if isinstance(rad, list) else rad)
        back.append(p), radii.append(q)
        sim.bond_dynamics_record()
        if also:
            also()
    assert sim.bond_dynamics_info()["records"] == len(records)
    return sim.bond_dynamics()[0], back, radii


def fresh_sim(pb, orc, n):
    return sim_with(pb, orc, np.zeros((n, 2), f32), np.zeros((n, 2), f32), np.full(n, 0.1, f32))


def same_or_nan(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan])


# ---- manual records on set states ------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", ["origin", "corner"])
def test_manual_records_around_the_wave_and_the_workgroup(pb, orc, n, where):
    recs, rad = walk_records(n, CORNER if where == "corner" else (0.0, 0.0))
    sim = fresh_sim(pb, orc, n)
    rows, back, radii = record_manually(sim, recs, rad, LAGS, GAP, MAX_RADIUS, OVERLAP)
    for got, want in zip(back, recs):
        assert same_bits(got, want)
    want = BR.table(back, radii, [0] * RECORDS, LAGS, GAP, MAX_RADIUS, OVERLAP)
    print(n, where, rows[1])
    assert rows == want, (n, where)
    assert [r["origins"] for r in rows] == [7, 6, 5] and all(r["sum_steps"] == 0 for r in rows)
    assert [r["samples"] + r["crowded"] for r in rows] == [7 * n, 6 * n, 5 * n]  # everybody is present
    assert rows[0]["bonds_kept"] == rows[0]["bonds_then"] == rows[0]["bonds_now"] and rows[0]["plain_q2"] == 0
    if where == "origin" and n in PINNED:  # the recipe's numbers, as tests/test_bonds_api.py derives them
        one, two = rows[1], rows[2]
        assert (one["crowded"], one["bonds_kept"], one["bonds_then"], two["bonds_kept"], two["bonds_then"]) == PINNED[n]
    if n >= 64 and where == "origin":
        assert all(c > 0 for c in rows[1]["cage_samples"])  # every k from 1 to 8
    sim.close()


@pytest.mark.parametrize("n", SIZES)
def test_manual_records_with_bots_above_the_largest_radius(pb, orc, n):
    recs, rad = walk_records(n, (1.5, -2.25))
    sim = fresh_sim(pb, orc, n)
    rows, back, radii = record_manually(sim, recs, rad, LAGS, GAP, INSIDE_RADIUS, OVERLAP)
    want = BR.table(back, radii, [0] * RECORDS, LAGS, GAP, INSIDE_RADIUS, OVERLAP)
    assert rows == want, n
    here = int((rad <= f32(INSIDE_RADIUS)).sum())
    assert [r["samples"] + r["crowded"] for r in rows] == [7 * here, 6 * here, 5 * here]
    if n >= 63:
        assert 0 < here < n and 0 < rows[1]["bonds_kept"] < rows[1]["bonds_then"]
    sim.close()


def test_more_bots_than_one_pass_covers(pb, orc):
    n = header_constant("PB_BOND_BLOCKS") * 256 + 321  # the block loop runs twice for 321 lanes
    assert n == 65857
    recs, rad = walk_records(n, (-300.0, 700.0), records=3)
    sim = fresh_sim(pb, orc, n)
    rows, back, radii = record_manually(sim, recs, rad, 2, GAP, MAX_RADIUS, OVERLAP)
    assert rows == BR.table(back, radii, [0] * 3, 2, GAP, MAX_RADIUS, OVERLAP)
    assert [r["samples"] + r["crowded"] for r in rows] == [3 * n, 2 * n] and 0 < rows[1]["bonds_kept"] < rows[1]["bonds_then"]
    assert all(c > 0 for c in rows[1]["cage_samples"]) and rows[1]["crowded"] > 0
    sim.close()


def test_batch_of_members_with_different_states(pb, orc):
    n = 257
    ens = make_batch(pb, orc, 4, n)
    states = []
    for k in range(4):
        recs, rad = walk_records(n, (3.0 * k - 1.0, -2.0 * k), records=4, seed=9200 + k)
        if k == 1:  # no links: the blob spread out tenfold
            recs = [(p * f32(10.0)).astype(f32) for p in recs]
        if k == 2:  # NaN, infinite and out-of-range bots, and a radius that is not finite, each in some records only
            recs[1][3, 0] = np.nan
            recs[2][3, 0] = np.nan
            recs[2][40, 1] = np.inf
            recs[0][77] = 2048.0, 0.0
            recs[3][200] = -5000.0, 3.0
            rad = [rad.copy() for _ in range(4)]
            rad[1][100], rad[2][101], rad[3][102] = np.nan, np.inf, -np.inf
        if k == 3:  # wholly absent: every radius above the largest
            rad = (rad + f32(0.1)).astype(f32)
        states.append((recs, rad))
    ens.set_bond_dynamics(-1.0, 3, GAP, MAX_RADIUS, OVERLAP)
    back = [([], []) for _ in range(4)]
    for r in range(4):
        for k, (recs, rad) in enumerate(states):
            ens.set_state_of(k, pos=recs[r], rad=rad[r] if isinstance(rad, list) else rad)
            st = ens.get_state_of(k)
            assert same_or_nan(st["pos"], recs[r])
            back[k][0].append(st["pos"]), back[k][1].append(st["rad"])
        ens.bond_dynamics_record()
    rows = ens.bond_dynamics()
    assert len(rows) == 4 and all(len(r) == 3 for r in rows)
    for k in range(4):
        assert rows[k] == BR.table(back[k][0], back[k][1], [0] * 4, 3, GAP, MAX_RADIUS, OVERLAP), k
    assert rows[0][1]["bonds_kept"] > 0 and sum(rows[0][1]["cage_samples"]) > 0
    assert [r["samples"] for r in rows[1]] == [4 * n, 3 * n, 2 * n] and all(r["bonds_then"] == r["bonds_now"] == 0 for r in rows[1])
    assert rows[2][0]["samples"] + rows[2][0]["crowded"] == 4 * n - 8  # record 0: 1 absent, 1: 2, 2: 3, 3: 2
    assert rows[3] == [dict(BR.empty_row(l), origins=4 - l) for l in range(3)]
    assert ens.bond_dynamics() == rows  # twice: the same rows
    lone = fresh_sim(pb, orc, n)
    alone, _, _ = record_manually(lone, states[2][0], states[2][1], 3, GAP, MAX_RADIUS, OVERLAP)
    assert alone == rows[2]
    lone.close()
    ens.close()


def test_the_rosettes_the_largest_radius_and_a_lost_neighbour(pb, orc):
    for discs in (8, 9):
        pos, rad = rosette(discs)
        sim = fresh_sim(pb, orc, discs + 1)
        rows, back, radii = record_manually(sim, [pos, pos], rad, 2, 0.001, 0.3, 0.01)
        assert rows == BR.table(back, radii, [0, 0], 2, 0.001, 0.3, 0.01)
        assert rows[1]["crowded"] == (discs == 9) and rows[1]["cage_samples"] == [discs, 0, 0, 0, 0, 0, 0, int(discs == 8)]
        if discs == 8:
            below = float(np.nextafter(f32(0.3), f32(0.0)))  # the large disc is one step above it: absent
            rows, back, radii = record_manually(sim, [pos, pos], rad, 2, 0.001, below, 0.01)
            assert rows == BR.table(back, radii, [0, 0], 2, 0.001, below, 0.01)
            assert (rows[1]["samples"], rows[1]["bonds_then"]) == (8, 0)
            lost = pos.copy()
            lost[3, 0] = np.nan  # a neighbour that turns NaN uncages the large disc
            rows, back, radii = record_manually(sim, [pos, lost], rad, 2, 0.001, 0.3, 0.01)
            assert rows == BR.table(back, radii, [0, 0], 2, 0.001, 0.3, 0.01)
            assert rows[1]["cage_samples"] == [7, 0, 0, 0, 0, 0, 0, 0] and rows[1]["bonds_kept"] == 14
            far = pos.copy()
            far[0, 0] = 300.0  # 8 x 300 x 2^20 is past 2^31: sampled, not caged; the discs around it are, at k = 1
            rows, back, radii = record_manually(sim, [pos, far], rad, 2, 0.001, 0.3, 0.01)
            assert rows == BR.table(back, radii, [0, 0], 2, 0.001, 0.3, 0.01)
            assert rows[1]["samples"] == 9 and rows[1]["cage_samples"] == [8] + [0] * 7
            assert rows[1]["cage_q2"][0] == 8 * (300 << 20) ** 2 and rows[1]["plain_q2"] == 0
        sim.close()


def test_a_rigid_shift_and_the_tie(pb, orc):
    recs, rad, moved = dyadic_records()
    sim = fresh_sim(pb, orc, len(rad))
    rows, back, radii = record_manually(sim, recs, rad, 4, GAP, MAX_RADIUS, OVERLAP)
    for got, want in zip(back, recs):
        assert same_bits(got, want)
    assert rows == BR.table(back, radii, [0] * 4, 4, GAP, MAX_RADIUS, OVERLAP)
    caged = sum(rows[0]["cage_samples"]) // 4
    for l, row in enumerate(rows):
        assert row["bonds_kept"] == row["bonds_then"] > 0 and row["cage_q2"] == [0] * 8
    assert rows[3]["plain_q2"] == caged * ((moved[2][0]) ** 2 + (moved[2][1]) ** 2) > 0
    sim.close()
    recs, rad = tie_records(OVERLAP)
    sim = fresh_sim(pb, orc, 2)
    tie, back, radii = record_manually(sim, recs, rad, 2, GAP, MAX_RADIUS, OVERLAP)
    assert tie == BR.table(back, radii, [0, 0], 2, GAP, MAX_RADIUS, OVERLAP)
    more, _, _ = record_manually(sim, recs, rad, 2, GAP, MAX_RADIUS, OVERLAP + 2.0 ** -20)
    assert tie[1]["cage_samples"][0] == 2 and tie[1]["cage_overlap"][0] == 0 and more[1]["cage_overlap"][0] == 2
    assert more[1]["cage_q2"] == tie[1]["cage_q2"] == [2 * BR.qa_of(OVERLAP) ** 2] + [0] * 7
    sim.close()


def test_lag_one_bond_columns_are_the_devices_own_mark_and_compare(pb, orc):
    recs, rad = walk_records(64, records=2)
    sim = fresh_sim(pb, orc, 64)
    put(sim, recs[0], rad)
    sim.mark_reference(GAP)
    put(sim, recs[1], rad)
    marked = sim.rearrangement()[0]
    rows, _, _ = record_manually(sim, recs, rad, 2, GAP, MAX_RADIUS, OVERLAP)
    one = rows[1]
    assert one["crowded"] == 0 and one["samples"] == 64
    assert ([one[k] for k in ("bonds_then", "bonds_now", "bonds_kept", "bots_unchanged", "bots_lost", "bots_gained")] ==
            [marked[k] for k in ("bonds_marked", "bonds_now", "bonds_kept", "bots_unchanged", "bots_lost", "bots_gained")])
    assert one["plain_q2"] <= marked["sum_q2"]  # (the caged bots are some of the measured ones; the grid is exact)
    sim.close()


# ---- recorded while stepping -----------------------------------------------------------------------------------------

WIDTH, BINS, BOX = 0.03125, 16, 3


def stepping_sim(pb, orc, form, wave=True):
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0 if wave else 1, phase_update_interval=PUI,
                   centroid_steps=16, centroid_int=0.1)
    sim.set_resident(form["resident"])
    if "lanes" in form:
        sim.set_lanes_per_bot(form["lanes"])
    return sim


@pytest.mark.parametrize("name", list(FORMS))
def test_recorded_table_equals_a_twin_and_leaves_the_run_alone(pb, orc, name):
    form = FORMS[name]
    interval, steps = (0.0, 120) if name == "every_step" else (INTERVAL, STEPS)
    gates = SR.gate_steps(0.0, DT, interval, steps, 1e9)
    rec = [k for k, _ in gates]
    assert len(rec) > STEP_LAGS  # the ring wraps
    # a: the recorder on; b: the twin, stepped in pieces; d: set and switched off again; e: never set; c: the time
    # correlation alone at that interval, whose gate the recorder shares
    a, b, d, e, c = (stepping_sim(pb, orc, form) for _ in range(5))
    c.set_time_correlation(interval, STEP_LAGS, STEP_OVERLAP)
    a.set_bond_dynamics(interval, STEP_LAGS, STEP_GAP, STEP_RADIUS, STEP_OVERLAP)
    d.set_bond_dynamics(interval, STEP_LAGS, STEP_GAP, STEP_RADIUS, STEP_OVERLAP)
    d.set_bond_dynamics(interval, 0, 0.0, 0.0, 0.0)
    assert d.bond_dynamics_info() == OFF
    for s in (a, d, e, c):
        assert s.step(steps, dt=DT, sort_interval=SORT) == steps  # one call
    assert a.bond_dynamics_info()["records"] == len(rec)
    got = a.bond_dynamics()[0]
    radii = []

    def state_of():
        st = b.get_state()
        radii.append(st["rad"])
        return [st]
    states = twin_states(b, gates, steps, state_of=state_of)[0]
    want = BR.table([p for p, _ in states], radii, rec, STEP_LAGS, STEP_GAP, STEP_RADIUS, STEP_OVERLAP)
    print(name, got[1], got[STEP_LAGS - 1])
    assert got == want, name
    assert [g["origins"] for g in got] == [len(rec) - l for l in range(STEP_LAGS)]
    assert got[1]["samples"] > 0 and got[1]["bonds_then"] > 0 and sum(got[STEP_LAGS - 1]["cage_samples"]) > 0
    # the final state and the counters are the twin's, with the recorder on, off and never set
    sb = b.get_state()
    for s in (a, d, e, c):
        st = s.get_state()
        for k in sb:
            assert_bit_equal(st[k], sb[k], f"{name} {k}")
        assert s.time == b.time
    # switched off it is as if never set; switched on, the launches are those of any recorder at that interval
    assert d.stats() == e.stats() and a.stats() == c.stats()
    for key in ("steps", "resorts", "phase_updates"):
        assert a.stats()[key] == e.stats()[key], key
    n, ms = a.bond_dynamics_times()
    assert n == len(rec) and ms > 0.0
    for s in (a, b, d, e, c):
        s.close()


def test_the_other_recorders_the_mark_and_the_analyses_are_left_alone(pb, orc):
    form, steps = FORMS["fused"], STEPS
    vectors = pb.half_plane_vectors(3)
    switches = {
        "series": lambda s: s.set_series(INTERVAL, 512),
        "time_correlation": lambda s: s.set_time_correlation(INTERVAL, STEP_LAGS, STEP_OVERLAP),
        "scattering": lambda s: s.set_scattering(INTERVAL, STEP_LAGS, BOX, vectors),
        "van_hove": lambda s: s.set_van_hove(INTERVAL, STEP_LAGS, WIDTH, BINS),
        "van_hove_distinct": lambda s: s.set_van_hove_distinct(INTERVAL, STEP_LAGS, WIDTH, BINS),
        "coherent_scattering": lambda s: s.set_coherent_scattering(INTERVAL, STEP_LAGS, BOX, vectors),
        "four_point": lambda s: s.set_four_point(INTERVAL, STEP_LAGS, STEP_OVERLAP, BOX, vectors),
    }
    read = lambda s, name: s.series_of(0) if name == "series" else getattr(s, name)()
    sims = []
    for bonds in (True, False):
        s = stepping_sim(pb, orc, form)
        s.set_centroid_trail(True)
        s.mark_reference(STEP_GAP)
        for on in switches.values():
            on(s)
        if bonds:
            s.set_bond_dynamics(INTERVAL, STEP_LAGS, STEP_GAP, STEP_RADIUS, STEP_OVERLAP)
        assert s.step(steps, dt=DT, sort_interval=SORT) == steps
        sims.append(s)
    with_bonds, without = sims
    for name in switches:
        assert read(with_bonds, name) == read(without, name), name
    assert with_bonds.rearrangement() == without.rearrangement()
    assert with_bonds.reference_info() == without.reference_info()
    a, b = with_bonds.get_state(), without.get_state()
    for k in a:
        assert_bit_equal(a[k], b[k], k)
    assert with_bonds.bond_dynamics_info()["records"] == with_bonds.four_point_info()["records"] == len(with_bonds.series_of(0))
    # a bond record between two on-demand analyses does not change their answers
    first = (with_bonds.clusters(STEP_GAP), with_bonds.rearrangement(), with_bonds.structure(STEP_GAP))
    with_bonds.bond_dynamics_record()
    assert (with_bonds.clusters(STEP_GAP), with_bonds.rearrangement(), with_bonds.structure(STEP_GAP)) == first
    with_bonds.bond_dynamics_record()
    assert with_bonds.rearrangement() == first[1] == without.rearrangement()
    for s in sims:
        s.close()


def test_reading_and_recording_change_nothing(pb, orc):
    pos, vel, rad = recipe(300)
    sim = sim_with(pb, orc, pos, vel, rad, phase_update_interval=0.3)
    sim.set_time_correlation(0.1, 3, 0.5)
    sim.set_bond_dynamics(-1.0, 3, STEP_GAP, STEP_RADIUS, STEP_OVERLAP)
    assert sim.step(60, dt=DT, sort_interval=0.2) == 60
    assert sim.bond_dynamics_info()["records"] == 0  # manual only
    before, stats, lay, t = sim.get_state(), sim.stats(), layout_of(sim), sim.time
    assert lay[2] == 1 and not np.array_equal(lay[0], np.arange(300))  # sorted: the slots are not in original order
    corr = sim.time_correlation()
    sim.bond_dynamics_record()
    sim.bond_dynamics_record()
    first = sim.bond_dynamics()
    assert first == sim.bond_dynamics()
    assert first[0] == BR.table([before["pos"]] * 2, before["rad"], [60, 60], 3, STEP_GAP, STEP_RADIUS, STEP_OVERLAP)
    after = sim.get_state()
    for k in before:
        assert_bit_equal(before[k], after[k], k)
    assert sim.stats() == stats and sim.time == t and sim.time_correlation() == corr
    for x, y in zip(lay, layout_of(sim)):
        assert np.array_equal(x, y)
    # a later step and a set_state leave the ring alone: the next record pairs with the two it holds
    assert sim.step(7, dt=DT, sort_interval=0.2) == 7
    now = sim.get_state()
    sim.set_state(pos=now["pos"], vel=now["vel"], rad=now["rad"], phase=now["phase"], dead=now["dead"])
    sim.bond_dynamics_record()
    assert sim.bond_dynamics()[0] == BR.table([before["pos"]] * 2 + [now["pos"]], [before["rad"]] * 2 + [now["rad"]],
                                              [60, 60, 67], 3, STEP_GAP, STEP_RADIUS, STEP_OVERLAP)
    assert sim.bond_dynamics_times()[0] == 3 and sim.bond_dynamics_times()[1] > 0.0
    sim.close()


# ---- life cycle --------------------------------------------------------------------------------------------------------

def test_restart_switch_off_and_argument_errors(pb, orc):
    pos, vel, rad = recipe(300)
    a = sim_with(pb, orc, pos, vel, rad, wall_half=64.0, control=0, phase_update_interval=PUI)
    a.set_resident(1)
    assert a.bond_dynamics_info() == OFF and a.bond_dynamics_times() == (0, 0.0)
    for call in (a.bond_dynamics_record, a.bond_dynamics):
        with pytest.raises(RuntimeError, match="code 2.*the bond recorder is off"):
            call()
    for bad, word in (((-0.5, 4, 0.0, 0.1, 0.05), "interval"), ((float("nan"), 4, 0.0, 0.1, 0.05), "interval"),
                      ((0.0, 65, 0.0, 0.1, 0.05), "lags"), ((0.0, 4, -0.5, 0.1, 0.05), "linkGap"),
                      ((0.0, 4, float("inf"), 0.1, 0.05), "linkGap"), ((0.0, 4, 0.0, 0.0, 0.05), "maxRadius"),
                      ((0.0, 4, 0.0, float("nan"), 0.05), "maxRadius"), ((0.0, 4, 48.0, 1000.0, 0.05), "2 maxRadius"),
                      ((0.0, 4, 0.0, 0.1, 256.0), "overlapRadius"), ((0.0, 4, 0.0, 0.1, -1.0), "overlapRadius")):
        with pytest.raises(RuntimeError, match="code 2.*pbSimSetBondDynamics.*" + word):
            a.set_bond_dynamics(*bad)
    assert a.bond_dynamics_info() == OFF
    a.clusters(0.0)  # the analysis layer's scratch is made: from here on the recorder's own memory is counted
    made = live_memory()
    a.set_bond_dynamics(0.0, 4, STEP_GAP, STEP_RADIUS, STEP_OVERLAP)
    # the ring of heads, the lists beside it and the cells
    assert live_memory() == (made[0] + 3, made[1] + 4 * 300 * 48 + 4 * 42 * 8)
    assert a.step(20, dt=DT, sort_interval=SORT) == 20 and a.bond_dynamics_info()["records"] == 20
    assert live_memory() == (made[0] + 3, made[1] + 4 * 300 * 48 + 4 * 42 * 8)  # no record allocates
    rows = a.bond_dynamics()[0]
    assert [r["origins"] for r in rows] == [20, 19, 18, 17] and [r["sum_steps"] for r in rows] == [0, 19, 36, 51]
    # again: restarts at record 0 with a zeroed table
    a.set_bond_dynamics(0.05, 64, 0.0, 0.25, 0.0)
    assert a.bond_dynamics_info() == {"interval": float(f32(0.05)), "lags": 64, "link_gap": 0.0, "max_radius": 0.25,
                                      "overlap_radius": 0.0, "records": 0}
    assert a.bond_dynamics()[0] == [BR.empty_row(l) for l in range(64)]
    gates = SR.gate_steps(a.time, DT, 0.05, 30, 1e9)
    assert a.step(30, dt=DT, sort_interval=SORT) == 30
    rows = a.bond_dynamics()[0]
    assert a.bond_dynamics_info()["records"] == len(gates) and 5 <= len(gates) <= 7
    assert [r["origins"] for r in rows] == [max(len(gates) - l, 0) for l in range(64)]
    # lags 0 frees: the memory is back, later steps record nothing and are fused again
    a.set_bond_dynamics(0.05, 0, 0.0, 0.0, 0.0)
    assert a.bond_dynamics_info() == OFF and live_memory() == made
    stats = a.stats()
    assert a.step(30, dt=DT, sort_interval=SORT) == 30 and a.bond_dynamics_info() == OFF
    assert a.stats()["fused_launches"] == stats["fused_launches"] + 29  # every step but the call's last is fused again
    with pytest.raises(RuntimeError, match="code 2.*the bond recorder is off"):
        a.bond_dynamics()
    with pytest.raises(RuntimeError, match="code 2.*the bond recorder is off"):
        a.bond_dynamics_record()
    assert a.bond_dynamics_times() == (0, 0.0)
    a.close()
    # switched on first in a fresh batch, the call makes the filing's scratch too; destroyed with the ring live
    start = live_memory()
    b = sim_with(pb, orc, pos, vel, rad)
    b.set_bond_dynamics(-1.0, 2, 0.0, 0.25, 0.0)
    b.bond_dynamics_record()
    held = live_memory()
    b.bond_dynamics_record()
    assert live_memory() == held
    b.close()
    assert live_memory() == start


def test_legacy_engine_refuses(capfd):
    from particlerobotsimulations_amd import host
    h = host.HostSim(CFG, engine="legacy")
    capfd.readouterr()
    lib = host.lib()
    assert lib.pbHostSetBondDynamics(h._h, -1.0, 2, 0.0, 0.25, 0.05) == -1
    assert capfd.readouterr() == ("", "Particlebot::setBondDynamics: the bond recorder needs the fused engine\n")
    assert lib.pbHostBondDynamicsRecord(h._h) == -1
    assert capfd.readouterr() == ("", "Particlebot::bondDynamicsRecord: the bond recorder needs the fused engine\n")
    h.close()


# ---- the runner ------------------------------------------------------------------------------------------------------

COLUMNS = ("lag", "origins", "sum_steps", "samples", "crowded", "bonds_then", "bonds_now", "bonds_kept", "bots_unchanged",
           "bots_lost", "bots_gained", "plain_q2")
HEADER = ("Lag, Origins, SumSteps, Samples, Crowded, BondsThen, BondsNow, BondsKept, BotsUnchanged, BotsLost, BotsGained, "
          "PlainQ2, " + ", ".join(c + str(k) for c in ("CageSamples", "CageOverlap", "CageQ2") for k in range(1, 9)) +
          ", BondSurvival, FractionLost, CageMsd, PlainMsd, CageOverlap")


def test_runner_writes_the_table_at_the_end_of_the_run(tmp_path):
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import _analysis, _capi, host
    over = dict(max_time="30", dump_interval="2.5")
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--bonds", "b.csv", "--bonds-lags", "4", "--bonds-gap", "0.01",
                                                      "--bonds-overlap", "0.05"],
                       capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "b.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 4
    cells = [l.split(", ") for l in lines[1:]]
    assert all(len(c) == 12 + 24 + 5 for c in cells)
    assert [int(c[0]) for c in cells] == [0, 1, 2, 3] and [int(c[1]) for c in cells] == [12, 11, 10, 9]
    # the same rows from the class driven in-process through the host library's wrappers, with the runner's defaults
    flat = host.load_config(CFG, **over)
    h = host.HostSim(CFG, engine="fused", **over)
    lib = host.lib()
    assert lib.pbHostSetBondDynamics(h._h, flat.dump_interval, 4, 0.01, flat.max_radius, 0.05) == 0

    def info():
        return _analysis.read_info(_analysis.BOND_DYNAMICS_INFO, lambda *q: lib.pbHostBondDynamicsInfo(h._h, *q))
    assert info() == {"interval": float(f32(flat.dump_interval)), "lags": 4, "link_gap": float(f32(0.01)),
                      "max_radius": float(f32(flat.max_radius)), "overlap_radius": float(f32(0.05)), "records": 0}
    while not h.finished:
        if h.advance(h.steps_until_dump()) == 0:
            break
    rows, count = (_capi.pbBondRow * 4)(), C.c_ulonglong(0)
    assert lib.pbHostBondDynamicsRows(h._h, rows, 3, C.byref(count)) == -1 and count.value == 4  # too little room
    assert lib.pbHostBondDynamicsRows(h._h, rows, 4, C.byref(count)) == 0 and count.value == 4
    want = [_capi.bond_row(r) for r in rows]
    for c, w in zip(cells, want):
        assert c[:12] == [str(w[k]) for k in COLUMNS]
        assert c[12:36] == [str(v) for k in ("cage_samples", "cage_overlap", "cage_q2") for v in w[k]]
        s = pb.bond_dynamics_summary(w)
        for text, key in zip(c[36:], ("bond_survival", "fraction_lost", "cage_msd", "plain_msd", "cage_overlap")):
            if s[key] is None:
                assert text == "nan"
            else:
                assert float(text) == pytest.approx(s[key], rel=1e-6, abs=1e-12), (key, text, s)  # (long double against an exact fraction)
    assert want[1]["samples"] > 0 and want[1]["bonds_then"] > 0
    assert info()["records"] == 12
    assert lib.pbHostBondDynamicsRecord(h._h) == 0 and info()["records"] == 13
    assert lib.pbHostSetBondDynamics(h._h, 0.0, 0, 0.0, 0.0, 0.0) == 0 and info()["lags"] == 0  # off
    assert lib.pbHostBondDynamicsRecord(h._h) == -1
    h.close()
    # the defaults: 32 lags
    r = subprocess.run([RUN, CFG, "--quiet"] + sets + ["--bonds", "g.csv"], capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "g.csv").read().splitlines()
    assert lines[0] == HEADER and len(lines) == 1 + 32
