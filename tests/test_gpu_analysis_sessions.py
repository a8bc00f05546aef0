"""GPU: the analysis layer as one session.  A batch handle serves every analysis from one scratch object
(PbClusterScratch, csrc/pb_cluster.hpp) and a few private buffers, and every entry point re-files the bots on a grid of
its own; the other GPU test files call each analysis on a fresh session, in one order.  Here the catalogue of
tests/analysis_session_cases.py (60 named calls: every gap, bin count, map, vector list and frame shape at its largest
and then at its smallest, three reads of the rearrangement mark, two entries that replace it, and the strain analysis,
which files nothing and reads the mark's buffers, at three thresholds and per member) runs on ONE handle in six orders
on each of three states, and every result must equal both the restatement's expectation and the result of the same call
made alone on a fresh session brought to the state by the same recipe, bit for bit.  The same holds with a record of
the distinct van Hove function between every two calls: the recorder files the bots itself, on a grid no call of the
catalogue uses, and its table is that of a twin which made no analysis call.  Around the calls nothing of the engine's
state moves, the six recorders' rings and tables stay what a run without analyses leaves, the run counters and the
device memory held depend on the calls made and not on their order, and a refused call leaves the session usable.

tests/test_analysis_session_cases_ref.py proves without a device that the orders hold every grow-then-shrink, both
switches of the filing kind, a mark read behind five other families' re-filings (by a compare and by a strain call), a
strain call directly behind every family that re-files, behind a re-mark, a compare and a displacement correlation, and
a compare directly behind a strain call; and that the records' grid is no call's.

Measured on one MI355X, this file run alone: 30 tests in 9.2 s.  The slowest case is batch3x300-catalogue with 1.7 s: it
computes the state's expectations and makes its 84 fresh sessions; the next state's first case takes 1.2 s, single17's
0.6 s.  A case with records takes 0.3 s (catalogue: 59 records) or 0.5 s (a doubled shuffle: 119 records, and the
reference's table of 119 records of one member), every other case and test 0.03 ... 0.35 s (a doubled shuffle of 120
calls with both comparisons: 0.2 s).

Changes tried on a copy of the tree.  Earlier, on the catalogue of 54 calls: without the memset of sCounts in
pbSimRadialCounts all 18 cases of test_every_order fail (a fresh buffer holds no zeros), and so do 18 tests of the
per-analysis files, which call radial_counts twice on one handle.  With pbSimPairCorrelation skipping its filing at an
unchanged rMax, catalogue and reversed pass and 9 shuffles fail (batch3x300-shuffle1, every shuffle of the two other
states: a link grid of one cell hides it, which is what batch3x300_small_radii is there for); one per-analysis test
notices too (test_gpu_correlation's shared-scratch test).  With the rearrangement compare filing on the grid edge of
the analysis before it, batch3x300-catalogue, -shuffle0 and -shuffle1 fail and the per-analysis files stay green.
On this catalogue, each run on one MI355X:
  1. The hexatic sweep skips its filing when its gap is the one it last filed with.  The record test fails at
     batch3x300-shuffle1 (structure(0.0019) and structure(0.05) sweep the record's grid), and so do batch3x300-shuffle1
     and -shuffle2 of test_every_order; 27 of 30 pass, and test_gpu_structure, test_gpu_link_consumers and
     test_gpu_vanhove_distinct stay green.  Only batch3x300 can see it: there the link grid is one cell of edge 4100
     and the record's cells of edge 1 are too fine for it, whereas on the two other states the record's grid is coarser
     than the link rule needs and a sweep of it still meets every neighbour.  The catalogue order never repeats a gap
     in two consecutive hexatic calls, so it cannot take the skip at all.
  2. strainSweep without the memset of tRows.  All 18 cases of test_every_order, all 6 cases with records and the
     refused-call test fail, from the second strain call of a session on; 17 of 20 tests of test_gpu_strain fail too.
  3. pbSimMarkReference leaves the old entries of dOther in place when the new mark needs no more of them.  17 cases of
     test_every_order (all but batch3x300-reversed), all 6 cases with records and the refused-call test fail: the
     compare of the replacing entry and the strain reads under mark C, the one directly behind the re-mark among them
     (batch3x300-shuffle2 #48).  test_gpu_strain and test_gpu_dynamics stay green."""
import numpy as np
import pytest

import analysis_session_cases as AC
import geometry_cases as gc
import vanhove_distinct_ref as GR
from helpers import assert_bit_equal
from test_gpu_field import live_memory
from test_gpu_series import layout_of

pytestmark = pytest.mark.gpu

f32 = np.float32
STATE_KEYS = ("pos", "vel", "rad", "phase", "dead")
COUNTERS = ("cluster_times", "contact_times", "structure_times", "rearrangement_times", "correlation_times",
            "field_times", "structure_factor_times", "series_times", "time_correlation_times", "scattering_times",
            "render_stats", "strain_times", "van_hove_times", "van_hove_distinct_times")
VEC3 = [[1, 0], [-3, 2], [7, 5]]


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def assert_is_the_state(sim, st):
    """The device's state is the recipe's, bit for bit; on the stepped batch the slots are out of original order and the
    engine's cell lists are stale."""
    for m in range(st.nsims):
        got = AC.state_of(sim, m)
        for key in STATE_KEYS:
            assert_bit_equal(got[key], st.final[m][key], f"{st.name} member {m} {key}")
    assert sim.time == float(f32(st.time))
    if st.nsims == 3:
        from oracle import orclib as orc
        assert sim.stats()["resorts"] >= 2
        for m in range(st.nsims):
            orig, keys, is_sorted = layout_of(sim, m)
            assert is_sorted == 1 and not np.array_equal(orig, np.arange(st.n)), m
            P = st.params[m]
            cx, cy = gc.cells(orc, P, np.nan_to_num(st.final[m]["pos"][orig], nan=0.0, posinf=0.0, neginf=0.0))
            finite = np.isfinite(st.final[m]["pos"][orig]).all(axis=1)
            left = (cy * int(P.gridSizeX) + cx != keys) & finite  # bots that left the cell they are filed under
            assert left.sum() >= 3, m


def fresh_answer(pb, st, entry, mark):
    """The entry's result as the first analysis of a fresh session (behind the mark it reads, if that is not the
    recipe's)."""
    sim = AC.bring(pb, st)
    try:
        if entry.reads_mark and not entry.sets_mark and mark != "A":
            sim.mark_reference(AC.MARKS[mark])
        return entry.norm(entry.call(sim))
    finally:
        sim.close()


@pytest.fixture(scope="module")
def fresh(pb):
    """name of a state -> {(catalogue index, mark): the fresh session's answer}, built once per state."""
    built = {}

    def answers(name):
        if name not in built:
            st = AC.state(name)
            entries = AC.catalogue(st)
            built[name] = {(i, mark): fresh_answer(pb, st, entries[i], mark) for i, mark in AC.needed(st)}
        return built[name]

    return answers


def run_checked(st, sim, order, answers, what, mark="A", between=None):
    """Every call of the order on `sim`: the failures, each naming the call, its place and the call in front of it.
    between() is called between every two calls."""
    index = {e.name: i for i, e in enumerate(AC.catalogue(st))}
    failures, previous = [], "the recipe"
    for place, (e, mark_now) in enumerate(AC.walk(st, order, mark)):
        if between and place:
            between()
        got = e.norm(e.call(sim))
        where = f"{what} #{place} {e.name} [mark {mark_now}] behind {previous}"
        try:
            e.check(got, AC.expected(st, e, mark_now))
        except AssertionError as err:
            failures.append(f"{where}: not the restatement's: {str(err)[:300]}")
        if not AC.same_bits(got, answers[index[e.name], mark_now if e.reads_mark else None]):
            failures.append(f"{where}: not the fresh session's")
        previous = e.name
    return failures


def run_plain(st, sim, order):
    for e, _ in AC.walk(st, order):
        e.call(sim)


# ---- 1. every order, one answer --------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", AC.ORDERS)
@pytest.mark.parametrize("name", AC.ALL_STATES)
def test_every_order_gives_the_answers_of_a_fresh_session(pb, fresh, name, order):
    st = AC.state(name)
    answers = fresh(name)
    sim = AC.bring(pb, st)
    try:
        assert_is_the_state(sim, st)
        failures = run_checked(st, sim, AC.orders(st)[order], answers, f"{name} {order}")
        assert not failures, (len(failures), failures[:12])
        assert_is_the_state(sim, st)
    finally:
        sim.close()


# ---- 1b. a record of the distinct van Hove function between any two calls ------------------------------------------------

_REPEATED = {}


def repeated_table(st, member, records):
    """vanhove_distinct_ref's table of `records` records of the member's state as it is, computed once."""
    key = (st.name, member, records)
    if key not in _REPEATED:
        s = st.final[member]
        steps = AC.STEPS if st.nsims == 3 else 0
        _REPEATED[key] = GR.table([(s["pos"], s["rad"])] * records, [steps] * records, *AC.RECORD_BETWEEN)
    return _REPEATED[key]


@pytest.mark.parametrize("order", ["catalogue", "shuffle1"])
@pytest.mark.parametrize("name", AC.ALL_STATES)
def test_a_distinct_record_between_any_two_calls_changes_no_answer(pb, fresh, name, order):
    """The recorder files the bots itself, at rMax = 1 with perRmax = 0, on the scratch the analyses share: a call that
    trusted the grid, the cell starts or the filed copies of the call in front of it would meet the record's."""
    st = AC.state(name)
    answers = fresh(name)
    calls = AC.orders(st)[order]
    lags, width, bins = AC.RECORD_BETWEEN
    _, _, odd = AC.members_of(st)
    sim, twin = AC.bring(pb, st), AC.bring(pb, st, mark=False)
    try:
        for s in (sim, twin):
            s.set_van_hove_distinct(-1.0, lags, width, bins)  # manual records only
        assert_is_the_state(sim, st)
        failures = run_checked(st, sim, calls, answers, f"{name} {order} with records", between=sim.van_hove_distinct_record)
        assert not failures, (len(failures), failures[:12])
        assert_is_the_state(sim, st)
        records = len(calls) - 1
        for _ in range(records):  # the twin: the same records, no analysis call, not even the recipe's mark
            twin.van_hove_distinct_record()
        assert sim.van_hove_distinct_info() == twin.van_hove_distinct_info()
        assert sim.van_hove_distinct_info() == {"interval": -1.0, "lags": lags, "width": width, "bins": bins,
                                                "records": records}
        assert sim.van_hove_distinct_times()[0] == records and twin.strain_times()[0] == twin.cluster_times()[0] == 0
        got, alone = sim.van_hove_distinct(), twin.van_hove_distinct()
        assert AC.same_bits(got, alone)
        assert got[odd] == repeated_table(st, odd, records)
        for m, rows in enumerate(got):
            assert [r["origins"] for r in rows] == [records, records - 1], m
            assert rows[1]["pairs"] > 0 and sum(1 for c in rows[1]["counts"] if c) > 1, (m, rows[1])
    finally:
        sim.close()
        twin.close()


# ---- 2. nothing changes ------------------------------------------------------------------------------------------------

def engine_side(sim, st):
    return {"states": [AC.state_of(sim, m) for m in range(st.nsims)],
            "layouts": [layout_of(sim, m) for m in range(st.nsims)],
            "stats": sim.stats(), "time": sim.time, "phase_draws": sim.phase_draws}


def assert_same_engine_side(a, b, what):
    for m, (sa, sb) in enumerate(zip(a["states"], b["states"])):
        for key in sa:
            assert_bit_equal(sa[key], sb[key], f"{what} member {m} {key}")
    for m, (la, lb) in enumerate(zip(a["layouts"], b["layouts"])):
        assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]) and la[2] == lb[2], (what, m)
    assert a["stats"] == b["stats"] and a["time"] == b["time"] and a["phase_draws"] == b["phase_draws"], what


@pytest.mark.parametrize("name", AC.STATES)
def test_a_session_of_analyses_changes_nothing(pb, name):
    st = AC.state(name)
    sim, twin = AC.bring(pb, st), AC.bring(pb, st, mark=False)
    try:
        before = engine_side(sim, st)
        run_plain(st, sim, AC.orders(st)["shuffle3"])
        assert_same_engine_side(engine_side(sim, st), before, f"{name} around the shuffle")
        for s in (sim, twin):
            assert s.step(30, dt=AC.DT, sort_interval=AC.SORT_INTERVAL) == 30
        assert_same_engine_side(engine_side(sim, st), engine_side(twin, st), f"{name} 30 steps on")
        assert sim.stats()["steps"] == before["stats"]["steps"] + 30
    finally:
        sim.close()
        twin.close()


# ---- 3. the recorders ------------------------------------------------------------------------------------------------

def test_recorders_run_through_interleaved_analyses(pb):
    st = AC.state("batch3x300")
    shuffles = [AC.orders(st)[f"shuffle{k}"] for k in range(3)]

    def run(analyses):
        sim = AC.bring(pb, st)
        try:
            sim.set_series(0.05, 16)
            sim.set_time_correlation(0.05, 4, 0.5)
            sim.set_scattering(0.05, 4, AC.SK_BOX, VEC3)
            sim.set_van_hove(AC.VAN_HOVE_INTERVAL, AC.VAN_HOVE_LAGS, AC.van_hove_self_width(), AC.VAN_HOVE_BINS)
            sim.set_van_hove_distinct(AC.VAN_HOVE_INTERVAL, AC.VAN_HOVE_LAGS, *AC.VAN_HOVE_DISTINCT)
            sim.set_centroid_trail(True)
            for chunk in range(4):
                assert sim.step(10, dt=AC.DT, sort_interval=AC.SORT_INTERVAL) == 10
                if analyses and chunk < 3:
                    run_plain(st, sim, shuffles[chunk])
                if chunk == 1:
                    sim.time_correlation_record()
                    sim.scattering_record()
                    sim.van_hove_record()
                    sim.van_hove_distinct_record()
            return {"series": [sim.series_of(m) for m in range(st.nsims)], "series_info": sim.series_info(),
                    "time_correlation": sim.time_correlation(), "time_correlation_info": sim.time_correlation_info(),
                    "scattering": sim.scattering(), "scattering_info": sim.scattering_info(),
                    "van_hove": sim.van_hove(), "van_hove_info": sim.van_hove_info(),
                    "van_hove_distinct": sim.van_hove_distinct(), "van_hove_distinct_info": sim.van_hove_distinct_info(),
                    "trail": [sim.centroid_trail(m) for m in range(st.nsims)],
                    "states": [sim.get_state_of(m) for m in range(st.nsims)], "stats": sim.stats(), "time": sim.time,
                    "phase_draws": sim.phase_draws}, counters(sim)
        finally:
            sim.close()

    (got, ran), (want, idle) = run(True), run(False)
    # the analyses ran in between, three doubled shuffles of them; the twin made none beyond the recipe's mark
    assert ran["correlation_times"] == 3 * 2 * 9 and ran["field_times"] == 3 * 2 * 6 and ran["render_stats"] == 3 * 2 * 3
    assert ran["cluster_times"] > 0 and ran["rearrangement_times"] > 1 and ran["strain_times"] == 3 * 2 * 6
    assert [idle[k] for k in COUNTERS[:7]] == [0, 0, 0, 1, 0, 0, 0] and idle["render_stats"] == 0
    assert idle["strain_times"] == 0
    assert ran["series_times"] == idle["series_times"] and ran["scattering_times"] == idle["scattering_times"]
    assert ran["time_correlation_times"] == idle["time_correlation_times"]
    assert ran["van_hove_times"] == idle["van_hove_times"] >= 5
    assert ran["van_hove_distinct_times"] == idle["van_hove_distinct_times"] == idle["van_hove_times"]
    # the twin recorded something: rows while stepping, both manual records, a trail slot per member
    assert want["series_info"]["records"] >= 4 and len(want["series"][1]) == want["series_info"]["records"]
    assert want["time_correlation_info"]["records"] >= 5 and want["scattering_info"]["records"] >= 5
    assert all(rec >= 1 for _, _, rec in want["trail"])
    assert want["time_correlation"][0][1]["samples"] > 0 and want["scattering"][2][1][1]["samples"] > 0
    assert want["van_hove_info"]["records"] == want["van_hove_distinct_info"]["records"] >= 5
    for m in (0, 2):  # (nothing planted there) the ring of four lags wrapped, and both tables hold counts at its last lag
        assert sum(want["van_hove"][m][3]["radial"]) > 0 and want["van_hove_distinct"][m][3]["pairs"] > 0, m
    for key in want:
        assert AC.same_bits(got[key], want[key]), key


# ---- 4. counters and memory --------------------------------------------------------------------------------------------

def counters(sim):
    return {name: getattr(sim, name)()[0] for name in COUNTERS}


@pytest.mark.parametrize("name", AC.STATES)
def test_counters_and_memory_do_not_depend_on_the_order(pb, name):
    """The recipe's own mark counts as one run of the rearrangement clock: the counts compared are those of the order,
    taken behind the recipe.  Every buffer is sized by ensure() to the most any call asked for, and every order makes
    the same calls: the memory held is the same, twice through included."""
    st = AC.state(name)
    start = live_memory()
    runs, held = {}, {}
    for order_name, order in AC.orders(st).items():
        sim = AC.bring(pb, st)
        try:
            base = counters(sim)
            assert base["rearrangement_times"] == 1 and sum(base.values()) == 1
            run_plain(st, sim, order)
            after = counters(sim)
            runs[order_name] = {k: after[k] - base[k] for k in after}
            held[order_name] = live_memory()
        finally:
            sim.close()
        assert live_memory() == start, order_name
    once = runs["catalogue"]
    print(name, once, held["catalogue"], start)
    assert once["cluster_times"] > 0 and once["contact_times"] > 0 and once["structure_times"] > 0
    assert once["rearrangement_times"] > 0 and once["correlation_times"] == 9 and once["field_times"] == 6
    assert once["structure_factor_times"] == 6 and once["render_stats"] == 3
    assert once["strain_times"] == sum(1 for e in AC.catalogue(st) if e.family == "strain") == 6
    assert once["series_times"] == once["time_correlation_times"] == once["scattering_times"] == 0
    assert once["van_hove_times"] == once["van_hove_distinct_times"] == 0
    assert runs["reversed"] == once
    for k in range(AC.SHUFFLES):
        assert runs[f"shuffle{k}"] == {key: 2 * v for key, v in once.items()}, k
    assert held["catalogue"][0] > start[0] and held["catalogue"][1] > start[1]
    for order_name in AC.ORDERS:
        assert held[order_name] == held["catalogue"], order_name


# ---- 5. a refused call in the middle -------------------------------------------------------------------------------------

def test_a_refused_call_in_the_middle_leaves_the_session_usable(pb, fresh):
    st = AC.state("batch3x300")
    answers = fresh(st.name)
    entries = AC.catalogue(st)
    by_name = {e.name: (i, e) for i, e in enumerate(entries)}
    empty = np.zeros((0, 2), np.int32)
    view = (st.view["center"], st.view["half"])
    sim = AC.bring(pb, st)

    def good(name, mark="A"):
        i, e = by_name[name]
        got = e.norm(e.call(sim))
        e.check(got, AC.expected(st, e, mark))
        assert AC.same_bits(got, answers[i, mark if e.reads_mark else None]), name

    def refused(match, call):
        with pytest.raises(RuntimeError, match=match):
            call()

    try:
        before = counters(sim)
        for name, refusals in (
            ("clusters(0.0019)", [("code 2.*pbSimClusterStats.*linkGap must be finite and >= 0", lambda: sim.clusters(-1.0)),
                                  ("code 2.*pbSimClusterLabelsOf.*member out of range",
                                   lambda: sim.cluster_labels(0.0019, member=3))]),
            ("contacts(0.0019, member 1)", [("code 2.*pbSimContactsOf.*linkGap", lambda: sim.contacts(-1.0, member=1)),
                                            ("code 2.*pbSimContactVirialOf.*member out of range",
                                             lambda: sim.contact_virial(0.0019, member=3))]),
            ("hexatic(0.0019, member 2)", [("code 2.*pbSimStructureStats.*linkGap", lambda: sim.structure(-1.0)),
                                           ("code 2.*pbSimHexaticOf.*member out of range",
                                            lambda: sim.hexatic(0.0019, member=3))]),
            ("radial_counts(0.4, 7)", [("code 2.*pbSimRadialCounts", lambda: sim.radial_counts(0.4, 0)),
                                       ("code 2.*pbSimRadialCounts.*bins must be 1 ... 4096",
                                        lambda: sim.radial_counts(0.4, 4097))]),
            ("pair_correlation(velocity, 0.4, 7)", [("code 2.*pbSimPairCorrelation.*bins must be 1 ... 1024",
                                                     lambda: sim.pair_correlation("velocity", 0.4, 0)),
                                                    ("code 2.*pbSimPairCorrelation.*bins must be 1 ... 1024",
                                                     lambda: sim.pair_correlation("velocity", 0.4, 1025))]),
            ("field_map(8x8)", [("code 2.*pbSimFieldMap.*nx and ny must be 1 ... 1024", lambda: sim.field_map(0, 8, *view)),
                                ("code 2.*pbSimFieldMapOf.*member out of range",
                                 lambda: sim.field_map(8, 8, *view, member=3))]),
            ("structure_factor(3 vectors, velocity)", [("code 2.*pbSimStructureFactor.*nvec must be 1 ... 4096",
                                                        lambda: sim.structure_factor(empty, AC.SK_BOX)),
                                                       ("code 2.*pbSimStructureFactorOf.*member out of range",
                                                        lambda: sim.structure_factor(VEC3, AC.SK_BOX, member=3))]),
            ("rearrangement()", [("code 2.*pbSimRearrangementOf.*member out of range", lambda: sim.rearrangement_of(3)),
                                 ("code 2.*pbSimMarkReference.*linkGap", lambda: sim.mark_reference(-1.0))]),
            ("strain(0.0)", [("code 2.*pbSimStrainStats.*d2Threshold", lambda: sim.strain(-1.0)),
                             ("code 2.*pbSimStrainOf.*member out of range", lambda: sim.strain_of(3))]),
        ):
            good(name)
            refused(*refusals[0])
            good(name)
            refused(*refusals[1])
            good(name)
        # a refused mark is refused before it touches the one held
        assert sim.reference_info()["marked"] and sim.reference_info()["gap"] == float(f32(AC.MARKS["A"]))
        sim.clear_reference()
        for call in (sim.rearrangement, sim.rearrangement_of, lambda: sim.pair_correlation("displacement", 0.4, 7),
                     sim.strain, sim.strain_of):
            refused("code 2.*no reference marked", call)
        refused("code 2.*pbSimGetColorsOf", lambda: sim.colors(3))
        # nothing refused was counted; every good call was
        after = counters(sim)
        for name in ("rearrangement_times", "correlation_times", "field_times", "structure_factor_times", "strain_times"):
            assert after[name] == before[name] + 3, (name, before, after)
        # the whole catalogue behind all that: every family still gives its fresh-session answer; the mark is gone until
        # an entry takes a new one, so the three reads and the displacement correlations come behind the two that do
        takers = [i for i, e in enumerate(entries) if e.sets_mark]
        rest = [i for i, e in enumerate(entries) if not e.sets_mark]
        failures = run_checked(st, sim, takers + rest, answers, "behind the refusals")
        assert not failures, (len(failures), failures[:12])
        assert_is_the_state(sim, st)
    finally:
        sim.close()
