"""The analysis-session tests without a GPU: the states of tests/analysis_session_cases.py are reproducible from
their recipe bit for bit (the device's state is later required to equal them), the six orders of each hold every
grow-then-shrink, both switches of the filing kind, the long-lived mark and a strain call directly behind everything
that could disturb it (check_orders), the expectations say something on these states (check_not_trivial, the strain
rows among them), the distinct van Hove records taken between the calls file on a grid no call files on and leave a
table that says something, the van Hove shapes of the interleaving test fill their bins, and the comparisons and the
restatement the cases file adds behave."""
import numpy as np
import pytest

import analysis_session_cases as AC
import geometry_cases as gc

f32 = np.float32


@pytest.mark.parametrize("name", AC.ALL_STATES)
def test_orders_hold_every_precondition(orc, name):
    st = AC.state(name)
    count = AC.check_orders(st)
    assert count == 60
    all_orders = AC.orders(st)
    assert tuple(all_orders) == AC.ORDERS and len(all_orders["shuffle3"]) == 2 * count
    entries = AC.catalogue(st)
    families = {e.family for e in entries}
    assert families == set(AC.FILING) | {"mark", "strain", "field", "sfactor", "moments", "display", "render"}
    # the strain family: three thresholds and three members, every one a reader of the mark and none a taker
    strain = [e for e in entries if e.family == "strain"]
    assert len(strain) == 6 and all(e.reads_mark and not e.sets_mark for e in strain)
    low, middle, high = AC.strain_thresholds()
    assert low == 0.0 and high == 1.0e30 and 0.0 < middle < 1.0e-3 and middle == float(f32(middle))
    assert [e.name for e in strain[:3]] == [f"strain({t!r})" for t in (low, middle, high)]
    # every strain entry is wanted under every mark, by an order or by the session that lost its mark
    index = {e.name: i for i, e in enumerate(entries)}
    wanted = set(AC.needed(st))
    assert all((index[e.name], key) in wanted for e in strain for key in AC.MARKS)
    # the marks an order puts in place: the recipe's until an entry takes another, then that one
    marks = [mark for _, mark in AC.walk(st, all_orders["catalogue"])]
    assert marks[0] == "A" and marks[-2:] == ["B", "C"] and set(marks) == {"A", "B", "C"}
    assert {mark for k in range(4) for _, mark in AC.walk(st, all_orders[f"shuffle{k}"])} == {"A", "B", "C"}


@pytest.mark.parametrize("name", AC.ALL_STATES)
def test_expectations_are_not_trivial(orc, name):
    AC.check_not_trivial(AC.state(name))


def test_strain_expectations_are_the_references_own(orc):
    """The catalogue restates the marked network once per mark and feeds strain_ref.analyse_csr: the same rows and the
    same bits as strain_ref.analyse; and the middle threshold is the median it is said to be."""
    import strain_ref as ER
    st = AC.state("batch3x300")
    _, middle, _ = AC.strain_thresholds()
    for key in AC.MARKS:
        pos0, rad0, gap, _ = AC.mark_of(st, key)
        for m in range(st.nsims):
            row, bots = ER.analyse(pos0[m], rad0[m], st.final[m]["pos"], gap, middle)
            got_row, got_bots = AC._strain(st, key, middle)[m]
            assert got_row == row and tuple(row) == ER.FIELDS
            for k in ("moments", "gradient", "d2min"):
                assert got_bots[k].tobytes() == bots[k].tobytes(), (key, m, k)
    bots = [b for _, b in AC._strain(st, "A", 0.0)]
    d2 = np.concatenate([b["d2min"][b["fitted"]] for b in bots]) / 2.0 ** 40
    assert abs(int((d2 > middle).sum()) - int((d2 < middle).sum())) <= 2 and d2.size > 400
    single = AC._strain(AC.state("single17"), "A", 0.0)[0][0]
    assert single["fitted"] == 13 and single["max_d2"] > 0  # what check_strain_not_trivial's docstring says of it


@pytest.mark.parametrize("name", AC.ALL_STATES)
def test_records_between_the_calls_file_on_a_grid_of_their_own(orc, name):
    st = AC.state(name)
    edge, others = AC.check_record_grid(st)
    # the link rule's edges are those check_not_trivial describes: one cell for everything, or cells of a bot's diameter
    assert (max(others) > 4096.0) == (name == "batch3x300")
    lags, width, bins = AC.RECORD_BETWEEN
    assert lags == 2 and width * bins == 1.0 and all(width * bins != r for r, _ in AC.RADIAL + AC.CORRELATION)
    # and the table they leave says something: pairs at lag 1 in every member, in more than one bin
    import vanhove_distinct_ref as GR
    for m, s in enumerate(st.final):
        rows = GR.table([(s["pos"], s["rad"])] * 3, [0] * 3, lags, width, bins)
        assert rows[1]["pairs"] > 0 and sum(1 for c in rows[1]["counts"] if c) > 1, (m, rows[1])
        assert rows[1]["origins"] == 2 and rows[0]["origins"] == 3


def test_the_interleaving_tests_van_hove_shapes_say_something(orc):
    width = AC.check_van_hove_self_width()
    print("self width", width)
    # the distinct part: rMax 1 inside blobs a few units across, counts in most bins at lag 1 and at lag 3
    import vanhove_distinct_ref as GR
    st = AC.state("batch3x300")
    dw, dbins = AC.VAN_HOVE_DISTINCT
    for m, pos in enumerate(AC.oracle_lagged_positions()):
        rad = st.final[m]["rad"] if m != 1 else st.at_mark[m]["rad"]  # (any finite radii: presence is all they decide)
        rows = GR.table([(p, rad) for p in pos], [0, 5, 10, 15], AC.VAN_HOVE_LAGS, dw, dbins)
        for lag in (1, 3):
            assert sum(1 for c in rows[lag]["counts"] if c) >= dbins // 2 and rows[lag]["pairs"] > 0, (m, lag)


def test_the_limits_the_catalogue_names_are_the_librarys():
    from particlerobotsimulations_amd import _capi
    assert AC.SK_MOST == _capi.SK_MAX_VECTORS
    assert max(b for _, b in AC.RADIAL) == 4096 and max(b for _, b in AC.CORRELATION) == 1024
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "particlebot_hip.h")).read()
    assert "#define PB_RADIAL_MAX_BINS 4096u" in header and "#define PB_CORR_MAX_BINS 1024u" in header


def test_batch_is_reproducible_from_its_recipe(orc):
    """A second run of the recipe gives the same bits, member by member; the state is what its description says."""
    st = AC.state("batch3x300")
    assert (st.nsims, st.n) == (3, 300) and st.n % 64 and st.n % 256
    for k in range(3):
        again = AC._batch_start(k)
        for key, a in again.items():
            assert np.array_equal(a, st.start[k][key]), (k, key)
        at_mark, mark_time, final, time = AC._oracle_run(orc, AC._batch_params(orc, k), again)
        if k == 1:
            final = AC.plant_unmeasured(final)
        assert mark_time == st.mark_time and time == st.time
        for key in ("pos", "vel", "rad", "phase", "dead"):
            assert at_mark[key].tobytes() == st.at_mark[k][key].tobytes(), (k, key)
            assert final[key].tobytes() == st.final[k][key].tobytes(), (k, key)
    assert f32(st.mark_time) < f32(st.time) and abs(st.time - 1.2) < 1e-5 and abs(st.mark_time - 0.9) < 1e-5
    # the bots moved, between the start and the mark and between the mark and the end; three re-sorts fell in between
    for k in range(3):
        assert not np.array_equal(st.start[k]["pos"], st.at_mark[k]["pos"])
        moved = st.final[k]["pos"] != st.at_mark[k]["pos"]
        assert moved.any(axis=1).sum() > 150, k  # (static friction holds some bots where they are)
    # member 1: a tenth dead, and one bot of each unmeasured kind, planted behind the last step
    one = st.final[1]
    assert 20 <= int(one["dead"].sum()) <= 40 and not st.final[0]["dead"].any() and not st.final[2]["dead"].any()
    assert np.isnan(one["pos"][10, 0]) and np.isinf(one["pos"][40, 1]) and one["pos"][77, 0] == -2048.0
    assert one["vel"][123, 1] == 2048.0 and np.isnan(one["rad"][200]) and one["rad"][290] == 2048.0
    import series_ref as MR
    assert MR.moments(one["pos"], one["vel"], one["rad"])["measured"] == 300 - len(AC.UNMEASURED)
    for k in (0, 2):
        s = st.final[k]
        assert np.isfinite(s["pos"]).all() and MR.moments(s["pos"], s["vel"], s["rad"])["measured"] == 300
    # the state without the radius of 2048 is the same in every other bit
    other = AC.state("batch3x300_small_radii")
    for k in range(3):
        for key in ("pos", "vel", "rad", "phase", "dead"):
            differ = np.flatnonzero((other.final[k][key] != st.final[k][key]).reshape(300, -1).any(axis=1)
                                    & ~np.isnan(st.final[k][key]).reshape(300, -1).any(axis=1))
            assert differ.tolist() == ([290] if (k, key) == (1, "rad") else []), (k, key)
    assert other.final[1]["rad"][290] < 0.12
    # stale cell lists: 20 steps behind the last re-sort (at 1.0 s) some bots of every member sit in another cell
    for k in range(3):
        P = st.params[k]
        before = gc.cells(orc, P, _state_at(orc, st, k, 100))
        now = gc.cells(orc, P, np.nan_to_num(st.final[k]["pos"], nan=0.0, posinf=0.0, neginf=0.0))
        assert ((before[0] != now[0]) | (before[1] != now[1])).sum() >= 3, k


def _state_at(orc, st, k, steps):
    osim = orc.Sim(st.params[k], reset=False)
    for key in ("pos", "vel", "rad", "phase", "dead"):
        osim.set(key, st.start[k][key])
    assert osim.run(steps, dt=AC.DT, sort_interval=AC.SORT_INTERVAL)
    pos = osim.get("pos")
    osim.close()
    return pos


def test_single_is_seventeen_bots_marked_and_moved(orc):
    st = AC.state("single17")
    assert (st.nsims, st.n, st.wall_half) == (1, 17, 4.0e6)
    import test_gpu_link_consumers as LC
    pos, rad = LC.blob(17)
    assert np.array_equal(st.at_mark[0]["pos"], pos) and np.array_equal(st.final[0]["rad"], rad)
    assert st.at_mark[0]["vel"].any() and (st.final[0]["pos"] != pos).all()
    assert np.array_equal(st.final[0]["vel"], st.at_mark[0]["vel"])


def test_same_bits_tells_bits_apart():
    a = np.array([0.0, np.nan], f32)
    assert AC.same_bits(a, a.copy()) and not AC.same_bits(a, np.array([-0.0, np.nan], f32))
    assert not AC.same_bits(a, a.astype(np.float64)) and not AC.same_bits(a, a.reshape(1, 2))
    assert AC.same_bits({"x": [1, (2.0, a)]}, {"x": [1, (2.0, a.copy())]})
    assert not AC.same_bits({"x": 1}, {"x": 1, "y": 2}) and not AC.same_bits([1, 2], (1, 2))
    assert not AC.same_bits(0.0, -0.0) and AC.same_bits(float("nan"), float("nan")) and not AC.same_bits(1, 1.0)
    assert AC.same_bits(complex(1.0, -0.0), complex(1.0, -0.0)) and not AC.same_bits(complex(1.0, 0.0), complex(1.0, -0.0))


def test_centroid_restatement_is_the_mean_added_in_the_kernels_order():
    rng = np.random.default_rng(5)
    for n in (1, 17, 256, 257, 300, 70000):
        pos = rng.integers(-50, 51, (n, 2)).astype(f32)  # integers: every addition is exact, whatever the order
        exact = pos.astype(np.int64).sum(axis=0).astype(np.float64) / np.float64(n)
        assert AC.centroid_restated(pos) == (float(exact[0]), float(exact[1])), n
    # four bots whose sum depends on the order: lanes 0 and 128 meet first (1e17 - 1e17), then lanes 0 and 1
    pos = np.zeros((300, 2), f32)
    pos[0, 0], pos[128, 0], pos[1, 0] = 1.0e17, -1.0e17, 3.0
    assert AC.centroid_restated(pos) == (3.0 / 300.0, 0.0)
    pos[128, 0], pos[3, 0] = 0.0, -1.0e17   # lanes 1 and 3 meet first: 3 - 1e17 loses the 3 in float64
    assert AC.centroid_restated(pos) == (0.0, 0.0)
