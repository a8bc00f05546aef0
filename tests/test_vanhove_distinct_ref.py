"""CPU: tests/vanhove_distinct_ref.py, the reference the GPU tests of the distinct van Hove function compare against.  It
equals a plain loop over ordered pairs in Python ints that bisects in vanhove_ref.edges_of; it gives the known answers
written out by hand below (an edge, one quantum below it, the excluded outer edge, coincident bots, a bot that moves onto
another's old position, the unmoved self pair, absent bots of every kind at either instant); lag 0 is even and symmetric;
and with the self part's radial histogram it adds up to the histogram over all ordered pairs.  The recipe of
tests/test_gpu_vanhove_distinct.py is checked here too: conditions on the inputs."""
from bisect import bisect_right

import numpy as np
import pytest

import vanhove_distinct_ref as DR
import vanhove_ref as VR
from test_series_api import CORNER
from test_vanhove_api import MANUAL_LAGS, MANUAL_RECORDS, vanhove_records

f32 = np.float32
ONE = 1 << 20
U = 2.0 ** -20
SHAPES = [(1.0 / 32, 16), (1.0 / 8, 8), (1.0 / 16, 64)]  # (width, bins) of the GPU tests: rMax 0.5, 1 and 4


def with_rad(positions, rad=0.1):
    return [(p, np.full(len(p), rad, f32)) for p in positions]


def plain_table(records, steps, lags, width, bins):
    """The definition as a loop over records, lags and ordered pairs in Python ints, the bin by bisect in the edges."""
    qw = int(np.rint(f32(width) * f32(1048576.0)))
    edges = VR.edges_of(qw, bins)
    rows = [DR.empty_row(l, bins) for l in range(lags)]

    def here(p, r):
        return bool(np.isfinite(p[0]) and np.isfinite(p[1]) and np.isfinite(r))

    for r in range(len(records)):
        for l in range(min(r, lags - 1) + 1):
            row = rows[l]
            (pn, rn), (pt, rt) = records[r], records[r - l]
            row["origins"] += 1
            row["sum_steps"] += steps[r] - steps[r - l]
            row["centres"] += sum(here(p, q) for p, q in zip(pt, rt))
            row["partners"] += sum(here(p, q) for p, q in zip(pn, rn))
            for i in range(len(pt)):
                for j in range(len(pn)):
                    if i == j or not here(pt[i], rt[i]) or not here(pn[j], rn[j]):
                        continue
                    dx, dy = f32(pn[j][0]) - f32(pt[i][0]), f32(pn[j][1]) - f32(pt[i][1])
                    if not (abs(dx) < 2048.0 and abs(dy) < 2048.0):
                        continue
                    qx, qy = int(np.rint(f32(dx * f32(1048576.0)))), int(np.rint(f32(dy * f32(1048576.0))))
                    s = qx * qx + qy * qy
                    if s < edges[bins]:
                        row["counts"][bisect_right(edges, s) - 1] += 1
                        row["pairs"] += 1
    return rows


@pytest.mark.parametrize("width,bins", SHAPES + [(2.0 ** -20, 1), (3 * U, 1024), (2047.0 / 1024, 1024)])
@pytest.mark.parametrize("n", [1, 2, 65])
def test_reference_equals_a_plain_loop(n, width, bins):
    recs = with_rad([r[0] for r in vanhove_records(n, records=4)])
    steps = [0, 3, 4, 10]
    got = DR.table(recs, steps, 3, width, bins)
    assert got == plain_table(recs, steps, 3, width, bins)
    assert [r["origins"] for r in got] == [4, 3, 2] and [r["sum_steps"] for r in got] == [0, 10, 11]
    assert [r["centres"] for r in got] == [4 * n, 3 * n, 2 * n] == [r["partners"] for r in got]
    assert all(r["pairs"] == sum(r["counts"]) for r in got)
    if n == 65 and bins * width > 3.0:
        assert got[1]["pairs"] > 65


def test_integer_root_is_exact_at_squares_and_next_to_them():
    r = np.array([1, 2, 3, 1 << 16, (1 << 26) + 5, 94906266, (1 << 31) - 2, (1 << 31) - 1], np.int64)
    assert np.array_equal(DR.isqrt64(r * r), r) and np.array_equal(DR.isqrt64(r * r - 1), r - 1)
    assert np.array_equal(DR.isqrt64(r * r + 1), r) and np.array_equal(DR.isqrt64(r * r + 2 * r), r)
    assert list(DR.isqrt64(np.array([0, 1, 3, 4, 8, 9, (1 << 62) - 1], np.int64))) == [0, 1, 1, 2, 2, 3, (1 << 31) - 1]


# ---- known answers --------------------------------------------------------------------------------------------------------

KNOWN_WIDTH, KNOWN_BINS = 0.125, 8  # qw = 2^17, rMax = 1


def known_answer_records():
    """Five bots, two records.  THEN bot 0 is at the origin and the others far away; NOW all five are near the origin:
    bot 0 has not moved, bot 1 is exactly three widths from the origin, bot 2 one quantum less, bot 3 exactly bins widths
    away and bot 4 exactly ON bot 0's old (and present) position."""
    then = np.array([[0.0, 0.0], [100.0, 50.0], [200.0, 50.0], [300.0, 50.0], [400.0, 50.0]], f32)
    now = np.array([[0.0, 0.0], [0.375, 0.0], [0.375 - U, 0.0], [1.0, 0.0], [0.0, 0.0]], f32)
    return with_rad([then, now])


def known_answer_rows():
    """The rows of known_answer_records() with steps 0 and 10, written out by hand.
    Lag 1, centre bot 0 at the origin (every other centre is 99 or more away from every bot now): bot 1 has
    s == (3 qw)^2, an edge, which belongs to bin 3; bot 2 is one quantum below it, bin 2; bot 3 has s == (8 qw)^2 and is
    excluded; bot 4 sits on the centre, bin 0, counted once, for the pair (0, 4); the pair (0, 0) is the self pair and is
    not counted although the distance is 0 too.
    Lag 0: record 0 has no pair within 1.  Record 1, x = 0 (bot 0), 0.375, 0.375 - U, 1, 0 (bot 4): the unordered pairs
    (0,4) and (1,2) at 0 and U in bin 0, (0,2) and (2,4) in bin 2, (0,1) and (1,4) in bin 3, (1,3) at 0.625 (an edge)
    and (2,3) at 0.625 + U in bin 5, (0,3) and (3,4) at 1 excluded; each counted from both ends."""
    lag0 = dict(DR.empty_row(0, 8), origins=2, centres=10, partners=10, pairs=16, counts=[4, 0, 4, 4, 0, 4, 0, 0])
    lag1 = dict(DR.empty_row(1, 8), origins=1, sum_steps=10, centres=5, partners=5, pairs=3,
                counts=[1, 0, 1, 1, 0, 0, 0, 0])
    return [lag0, lag1]


def test_known_answers():
    recs = known_answer_records()
    rows = DR.table(recs, [0, 10], 2, KNOWN_WIDTH, KNOWN_BINS)
    assert rows == known_answer_rows() == plain_table(recs, [0, 10], 2, KNOWN_WIDTH, KNOWN_BINS)


ABSENT = [float("nan"), float("inf"), float("-inf")]


def absent_cases():
    """(name, records, the lag-1 row by hand) for a bot absent at either instant, by x, y or rad, each non-finite kind."""
    base = known_answer_rows()[1]
    out = []
    for v in ABSENT:
        for what in ("x", "y", "rad"):
            for who, when in ((0, 0), (4, 1), (1, 1), (1, 0)):
                (pt, rt), (pn, rn) = known_answer_records()
                pos, rad = ((pt, rt), (pn, rn))[when]
                if what == "rad":
                    rad[who] = v
                else:
                    pos[who, "xy".index(what)] = v
                if (who, when) == (0, 0):    # the one centre with partners is absent then: nothing is counted
                    row = dict(base, centres=4, pairs=0, counts=[0] * 8)
                elif (who, when) == (4, 1):  # the partner on the centre is absent now
                    row = dict(base, partners=4, pairs=2, counts=[0, 0, 1, 1, 0, 0, 0, 0])
                elif (who, when) == (1, 1):  # the partner on the edge is absent now
                    row = dict(base, partners=4, pairs=2, counts=[1, 0, 1, 0, 0, 0, 0, 0])
                else:                        # a far centre is absent then: it had no partner, only the count changes
                    row = dict(base, centres=4)
                out.append((f"{what}={v} bot {who} record {when}", [(pt, rt), (pn, rn)], row))
    return out


def test_absent_bots_are_no_centres_and_no_partners():
    cases = absent_cases()
    assert len(cases) == 36
    for name, recs, lag1 in cases:
        rows = DR.table(recs, [0, 10], 2, KNOWN_WIDTH, KNOWN_BINS)
        assert rows[1] == lag1, name
        assert rows == plain_table(recs, [0, 10], 2, KNOWN_WIDTH, KNOWN_BINS), name


# ---- identities -----------------------------------------------------------------------------------------------------------

def all_ordered_pairs_histogram(now, then, width, bins):
    """The radial histogram over ALL ordered (i, j), i == j included, of two position arrays, by bisect."""
    qw = VR.qw_of(width)
    edges = VR.edges_of(qw, bins)
    hist = [0] * bins
    for pi in then:
        for pj in now:
            for qx, qy in VR.quantised_pairs([pj], [pi]):
                s = qx * qx + qy * qy
                if s < edges[bins]:
                    hist[bisect_right(edges, s) - 1] += 1
    return hist


@pytest.mark.parametrize("width,bins", SHAPES)
def test_self_plus_distinct_is_every_ordered_pair_and_lag_zero_is_even_and_symmetric(width, bins):
    recs = [r[0] for r in vanhove_records(65, records=3)]
    self_rows = VR.table(recs, [0, 0, 0], 2, width, bins)
    rows = DR.table(with_rad(recs), [0, 0, 0], 2, width, bins)
    for lag in (0, 1):
        total = [0] * bins
        for r in range(lag, 3):
            total = [a + b for a, b in zip(total, all_ordered_pairs_histogram(recs[r], recs[r - lag], width, bins))]
        assert [a + b for a, b in zip(self_rows[lag]["radial"], rows[lag]["counts"])] == total, lag
    assert all(c % 2 == 0 for c in rows[0]["counts"]) and rows[0]["pairs"] > 0
    qw = VR.qw_of(width)
    i, j, b = DR.counted_pairs(with_rad(recs)[2], with_rad(recs)[2], qw, bins)
    there = sorted(zip(i.tolist(), j.tolist(), b.tolist()))
    assert there == sorted(zip(j.tolist(), i.tolist(), b.tolist()))  # (i, j) and (j, i) in the same bin


# ---- the GPU tests' recipe --------------------------------------------------------------------------------------------------

def test_the_recipe_fills_every_bin_and_moves_bots_out_of_their_cells():
    recs = with_rad([r[0] for r in vanhove_records(1000)])
    assert len(recs) == MANUAL_RECORDS
    for (width, bins), share in zip(SHAPES, (0.015, 0.057, 0.61)):
        i, j, b = DR.counted_pairs(recs[1], recs[0], VR.qw_of(width), bins)
        hist = np.bincount(b, minlength=bins)
        print(width, bins, len(b) / (1000 * 999), int(hist.min()))
        assert hist.min() > 0 and abs(len(b) / (1000 * 999) - share) < 0.1 * share
        assert DR.missed_around_the_current_position(recs[1], recs[0], width, bins) > 0
    small = with_rad([r[0] for r in vanhove_records(63)])
    assert DR.table(small[:2], [0, 0], 2, 1.0 / 32, 16)[1]["pairs"] == 85
    # the grids of n = 1, 63, 65: 4 x 4, 8 x 8 and 16 x 8 cells
    assert [DR.grid_of(n, 0.125, 8)[1:] for n in (1, 63, 65, 4097)] == [(4, 4), (8, 8), (16, 8), (128, 64)]
    # at the corner the positions keep 2^-13 of resolution and stay inside the guaranteed range
    far = [r[0] for r in vanhove_records(257, center=CORNER)]
    assert max(float(np.abs(p).max()) for p in far) < 2100.0
    assert MANUAL_LAGS == 3
