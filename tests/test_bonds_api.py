"""CPU checks of the bond recorder (pbSimSetBondDynamics ... pbSimGetBondDynamicsTimes, csrc/pb_bonds.hip).

1. tests/bonds_ref.py, the reference the GPU tests compare against: it equals a plain O(n^2) loop over sets, it satisfies
   its identities (lag 0, the rearrangement analysis' bond columns, a rigid shift, the overlap's tie) and it gives the
   hand-built answers.
2. The recipe of tests/test_gpu_bonds.py leaves few bots out, breaks some bonds but not all, and reaches every k: the
   numbers are pinned.
3. The summary on known integers, a row from its words.
4. The symbols, the header's words and bad arguments before the device is touched.
5. The runner knows --bonds and its options and refuses them on the legacy engine; the host library's wrappers refuse on
   the host engine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bonds_ref as BR
import dynamics_ref as DR
from helpers import jittered_blob
from test_runner_analysis_flags import USAGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
Q = 1 << 20  # quanta per world unit

# ---- what tests/test_gpu_bonds.py records ----------------------------------------------------------------------------
GAP, MAX_RADIUS, INSIDE_RADIUS, OVERLAP = 0.0019, 0.125, 0.1, 0.0078125
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025)
RECORDS, LAGS = 7, 3


def walk_records(n, center=(0.0, 0.0), records=RECORDS, seed=None):
    """(records, rad): tests/helpers.py's blob and a walk of multiples of 1/256 within +-1/64 per axis and record."""
    rng = np.random.default_rng(9000 + n if seed is None else seed)
    pos, _, rad = jittered_blob(n, 0.15, rng, center=center, jitter=0.3)
    recs = [pos]
    for _ in range(records - 1):
        step = (rng.integers(-4, 5, size=pos.shape) / 256.0).astype(f32)
        recs.append((recs[-1] + step).astype(f32))
    return recs, rad


def dyadic_records(n=257, shifts=((0.5, -0.25), (3.0, 1.0 / 1024.0), (-7.75, 12.5))):
    """(records, rad, shifts in quanta): the blob rounded to multiples of 2^-10 and shifted rigidly by multiples of
    2^-10, cumulatively: every fp32 sum and difference is exact, so the links of every record are those of the first."""
    pos, _, rad = jittered_blob(n, 0.15, np.random.default_rng(9100 + n), jitter=0.3)
    pos = (np.rint(pos * f32(1024.0)) / f32(1024.0)).astype(f32)
    recs, total, moved = [pos], np.zeros(2), []
    for s in shifts:
        total = total + np.asarray(s)
        recs.append((pos + total.astype(f32)).astype(f32))
        assert np.array_equal(recs[-1].astype(np.float64), pos.astype(np.float64) + total)
        moved.append((int(total[0] * Q), int(total[1] * Q)))
    return recs, rad, moved


def rosette(discs):
    """(pos, rad): a disc of radius 0.3 at the origin and `discs` of radius 0.05 around it, 0.0005 clear of it."""
    angle = 2.0 * np.pi * np.arange(discs) / discs
    ring = 0.3505 * np.stack([np.cos(angle), np.sin(angle)], axis=1)
    pos = np.concatenate([np.zeros((1, 2)), ring]).astype(f32)
    return pos, np.concatenate([[0.3], np.full(discs, 0.05)]).astype(f32)


def tie_records(radius):
    """Two bots in contact; the second moves by exactly `radius` along x: s == (1 qa)^2 for both."""
    pos = np.array([[0.0, 0.0], [0.0, 0.2]], f32)
    then = pos.copy()
    then[1, 0] += f32(radius)
    return [pos, then], np.full(2, 0.1, f32)


# ---- 1. the reference --------------------------------------------------------------------------------------------------

def plain_table(records, rad, lags, gap, max_radius, overlap_radius):
    """The definition as a loop over every pair of bots and over Python sets, in float32 where the header says so."""
    qa = int(np.rint(f32(overlap_radius) * f32(Q)))
    snaps = []
    for pos in records:
        pos, rad = np.asarray(pos, f32), np.asarray(rad, f32)
        n = len(rad)
        with np.errstate(all="ignore"):
            here = [bool(abs(pos[i, 0]) < 2048 and abs(pos[i, 1]) < 2048 and np.isfinite(rad[i]) and rad[i] <= f32(max_radius))
                    for i in range(n)]
            q = [(int(np.rint(pos[i, 0] * f32(Q))), int(np.rint(pos[i, 1] * f32(Q)))) if here[i] else None for i in range(n)]
            links = [set() for _ in range(n)]
            for i in range(n):
                for j in range(n):
                    if i != j and here[i] and here[j]:
                        rx, ry = pos[j, 0] - pos[i, 0], pos[j, 1] - pos[i, 1]
                        dist = np.sqrt(f32(rx * rx) + f32(ry * ry))
                        if f32(dist - f32(rad[i] + rad[j])) < f32(gap):
                            links[i].add(j)
        snaps.append((here, q, links))
    rows = [BR.empty_row(l) for l in range(lags)]
    for r in range(len(snaps)):
        for l in range(min(r, lags - 1) + 1):
            (hn, qn, ln), (ht, qt, lt) = snaps[r], snaps[r - l]
            row = rows[l]
            row["origins"] += 1
            for i in range(len(hn)):
                if not (hn[i] and ht[i]):
                    continue
                if len(ln[i]) > 8 or len(lt[i]) > 8:
                    row["crowded"] += 1
                    continue
                t, w, kept = len(lt[i]), len(ln[i]), len(lt[i] & ln[i])
                row["samples"] += 1
                row["bonds_then"] += t
                row["bonds_now"] += w
                row["bonds_kept"] += kept
                row["bots_unchanged"] += kept == t == w
                row["bots_lost"] += kept < t
                row["bots_gained"] += kept < w
                if t < 1 or not all(hn[j] for j in lt[i]):
                    continue
                d = lambda x, a: qn[x][a] - qt[x][a]
                c = [t * d(i, a) - sum(d(j, a) for j in lt[i]) for a in (0, 1)]
                if max(abs(c[0]), abs(c[1])) >= 1 << 31:
                    continue
                s = c[0] ** 2 + c[1] ** 2
                row["cage_samples"][t - 1] += 1
                row["cage_overlap"][t - 1] += s < (t * qa) ** 2
                row["cage_q2"][t - 1] += s
                row["plain_q2"] += d(i, 0) ** 2 + d(i, 1) ** 2
    return rows


@pytest.mark.parametrize("n,max_radius", [(65, MAX_RADIUS), (130, INSIDE_RADIUS)])
def test_reference_equals_a_plain_loop_over_sets(n, max_radius):
    recs, rad = walk_records(n, records=4)
    recs[2][5] = np.nan, 0.0
    recs[1][7, 1] = 2048.0
    got = BR.table(recs, rad, [0, 3, 5, 9], 3, GAP, max_radius, OVERLAP)
    want = plain_table(recs, rad, 3, GAP, max_radius, OVERLAP)
    want[1]["sum_steps"], want[2]["sum_steps"] = 3 + 2 + 4, 5 + 6
    assert got == want
    assert all(tuple(r) == tuple(want[0]) for r in got) and set(got[0]) == set(BR.FIELDS)
    assert got[1]["samples"] > n and got[1]["bots_lost"] > 0 and sum(got[1]["cage_samples"]) > n // 4


def test_lag_zero_pairs_a_record_with_itself():
    recs, rad = walk_records(257)
    rows = BR.table(recs, rad, [0] * 7, 3, GAP, MAX_RADIUS, OVERLAP)
    zero = rows[0]
    assert zero["bonds_kept"] == zero["bonds_then"] == zero["bonds_now"] > 0
    assert zero["bots_unchanged"] == zero["samples"] and zero["bots_lost"] == zero["bots_gained"] == 0
    assert zero["cage_q2"] == [0] * 8 and zero["plain_q2"] == 0
    assert zero["cage_overlap"] == zero["cage_samples"] and sum(zero["cage_samples"]) > 0  # qa >= 1: 0 < (k qa)^2
    none = BR.table(recs, rad, [0] * 7, 3, GAP, MAX_RADIUS, 0.0)[0]
    assert none["cage_overlap"] == [0] * 8 and none["cage_samples"] == zero["cage_samples"]  # a radius of 0 overlaps nothing


def test_bond_columns_are_the_rearrangement_analysis_when_nobody_is_absent_or_crowded():
    recs, rad = walk_records(64, records=2)
    rows = BR.table(recs, rad, [0, 0], 2, GAP, MAX_RADIUS, OVERLAP)
    want, _ = DR.analyse(recs[0], rad, recs[1], rad, f32(GAP))
    one = rows[1]
    assert one["crowded"] == 0 and one["samples"] == 64
    assert ([one[k] for k in ("bonds_then", "bonds_now", "bonds_kept", "bots_unchanged", "bots_lost", "bots_gained")] ==
            [want[k] for k in ("bonds_marked", "bonds_now", "bonds_kept", "bots_unchanged", "bots_lost", "bots_gained")])
    assert 0 < one["bonds_kept"] < one["bonds_then"]


def test_a_rigid_shift_keeps_every_bond_and_every_cage():
    recs, rad, moved = dyadic_records()
    rows = BR.table(recs, rad, [0] * 4, 4, GAP, MAX_RADIUS, OVERLAP)
    for l, row in enumerate(rows):
        assert row["bonds_kept"] == row["bonds_then"] == row["bonds_now"] > 0 and row["bots_unchanged"] == row["samples"]
        assert row["cage_q2"] == [0] * 8 and row["cage_overlap"] == row["cage_samples"]
    caged = sum(rows[0]["cage_samples"]) // 4  # the same bots are caged in every record
    assert caged > 200
    shift = lambda a, b: (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2
    at = [(0, 0)] + moved
    for l in range(1, 4):
        assert rows[l]["plain_q2"] == caged * sum(shift(at[r], at[r - l]) for r in range(l, 4))
    assert rows[3]["plain_q2"] == caged * ((-4.25 * Q) ** 2 + (12.25 * Q + 1024) ** 2)


def test_a_tie_does_not_overlap_and_one_quantum_more_does():
    recs, rad = tie_records(OVERLAP)
    qa = BR.qa_of(OVERLAP)
    tie = BR.table(recs, rad, [0, 0], 2, GAP, MAX_RADIUS, OVERLAP)[1]
    assert tie["cage_samples"][0] == 2 and tie["cage_q2"][0] == 2 * qa * qa and tie["cage_overlap"][0] == 0
    more = BR.table(recs, rad, [0, 0], 2, GAP, MAX_RADIUS, OVERLAP + 2.0 ** -20)[1]
    assert more["cage_q2"] == tie["cage_q2"] and more["cage_overlap"][0] == 2
    assert tie["bonds_kept"] == 2 and tie["plain_q2"] == qa * qa  # only the second bot moved


def test_hand_cases():
    # a pair of bots, k = 1: the second moves by 1/256 along x and each sees the other's displacement
    pos = np.array([[0.0, 0.0], [0.2, 0.0]], f32)
    rad = np.full(2, 0.1, f32)
    later = pos + np.array([[0.0, 0.0], [1.0 / 256.0, 0.0]], f32)
    row = BR.table([pos, later], rad, [10, 14], 2, 0.01, 0.125, 1.0)[1]
    assert row == dict(BR.empty_row(1), origins=1, sum_steps=4, samples=2, bonds_then=2, bonds_now=2, bonds_kept=2,
                       bots_unchanged=2, plain_q2=4096 ** 2, cage_samples=[2] + [0] * 7, cage_overlap=[2] + [0] * 7,
                       cage_q2=[2 * 4096 ** 2] + [0] * 7)
    # a rosette of 8: the large disc is sampled with k = 8; of 9: it is crowded, and the small discs are not
    for discs in (8, 9):
        pos, rad = rosette(discs)
        row = BR.table([pos, pos], rad, [0, 0], 2, 0.001, 0.3, 0.01)[1]
        assert row["crowded"] == (discs == 9) and row["samples"] == discs + (discs == 8)
        assert row["bonds_then"] == discs + 8 * (discs == 8)
        assert row["cage_samples"] == [discs, 0, 0, 0, 0, 0, 0, int(discs == 8)]
    # a radius one step above maxRadius is absent: the rosette's discs have no links left
    pos, rad = rosette(8)
    row = BR.table([pos, pos], rad, [0, 0], 2, 0.001, float(np.nextafter(f32(0.3), f32(0.0))), 0.01)[1]
    assert (row["samples"], row["bonds_then"], sum(row["cage_samples"])) == (8, 0, 0)
    # a neighbour that turns NaN uncages its bot: the large disc loses its cage, the other discs keep theirs
    later = pos.copy()
    later[3, 0] = np.nan
    row = BR.table([pos, later], rad, [0, 0], 2, 0.001, 0.3, 0.01)[1]
    assert row["samples"] == 8 and row["bonds_then"] == 7 + 8 and row["bonds_kept"] == 7 + 7
    assert row["cage_samples"] == [7, 0, 0, 0, 0, 0, 0, 0] and row["bots_lost"] == 1
    # a displacement of 300 with k = 8: 8 x 300 x 2^20 is past 2^31, so the large disc is sampled and not caged; the
    # discs around it, k = 1, see 300 x 2^20 < 2^31 and are caged, and their own plain displacement is 0
    later = pos.copy()
    later[0, 0] = 300.0
    row = BR.table([pos, later], rad, [0, 0], 2, 0.001, 0.3, 0.01)[1]
    assert row["samples"] == 9 and row["bonds_then"] == 16 and row["bonds_kept"] == 0 and row["bots_lost"] == 9
    assert row["cage_samples"] == [8] + [0] * 7 and row["cage_q2"] == [8 * (300 * Q) ** 2] + [0] * 7
    assert row["plain_q2"] == 0 and row["cage_overlap"] == [0] * 8


# ---- 2. the GPU recipe ---------------------------------------------------------------------------------------------------

PINNED = {  # n: (crowded at lag 1, bonds kept, bonds then at lag 1; bonds kept, bonds then at lag 2)
    63: (0, 1482, 1590, 1196, 1332), 64: (0, 1616, 1720, 1300, 1436), 65: (2, 1574, 1706, 1255, 1433),
    255: (11, 7129, 7593, 5815, 6353), 256: (7, 7001, 7452, 5684, 6219), 257: (12, 7132, 7593, 5782, 6321),
    1025: (44, 29104, 31096, 23565, 25861)}


@pytest.fixture(scope="module")
def recipe_tables():
    return {n: BR.table(*walk_records(n), [0] * RECORDS, LAGS, GAP, MAX_RADIUS, OVERLAP) for n in PINNED}


def test_the_recipe_leaves_few_bots_out_and_breaks_some_bonds(recipe_tables):
    for n, rows in recipe_tables.items():
        one, two = rows[1], rows[2]
        assert (one["crowded"], one["bonds_kept"], one["bonds_then"], two["bonds_kept"], two["bonds_then"]) == PINNED[n], n
        for l, row in enumerate(rows):
            assert row["samples"] + row["crowded"] == (RECORDS - l) * n  # everybody is present
            assert 50 * row["crowded"] <= row["samples"] + row["crowded"], (n, l)  # at most 2 %
        assert 0 < one["bonds_kept"] < one["bonds_then"] and 0 < two["bonds_kept"] < two["bonds_then"]
        if n >= 64:
            assert all(c > 0 for c in one["cage_samples"]), n  # every k from 1 to 8
        assert 0 < sum(one["cage_overlap"]) < sum(one["cage_samples"])  # some cages overlap, some do not
    assert recipe_tables[1025][1]["crowded"] >= 1
    inside = BR.table(*walk_records(257), [0] * RECORDS, LAGS, GAP, INSIDE_RADIUS, OVERLAP)
    assert 0 < inside[1]["samples"] + inside[1]["crowded"] < 6 * 257 * 3 // 4  # a quarter of the bots and more are absent


# ---- 3. the summary and the row ----------------------------------------------------------------------------------------

def test_summary_on_known_integers():
    import particlerobotsimulations_amd as pb
    row = dict(BR.empty_row(2), origins=4, sum_steps=100, samples=30, crowded=10, bonds_then=120, bonds_now=118,
               bonds_kept=90, bots_unchanged=12, bots_lost=15, bots_gained=9, plain_q2=5 << 40,
               cage_samples=[2, 2, 0, 0, 0, 0, 0, 4], cage_overlap=[1, 0, 0, 0, 0, 0, 0, 1],
               cage_q2=[1 << 40, 4 << 40, 0, 0, 0, 0, 0, 64 << 40])
    assert pb.bond_dynamics_summary(row) == {"bond_survival": 0.75, "fraction_lost": 0.5, "cage_msd": 3.0 / 8.0,
                                             "plain_msd": 5.0 / 8.0, "cage_overlap": 0.25, "crowded_fraction": 0.25,
                                             "mean_lag_steps": 25.0}
    assert pb.bond_dynamics_summary(BR.empty_row(0)) == dict.fromkeys(
        ("bond_survival", "fraction_lost", "cage_msd", "plain_msd", "cage_overlap", "crowded_fraction", "mean_lag_steps"))
    third = pb.bond_dynamics_summary(dict(row, cage_q2=[0, 0, 1 << 40, 0, 0, 0, 0, 0]))["cage_msd"]
    assert third == 1.0 / 72.0  # (1 / 9) / 8 as one exact fraction, rounded once


def test_a_row_composes_from_its_words():
    from particlerobotsimulations_amd import _capi
    m = _capi.pbMoment128
    row = _capi.pbBondRow(lag=2, reserved=9, origins=5, sum_steps=60, samples=50, crowded=3, bonds_then=40, bonds_now=41,
                          bonds_kept=39, bots_unchanged=30, bots_lost=4, bots_gained=5, plain_q2=m(7, (1 << 62) + 1),
                          cage_samples=(C.c_ulonglong * 8)(*range(1, 9)), cage_overlap=(C.c_ulonglong * 8)(*range(8)),
                          cage_q2=(m * 8)(*[m(k, k << 50) for k in range(8)]))
    d = _capi.bond_row(row)
    assert d == {"lag": 2, "origins": 5, "sum_steps": 60, "samples": 50, "crowded": 3, "bonds_then": 40, "bonds_now": 41,
                 "bonds_kept": 39, "bots_unchanged": 30, "bots_lost": 4, "bots_gained": 5,
                 "plain_q2": (((1 << 62) + 1) << 32) + 7, "cage_samples": list(range(1, 9)),
                 "cage_overlap": list(range(8)), "cage_q2": [(k << 82) + k for k in range(8)]}
    assert tuple(d) == BR.FIELDS
    assert _capi.BOND_ROW_DTYPE.itemsize == C.sizeof(_capi.pbBondRow) == 360
    as_record = np.frombuffer(bytes(row), _capi.BOND_ROW_DTYPE)[0]
    assert int(as_record["bonds_kept"]) == 39 and int(as_record["plain_q2_hi"]) == (1 << 62) + 1
    assert as_record["cage_q2"].tolist() == [[k, k << 50] for k in range(8)]


# ---- 4. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimSetBondDynamics", "pbSimBondDynamicsRecord", "pbSimGetBondDynamicsInfo", "pbSimGetBondDynamics",
         "pbSimGetBondDynamicsTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _analysis, _capi, host
    import particlerobotsimulations_amd as pb
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert "typedef struct pbBondRow {             /* 360 bytes */" in header
    for line in ("#define PB_BOND_MAX_LAGS 64u", "#define PB_BOND_BLOCKS 256u", "#define PB_BOND_WIDTH 8u"):
        assert line in header
    assert (_capi.BOND_MAX_LAGS, _capi.BOND_WIDTH) == (64, 8) == (64, BR.WIDTH)
    csrc = os.path.join(ROOT, "particlerobotsimulations_amd", "csrc")
    source = open(os.path.join(csrc, "pb_bonds.hip")).read()
    assert "static_assert(sizeof(pbBondRow) == 360" in source and '#include "pb_bonds.hpp"' in source
    for word in ("pbClusterFile(S, 2.0 * (double)B.maxRadius + (double)B.gap, 0.0)", "pbWalkNine<false>", "pbWhenLinked(",
                 "pbLagPair(", "pbClusterEnsureScratch(S)", "pbLagFetch(", "__HIP_MEMORY_SCOPE_WORKGROUP"):
        assert word in source, word
    arithmetic = open(os.path.join(csrc, "pb_bonds.hpp")).read()
    for word in ("pbBondPresent", "pbBondSort", "pbBondKept", "pbBondCage", "pbBondOverlaps", "pbBondPlainSplit",
                 "PB_BOND_WORDS"):
        assert word in arithmetic and word in source, word
    engine = open(os.path.join(csrc, "pb_engine.hpp")).read()
    assert "PB_BOND_MAX_LAGS == PB_LAG_MAX_LAGS" in engine and "PB_BOND_BLOCKS == PB_LAG_BLOCKS" in engine
    assert "struct PbBondDynamics" in engine and "PbLagRing<int4> lag;" in engine
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert " pb_bonds.hip" in makefile and " pb_bonds.hpp" in makefile
    for name in ("pbHostSetBondDynamics", "pbHostBondDynamicsRecord", "pbHostBondDynamicsInfo", "pbHostBondDynamicsRows"):
        assert hasattr(host.lib(), name)
    for name in ("set_bond_dynamics", "bond_dynamics_record", "bond_dynamics_info", "bond_dynamics", "bond_dynamics_times"):
        assert hasattr(pb.Sim, name) and hasattr(pb.Ensemble, name)
    assert "bond_dynamics_summary" in pb.__all__
    assert [k for k, _ in _analysis.BOND_DYNAMICS_INFO] == ["interval", "lags", "link_gap", "max_radius",
                                                            "overlap_radius", "records"]
    block = header.split("Bond dynamics on the device")[1].split("#define PB_BOND_MAX_LAGS")[0]
    flat = re.sub(r"\s*\n \*\s+", " ", block)
    for word in ("BOND-BREAKING", "CAGE-RELATIVE", "Mermin-Wagner", "PRESENT iff", "finite and <= maxRadius",
                 "fl(dist - (ri + rj)) < linkGap", "(2 maxRadius + linkGap)(1 + 2^-10)", "a record never waits",
                 "(qx, qy, degree, 0)", "(INT32_MIN, 0, 0, 0)", "strictly ascending, padded with 0xFFFFFFFF", "CROWDED",
                 "48 bytes per bot and slot", "SAMPLED iff", "kept = |N_then n N_now|", "CAGED iff k >= 1",
                 "|cx|, |cy| < 2^31", "s < (k qa)^2", "equality does not overlap", "nothing on the device is divided",
                 "|dq| <= 2^32 - 256", "below 2^36", "s < 2^63", "(k qa)^2 < 2^62", "each square is split on its own",
                 "cage_q2[k - 1] < 2^94", "plain_q2 < 2^96", "a lag holds 2^31 samples or more: restart the bond recorder",
                 "behind the four-point record and in front of the centroid trail", "Recording never waits for the device",
                 "not part of a checkpoint", "2 maxRadius + linkGap >= 2048", "outside [0, 256)", "65535 members",
                 "2^28 bots", "2^33 bytes (lags x total x 48)", "per-bot outputs", "logarithmic lags",
                 "lists wider than 8", "rotation-corrected cage", "neighbour exchange (T1) counting", "summary rows",
                 "legacy engine"):
        assert word in block or word in flat, word
    # the pinned sentences of the older blocks stand as they were
    whole = re.sub(r"\s*\n \* ", " ", header)
    assert whole.count("distinct van Hove, coherent scattering, four-point; then the centroid trail and the phase update") == 2
    assert "neighbour-based quantities per lag such as bond lifetime" in whole
    body = open(os.path.join(csrc, "pb_engine.hip")).read().split("PbHostEvent events[10]")[1]
    fired = [body.index(w) for w in ("pbFourPointRecord(B)", "pbBondDynamicsRecord(B)", "trailRecord}", "phaseUpdate(B)")]
    assert fired == sorted(fired)


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    lib = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    row = _capi.pbBondRow(lag=7, samples=7)
    i, l, g, m, a, r, ms = (C.c_float(7.0), C.c_uint(7), C.c_float(7.0), C.c_float(7.0), C.c_float(7.0), C.c_ulonglong(7),
                            C.c_float(7.0))

    def refused(rc, fn, word=None):
        msg = lib.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and fn.encode() in msg and (word is None or word.encode() in msg), (rc, msg)

    fn = "pbSimSetBondDynamics"
    refused(lib.pbSimSetBondDynamics(None, 0.05, 8, 0.0, 0.1, 0.05), fn, "null")
    for bad in (-0.5, -2.0, -1e-30, np.nextafter(f32(-1.0), f32(0.0)), float("nan"), float("inf"), float("-inf")):
        refused(lib.pbSimSetBondDynamics(fake, float(bad), 8, 0.0, 0.1, 0.05), fn, "interval")
        refused(lib.pbSimSetBondDynamics(fake, float(bad), 0, 0.0, 0.1, 0.05), fn, "interval")  # switching off checks it too
    for bad in (65, 1 << 31):
        refused(lib.pbSimSetBondDynamics(fake, 0.05, bad, 0.0, 0.1, 0.05), fn, "lags")
        refused(lib.pbSimSetBondDynamics(fake, -1.0, bad, 0.0, 0.1, 0.05), fn, "lags")  # -1 is an interval
    for bad in (-1e-30, -1.0, float("nan"), float("inf"), float("-inf")):
        refused(lib.pbSimSetBondDynamics(fake, 0.0, 8, bad, 0.1, 0.05), fn, "linkGap")
    for bad in (0.0, -0.0, -1e-30, -1.0, float("nan"), float("inf"), float("-inf")):
        refused(lib.pbSimSetBondDynamics(fake, 0.0, 8, 0.0, bad, 0.05), fn, "maxRadius")
    for gap, radius in ((0.0, 1024.0), (2048.0, 1e-3), (1.0, 1023.5), (1e9, 0.1), (0.0, 1e9)):
        refused(lib.pbSimSetBondDynamics(fake, 0.0, 8, gap, radius, 0.05), fn, "2 maxRadius + linkGap")
    for bad in (-1e-30, -1.0, 256.0, 1e9, float("nan"), float("inf"), float("-inf")):
        refused(lib.pbSimSetBondDynamics(fake, 0.0, 8, 0.0, 0.1, bad), fn, "overlapRadius")
    refused(lib.pbSimBondDynamicsRecord(None), "pbSimBondDynamicsRecord", "null")
    refused(lib.pbSimGetBondDynamicsInfo(None, C.byref(i), C.byref(l), C.byref(g), C.byref(m), C.byref(a), C.byref(r)),
            "pbSimGetBondDynamicsInfo", "null")
    refused(lib.pbSimGetBondDynamicsInfo(fake, None, None, None, None, None, None), "pbSimGetBondDynamicsInfo", "all null")
    refused(lib.pbSimGetBondDynamics(None, C.byref(row)), "pbSimGetBondDynamics", "null")
    refused(lib.pbSimGetBondDynamics(fake, None), "pbSimGetBondDynamics", "null")
    refused(lib.pbSimGetBondDynamicsTimes(None, C.byref(r), C.byref(ms)), "pbSimGetBondDynamicsTimes", "null")
    assert (i.value, l.value, g.value, m.value, a.value, r.value, ms.value) == (7.0, 7, 7.0, 7.0, 7.0, 7, 7.0)
    assert row.lag == 7 and row.samples == 7


# ---- 5. the runner and the other engines -------------------------------------------------------------------------------

NOT_A_NUMBER = ["", "abc", "-1", "-1e-30", "nan", "inf", "-inf", "0.1x"]
BAD_FLAGS = ([("--bonds-interval", v) for v in NOT_A_NUMBER]
             + [("--bonds-lags", v) for v in ("", "0", "-3", "1.5", "65", "many")]
             + [("--bonds-gap", v) for v in NOT_A_NUMBER + ["2048", "1e9"]]
             + [("--bonds-max-radius", v) for v in NOT_A_NUMBER + ["0", "1024", "1e9"]]
             + [("--bonds-overlap", v) for v in NOT_A_NUMBER + ["256", "1e9"]])


@pytest.mark.parametrize("flag,value", BAD_FLAGS, ids=[f"{f}={v!r}" for f, v in BAD_FLAGS])
def test_runner_refuses_a_bad_bonds_value(tmp_path, flag, value):
    for args in ([flag, value], [CFG, "--bonds", "b.csv", flag, value, "--quiet"]):
        r = subprocess.run([RUN] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), args
    assert not os.listdir(tmp_path)


def test_runner_bonds_flags_need_their_values_and_the_fused_engine(tmp_path):
    flags = ("--bonds", "--bonds-interval", "--bonds-lags", "--bonds-gap", "--bonds-max-radius", "--bonds-overlap")
    for flag in flags:
        r = subprocess.run([RUN, CFG, flag], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), flag
    said = "--bonds needs the fused engine (the recorder runs on its resident state)\n"
    for extra in ([], ["--bonds-interval", "0"], ["--bonds-interval", "3.4e38", "--bonds-lags", "1"],
                  ["--bonds-lags", "64", "--bonds-gap", "0"], ["--bonds-gap", "2047.9"], ["--bonds-max-radius", "1023.9"],
                  ["--bonds-overlap", "0"], ["--bonds-overlap", "255.9"]):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--bonds", "b.csv"] + extra, capture_output=True, text=True,
                           timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", said), extra
    # last in the engine-check table: any earlier file flag speaks first
    for flag, line in (("--timecorr", "--timecorr needs the fused engine (the recorder runs on its resident state)\n"),
                       ("--fourpoint", "--fourpoint needs the fused engine (the recorder runs on its resident state)\n")):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--bonds", "b.csv", flag, "a.csv"], capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stderr) == (2, line)
    assert not os.listdir(tmp_path)
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_runner.cpp")).read()
    for flag in ("--bonds FILE", "--bonds-interval T", "--bonds-lags N", "--bonds-gap G", "--bonds-max-radius R",
                 "--bonds-overlap A"):
        assert flag in source and flag in open(os.path.join(ROOT, "README.md")).read(), flag
        assert flag.split()[0] in open(os.path.join(ROOT, "INTEGRATION.md")).read(), flag
    for text in (source, open(os.path.join(ROOT, "INTEGRATION.md")).read()):
        assert "larger than max_radius is ABSENT" in re.sub(r"\s*\n\s*(// )?", " ", text)
    assert "BotsGained, PlainQ2" in source and "BondSurvival, FractionLost, CageMsd, PlainMsd, CageOverlap" in source
    assert "bonds" not in USAGE  # the usage line stays as it is


NEEDS = "the bond recorder needs the fused engine"
REFUSED = [  # the host library's wrappers (HostSim has no methods for this recorder: a caller goes through host.lib())
    (lambda L, h: L.pbHostSetBondDynamics(h, 0.05, 8, 0.0, 0.1, 0.05), "Particlebot::setBondDynamics: " + NEEDS + "\n"),
    (lambda L, h: L.pbHostBondDynamicsRecord(h), "Particlebot::bondDynamicsRecord: " + NEEDS + "\n"),
    (lambda L, h: L.pbHostBondDynamicsInfo(h, None, C.byref(C.c_uint(7)), None, None, None, None),
     "Particlebot::bondDynamicsInfo: " + NEEDS + "\n"),
]


@pytest.mark.parametrize("call,line", REFUSED, ids=["set", "record", "info"])
def test_host_engine_has_no_bond_recorder(capfd, call, line):
    from particlerobotsimulations_amd import _capi, host
    h = host.HostSim(CFG, engine="host")  # (the legacy engine needs a device: tests/test_gpu_bonds.py asks it)
    capfd.readouterr()
    lib = host.lib()
    assert call(lib, h._h) == -1
    assert capfd.readouterr() == ("", line)
    assert lib.pbHostBondDynamicsRows(h._h, None, 0, None) == -1  # a NULL count is refused before the class is asked
    assert capfd.readouterr() == ("", "")
    row, count = _capi.pbBondRow(lag=7), C.c_ulonglong(7)
    assert lib.pbHostBondDynamicsRows(h._h, C.byref(row), 1, C.byref(count)) == -1 and (row.lag, count.value) == (7, 7)
    assert capfd.readouterr() == ("", "Particlebot::bondDynamicsRows: " + NEEDS + "\n")
    h.close()
