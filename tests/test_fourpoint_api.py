"""CPU side of the four-point recorder (pbSimSetFourPoint / pbSimFourPointRecord / pbSimGetFourPoint,
csrc/pb_fourpoint.hip).

1. tests/fourpoint_ref.py, the reference the GPU tests compare against: it equals a plain double loop in Python ints, and
   it satisfies the identities the header states: the zero vector, lag 0 against the coherent recorder's reference, a
   radius of 0, the time correlation's overlap on dyadic positions.
2. The recipe of tests/test_gpu_fourpoint.py mixes overlapping and non-overlapping bots in every wave, makes Q fluctuate
   and, on the dyadic grid, holds exact ties.
3. four_point_summary on known integers.
4. The C-ABI entries are declared, exported and reject bad arguments before they touch the device.
5. The runner knows --fourpoint and its options and refuses them on the legacy engine; the host library's wrappers
   refuse on the placement-only host engine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import coherent_ref as CR
import fourpoint_ref as FR
import sfactor_ref as KR
import timecorr_ref as TR
from test_runner_analysis_flags import USAGE
from test_scatter_api import TOP, dyadic_positions, vector_list
from test_series_api import CORNER, recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
RADIUS = 0.25
WALK_SIZES = [63, 64, 65, 255, 256, 257, 1000]


# ---- what tests/test_gpu_fourpoint.py records --------------------------------------------------------------------------

def walk(start, seed, records):
    """`records` positions: `start`, then every bot stepped, record after record, by a multiple of 1/64 within +-1/4 per
    axis of its own."""
    rng = np.random.default_rng(seed)
    out = [np.asarray(start, f32)]
    for _ in range(records - 1):
        out.append((out[-1] + rng.integers(-16, 17, size=out[-1].shape).astype(f32) / f32(64.0)).astype(f32))
    return out


def walk_records(n, center=(0.0, 0.0), records=7):
    """The recipe of n bots and a random walk of every bot on its own: unlike a rigid shift, some bots of an origin stay
    within RADIUS and some do not."""
    return walk(recipe(n, center)[0], 7000 + n, records)


def dyadic_walk(records=7):
    """The same walk from positions on the grid of 1/64: every difference is exact in fp32, and some have a length of
    exactly RADIUS."""
    return walk(dyadic_positions(257), 7000 + 257, records)


# ---- 1. the reference --------------------------------------------------------------------------------------------------

def plain_loop(records, steps, lags, radius, vectors, box_log2):
    """The definition, bot by bot in Python ints."""
    tab = KR.table()
    quant = lambda v: int(np.rint(np.float64(v) * 2.0 ** 20))  # float64: exact, ties to even
    qa = int(np.rint(np.float64(f32(radius)) * 2.0 ** 20))
    snaps = [[(quant(x), quant(y)) if abs(x) < 2048.0 and abs(y) < 2048.0 else None for x, y in np.asarray(p, f32)]
             for p in records]
    rows = [[dict(dict.fromkeys(FR.FIELDS, 0), lag=l, nx=int(nx), ny=int(ny)) for nx, ny in vectors] for l in range(lags)]
    for r in range(len(snaps)):
        for l in range(min(r, lags - 1) + 1):
            pairs = [(a, b) for a, b in zip(snaps[r], snaps[r - l]) if a is not None and b is not None]
            slow = [b for a, b in pairs if (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 < qa * qa]
            for row in rows[l]:
                a = b = 0
                for qx, qy in slow:
                    u = (row["nx"] * qx + row["ny"] * qy) & 0xFFFFFFFF
                    t = (u << (12 - box_log2)) & 0xFFFFFFFF
                    idx = (((t + 0x80000) & 0xFFFFFFFF) >> 20) & 4095
                    a += int(tab[idx, 0])
                    b += int(tab[idx, 1])
                row["origins"] += 1
                row["sum_steps"] += steps[r] - steps[r - l]
                row["samples"] += len(pairs)
                row["overlap"] += len(slow)
                row["overlap2"] += len(slow) ** 2
                row["re"] += a
                row["im"] += b
                row["power"] += a * a + b * b
    return rows


def test_reference_equals_a_plain_double_loop():
    recs = walk_records(65, CORNER, records=5)
    recs[1][17, 0] = np.nan
    recs[3][18, 1] = -2048.0
    vectors = vector_list(3).tolist() + [[0, 0], [-7, 11]]
    assert [TOP, -TOP - 1] in vectors and vectors[0] == vectors[2]
    steps = [0, 4, 9, 15, 16]
    for box in (-8, 3, 12):
        got = FR.table(recs, steps, 3, RADIUS, vectors, box)
        assert got == plain_loop(recs, steps, 3, RADIUS, vectors, box), box
        assert all(tuple(g) == FR.FIELDS for row in got for g in row)
    assert [row[0]["origins"] for row in got] == [5, 4, 3] and [row[0]["sum_steps"] for row in got] == [0, 16, 27]
    # bot 17 is missing from the pairs with record 1, bot 18 from those with record 3
    assert [row[0]["samples"] for row in got] == [5 * 65 - 2, 4 * 65 - 4, 3 * 65 - 2]  # (lag 2 pairs record 3 with record 1)
    assert got[0][0]["overlap"] == got[0][0]["samples"]  # a measured bot overlaps itself
    assert 0 < got[1][0]["overlap"] < got[1][0]["samples"] and 0 < got[2][0]["overlap"] < got[1][0]["overlap"]
    assert all(all(g[k] == row[0][k] for k in ("samples", "overlap", "overlap2")) for row in got for g in row)
    assert got[1][0] == got[1][2] and got[1][0]["im"] != 0  # the repeated vector


def test_the_zero_vector_counts_the_overlapping_bots():
    recs = walk_records(257, (1.5, -2.25))
    for box in (-8, 3, 12):
        rows = FR.table(recs, range(7), 3, RADIUS, [(0, 0), (1, 0)], box)
        for lag in rows:
            assert lag[0]["re"] == lag[0]["overlap"] << 30 and lag[0]["im"] == 0
            assert lag[0]["power"] == lag[0]["overlap2"] << 60
            assert lag[1]["power"] <= lag[1]["overlap2"] << 60 and lag[1]["power"] != lag[0]["power"]


def test_lag_zero_is_the_coherent_recorders_lag_zero():
    recs = walk_records(257, (1.5, -2.25), records=4)
    vectors = vector_list(65)
    for radius in (RADIUS, 2.0 ** -20, float(np.nextafter(f32(2048.0), f32(0.0)))):  # qa >= 1: a bot overlaps itself
        rows = FR.table(recs, range(4), 2, radius, vectors, 3)
        want = CR.table(recs, range(4), 2, vectors, 3)
        assert [r["power"] for r in rows[0]] == [r["re"] for r in want[0]]
        assert all(r["samples"] == r["overlap"] == 4 * 257 and r["overlap2"] == 4 * 257 * 257 for r in rows[0])
        modes = [CR.modes(p, vectors, 3)[1] for p in recs]
        assert [(r["re"], r["im"]) for r in rows[0]] == [tuple(sum(m[k][c] for m in modes) for c in (0, 1))
                                                          for k in range(65)]


def test_radius_zero_overlaps_nothing_and_still_counts_the_samples():
    recs = walk_records(65)
    recs[2][5, 1] = np.inf
    rows = FR.table(recs, range(7), 3, 0.0, vector_list(3), 3)
    for l, lag in enumerate(rows):
        for r in lag:
            assert (r["overlap"], r["overlap2"], r["re"], r["im"], r["power"]) == (0, 0, 0, 0, 0)
            assert r["samples"] == (7 - l) * 65 - (1 if l == 0 else 2) and r["origins"] == 7 - l


def test_overlap_is_the_time_correlations_on_dyadic_positions():
    recs = dyadic_walk()
    zeros = np.zeros((257, 2), f32)
    for radius in (RADIUS, 0.3125, 0.015625):
        rows = FR.table(recs, range(7), 3, radius, [(1, 0)], 3)
        want = TR.table([(p, zeros) for p in recs], range(7), 3, radius)
        assert [r[0]["overlap"] for r in rows] == [w["overlap"] for w in want]
        assert [r[0]["samples"] for r in rows] == [w["samples"] for w in want] == [7 * 257, 6 * 257, 5 * 257]


# ---- 2. the recipe -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", WALK_SIZES)
@pytest.mark.parametrize("where", ["origin", "corner"])
def test_the_walk_mixes_every_wave_and_makes_the_overlap_fluctuate(n, where):
    recs = walk_records(n, CORNER if where == "corner" else (0.0, 0.0))
    assert all(np.all(np.abs(p) < 2048.0) for p in recs)
    per_lag = FR.overlaps(recs, 3, RADIUS)
    assert [len(o) for o in per_lag] == [7, 6, 5]
    for lag in (1, 2):
        for m, q, w in per_lag[lag]:
            assert m == n
            # every 64-bot chunk in original order: a wave's staging ballot is neither 0 nor full (the one-bot tail of
            # 65 and 257 can only be one of the two)
            for c in range(0, n - 1, 64):
                if len(w[c:c + 64]) > 1:
                    assert 0 < int(w[c:c + 64].sum()) < len(w[c:c + 64]), (n, where, lag, c)
    assert len({q for _, q, _ in per_lag[1]}) >= 4  # chi_4 != 0
    rows = FR.table(recs, range(7), 3, RADIUS, [(0, 0)], 3)
    o, q, q2 = rows[1][0]["origins"], rows[1][0]["overlap"], rows[1][0]["overlap2"]
    assert q2 * o - q * q > 0


def test_the_dyadic_walk_holds_exact_ties():
    recs = dyadic_walk()
    assert all(np.array_equal(p * 64, np.rint(p * 64)) for p in recs)  # on the grid of 1/64
    qa = FR.qa_of(RADIUS)
    assert qa == 1 << 18
    ties = []
    for lag in (1, 2):
        count = 0
        for r in range(lag, 7):
            d = np.rint((recs[r].astype(np.float64) - recs[r - lag].astype(np.float64)) * 2.0 ** 20).astype(np.int64)
            count += int(((d * d).sum(1) == qa * qa).sum())
        ties.append(count)
    print("ties at lags 1 and 2:", ties)
    assert ties[0] > 0 and ties[1] > 0
    # a tie does not overlap: one quantum more of radius and it does
    rows = FR.table(recs, range(7), 3, RADIUS, [(0, 0)], 3)
    more = FR.table(recs, range(7), 3, RADIUS + 2.0 ** -20, [(0, 0)], 3)
    assert [m[0]["overlap"] - r[0]["overlap"] for r, m in zip(rows, more)][1:] == ties


# ---- 3. the summary ----------------------------------------------------------------------------------------------------

def test_four_point_summary_on_known_integers():
    import particlerobotsimulations_amd as pb
    u = 1 << 30
    # four origins of 10 measured bots: Q = 2, 4, 4, 6.  <Q> = 4, <Q^2> = 18, chi_4 = (18 - 16) / 10
    base = {"lag": 1, "origins": 4, "sum_steps": 48, "samples": 40, "overlap": 16, "overlap2": 72}
    zero = dict(base, nx=0, ny=0, re=16 * u, im=0, power=72 * u * u)
    # a vector whose modes were (2u, 0), (0, 4u), (-4u, 0), (0, -6u): <|W|^2> = 18, <W> = (-2 - 2i) / 4
    wave = dict(base, nx=1, ny=0, re=-2 * u, im=-2 * u, power=72 * u * u)
    s = pb.four_point_summary([zero, wave])
    assert s == {"mean_overlap": 0.4, "chi4": 0.2, "s4": [0.2, (18 - 0.5) / 10], "mean_lag_steps": 12.0}
    assert pb.four_point_summary(zero) == dict(s, s4=[0.2])  # one row alone
    # formed as exact fractions from integers past 2^128
    big = dict(base, nx=0, ny=0, origins=3, samples=3 * ((1 << 28) - 1), overlap=3 * ((1 << 28) - 1),
               overlap2=3 * ((1 << 28) - 1) ** 2, re=3 * ((1 << 28) - 1) * u, im=0, power=3 * ((1 << 28) - 1) ** 2 * u * u + 3)
    s = pb.four_point_summary([big])
    assert s["chi4"] == 0.0 and s["mean_overlap"] == 1.0 and s["s4"] == [9.0 / (9 * ((1 << 28) - 1) * (1 << 60))]
    none = pb.four_point_summary([dict.fromkeys(FR.FIELDS, 0)])
    assert none == {"mean_overlap": None, "chi4": None, "s4": [None], "mean_lag_steps": None}
    unmeasured = pb.four_point_summary([dict(dict.fromkeys(FR.FIELDS, 0), origins=2, sum_steps=10)])
    assert unmeasured == {"mean_overlap": None, "chi4": None, "s4": [None], "mean_lag_steps": 5.0}
    # on the reference's rows: the zero vector's S_4 is chi_4
    rows = FR.table(walk_records(257), range(7), 3, RADIUS, [(0, 0), (1, 0)], 3)
    for lag in rows[1:]:
        s = pb.four_point_summary(lag)
        assert s["chi4"] > 0.0 and s["s4"][0] == s["chi4"] and s["s4"][1] > 0.0 and 0.0 < s["mean_overlap"] < 1.0
    assert pb.four_point_summary(rows[0])["chi4"] == 0.0  # at lag 0 every bot overlaps: nothing fluctuates


def test_rows_compose_from_their_limbs():
    from particlerobotsimulations_amd import _capi
    ones = (1 << 64) - 1
    assert FR.limbs(-1, 2) == [ones, ones] and FR.limbs(1 << 64, 2) == [0, 1] and FR.limbs(-(1 << 64), 2) == [0, ones]
    for v in (0, 1, -1, (1 << 89) - 1, -(1 << 89), (1 << 127) - 1, -(1 << 127)):
        assert _capi.signed_128(FR.limbs(v, 2)) == v, v
    most = ((1 << 31) - 1) * 2 * ((1 << 58) - 1) ** 2  # the largest power there is: below 2^148
    row = _capi.pbFourPointRow(lag=2, nx=-2, ny=5, reserved=9, origins=5, sum_steps=60, samples=50, overlap=16,
                               overlap2=(C.c_ulonglong * 2)(7, 3), re=(C.c_ulonglong * 2)(*FR.limbs(-3 << 70, 2)),
                               im=(C.c_ulonglong * 2)(*FR.limbs(5, 2)), power=(C.c_ulonglong * 3)(*FR.limbs(most, 3)),
                               reserved2=11)
    d = _capi.four_point_row(row)
    assert d == {"lag": 2, "nx": -2, "ny": 5, "origins": 5, "sum_steps": 60, "samples": 50, "overlap": 16,
                 "overlap2": 7 + (3 << 64), "re": -3 << 70, "im": 5, "power": most}
    assert tuple(d) == FR.FIELDS
    assert _capi.FOUR_POINT_ROW_DTYPE.itemsize == 128
    as_record = np.frombuffer(bytes(row), _capi.FOUR_POINT_ROW_DTYPE)[0]
    assert int(as_record["samples"]) == 50 and [int(v) for v in as_record["power"]] == FR.limbs(most, 3)


# ---- 4. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimSetFourPoint", "pbSimFourPointRecord", "pbSimGetFourPointInfo", "pbSimGetFourPoint",
         "pbSimGetFourPointTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _analysis, _capi, host
    import particlerobotsimulations_amd as pb
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbFourPointRow) == 128
    assert "typedef struct pbFourPointRow {        /* 128 bytes */" in header
    for line in ("#define PB_FOURPOINT_MAX_LAGS 64u", "#define PB_FOURPOINT_MAX_VECTORS 256u",
                 "#define PB_FOURPOINT_BLOCKS 256u"):
        assert line in header
    assert (_capi.FOURPOINT_MAX_LAGS, _capi.FOURPOINT_MAX_VECTORS) == (64, 256)
    csrc = os.path.join(ROOT, "particlerobotsimulations_amd", "csrc")
    source = open(os.path.join(csrc, "pb_fourpoint.hip")).read()
    assert "static_assert(sizeof(pbFourPointRow) == 128" in source and '#include "pb_fourpoint.hpp"' in source
    arithmetic = open(os.path.join(csrc, "pb_fourpoint.hpp")).read()
    for word in ('#include "pb_coherent.hpp"', "pbCohMul", "pbCohSum", "pbCohAdd", "pbFpOverlaps"):
        assert word in arithmetic
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert " pb_fourpoint.hip" in makefile and " pb_fourpoint.hpp" in makefile
    for name in ("pbHostSetFourPoint", "pbHostFourPointRecord", "pbHostFourPointInfo", "pbHostFourPointRows"):
        assert hasattr(host.lib(), name)
    for name in ("set_four_point", "four_point_record", "four_point_info", "four_point", "four_point_times"):
        assert hasattr(pb.Sim, name) and hasattr(pb.Ensemble, name)
    assert "four_point_summary" in pb.__all__
    assert [k for k, _ in _analysis.FOUR_POINT_INFO] == ["interval", "lags", "overlap_radius", "box_log2", "nvec",
                                                         "records"]
    block = header.split("Four-point dynamics on the device")[1].split("#define PB_FOURPOINT_MAX_LAGS")[0]
    flat = re.sub(r"\s*\n \* ", " ", block)
    for word in ("chi_4", "S_4(k, tau)", "squared exactly once per origin", "(INT32_MIN, 0)", "MEASURED iff both instants are",
                 "rint(overlapRadius * 1048576.0f)", "dqx^2 + dqy^2 < a2", "below 2^62", "QUANTISED positions",
                 "does not overlap", "EARLIER position", "overlap2 += Q^2", "power += A^2 + B^2", "sum Q < 2^59",
                 "sum Q^2 < 2^87", "sums below 2^89", "sum < 2^148", "a lag holds 2^31 origins or more",
                 "derived, not measured", "two position quanta",
                 "distinct van Hove, coherent scattering, four-point; then the centroid trail",
                 "never waits for the device", "not part of a checkpoint", "(64 + 16)", "2^33 bytes", "65535 members",
                 "2^28 bots", "the phasor at the later position", "weights other than the overlap", "mobility",
                 "logarithmic lags", "radial averaging", "summary rows", "legacy engine"):
        assert word in block or word in flat, word
    assert "pbSimSetCoherent, below" not in flat
    # the two lists that used to name chi_4 as out of scope point here now, and the order sentence names the recorder
    whole = re.sub(r"\s*\n \* ", " ", header)
    assert whole.count("pbSimSetFourPoint, further below") == 1 and "are pbSimSetFourPoint's, next" in whole
    assert "Out of scope: chi_4; weights other than 1" not in whole and "256-bit products); chi_4;" not in whole
    assert whole.count("distinct van Hove, coherent scattering, four-point; then the centroid trail") == 2


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    lib = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    row = _capi.pbFourPointRow(lag=7, samples=7)
    vec = (C.c_int * 4)(1, 0, 0, 1)
    i, l, a, e, k, r, ms = (C.c_float(7.0), C.c_uint(7), C.c_float(7.0), C.c_int(7), C.c_uint(7), C.c_ulonglong(7),
                            C.c_float(7.0))

    def refused(rc, fn, word=None):
        msg = lib.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and fn.encode() in msg and (word is None or word.encode() in msg), (rc, msg)

    fn = "pbSimSetFourPoint"
    refused(lib.pbSimSetFourPoint(None, 0.05, 8, 0.5, 3, vec, 2), fn, "null")
    refused(lib.pbSimSetFourPoint(fake, 0.05, 8, 0.5, 3, None, 2), fn, "null vectors")
    for bad in (-0.5, -2.0, -1e-30, np.nextafter(f32(-1.0), f32(0.0)), float("nan"), float("inf"), float("-inf")):
        refused(lib.pbSimSetFourPoint(fake, float(bad), 8, 0.5, 3, vec, 2), fn, "interval")
        refused(lib.pbSimSetFourPoint(fake, float(bad), 0, 0.5, 3, vec, 2), fn, "interval")  # switching off checks it too
    for bad in (65, 1 << 31):
        refused(lib.pbSimSetFourPoint(fake, 0.05, bad, 0.5, 3, vec, 2), fn, "lags")
        refused(lib.pbSimSetFourPoint(fake, -1.0, bad, 0.5, 3, vec, 2), fn, "lags")  # -1 is an interval
    for bad in (-1e-30, -1.0, 2048.0, 1e9, float("nan"), float("inf"), float("-inf")):
        refused(lib.pbSimSetFourPoint(fake, 0.0, 8, bad, 3, vec, 2), fn, "overlapRadius")
    for bad in (-9, 13, -(1 << 31), (1 << 31) - 1):
        refused(lib.pbSimSetFourPoint(fake, 0.0, 8, 0.5, bad, vec, 2), fn, "boxLog2")
    for bad in (0, 257, 1 << 31):
        refused(lib.pbSimSetFourPoint(fake, 0.0, 8, 0.5, 3, vec, bad), fn, "nvec")
    refused(lib.pbSimFourPointRecord(None), "pbSimFourPointRecord", "null")
    refused(lib.pbSimGetFourPointInfo(None, C.byref(i), C.byref(l), C.byref(a), C.byref(e), C.byref(k), C.byref(r)),
            "pbSimGetFourPointInfo", "null")
    refused(lib.pbSimGetFourPointInfo(fake, None, None, None, None, None, None), "pbSimGetFourPointInfo", "all null")
    refused(lib.pbSimGetFourPoint(None, C.byref(row)), "pbSimGetFourPoint", "null")
    refused(lib.pbSimGetFourPoint(fake, None), "pbSimGetFourPoint", "null")
    refused(lib.pbSimGetFourPointTimes(None, C.byref(r), C.byref(ms)), "pbSimGetFourPointTimes", "null")
    assert (i.value, l.value, a.value, e.value, k.value, r.value, ms.value) == (7.0, 7, 7.0, 7, 7, 7, 7.0)
    assert row.lag == 7 and row.samples == 7


# ---- 5. the runner and the other engines -------------------------------------------------------------------------------

NOT_A_NUMBER = ["", "abc", "-1", "-1e-30", "nan", "inf", "-inf", "0.1x"]
BAD_FLAGS = ([("--fourpoint-interval", v) for v in NOT_A_NUMBER]
             + [("--fourpoint-lags", v) for v in ("", "0", "-3", "1.5", "65", "many")]
             + [("--fourpoint-overlap", v) for v in NOT_A_NUMBER + ["2048", "1e9"]]
             + [("--fourpoint-box-log2", v) for v in ("", "-9", "13", "1.5", "big")]
             + [("--fourpoint-nmax", v) for v in ("", "0", "-1", "11", "2.5", "all")])  # 11: 265 vectors, past 256


@pytest.mark.parametrize("flag,value", BAD_FLAGS, ids=[f"{f}={v!r}" for f, v in BAD_FLAGS])
def test_runner_refuses_a_bad_fourpoint_value(tmp_path, flag, value):
    for args in ([flag, value], [CFG, "--fourpoint", "f.csv", flag, value, "--quiet"]):
        r = subprocess.run([RUN] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), args
    assert not os.listdir(tmp_path)


def test_runner_fourpoint_flags_need_their_values_and_the_fused_engine(tmp_path):
    flags = ("--fourpoint", "--fourpoint-interval", "--fourpoint-lags", "--fourpoint-overlap", "--fourpoint-box-log2",
             "--fourpoint-nmax")
    for flag in flags:
        r = subprocess.run([RUN, CFG, flag], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), flag
    said = "--fourpoint needs the fused engine (the recorder runs on its resident state)\n"
    for extra in ([], ["--fourpoint-interval", "0"], ["--fourpoint-interval", "3.4e38", "--fourpoint-lags", "1"],
                  ["--fourpoint-lags", "64", "--fourpoint-nmax", "10"], ["--fourpoint-box-log2", "-8"],
                  ["--fourpoint-overlap", "0"], ["--fourpoint-overlap", "2047.9", "--fourpoint-nmax", "1"]):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--fourpoint", "f.csv"] + extra, capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", said), extra
    # last in the engine-check table: any earlier file flag speaks first
    for flag, line in (("--scatter", "--scatter needs the fused engine (the recorder runs on its resident state)\n"),
                       ("--coherent", "--coherent needs the fused engine (the recorder runs on its resident state)\n")):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--fourpoint", "f.csv", flag, "a.csv"], capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stderr) == (2, line)
    assert not os.listdir(tmp_path)
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_runner.cpp")).read()
    for flag in ("--fourpoint FILE", "--fourpoint-interval T", "--fourpoint-lags N", "--fourpoint-overlap A",
                 "--fourpoint-box-log2 E", "--fourpoint-nmax M"):
        assert flag in source and flag in open(os.path.join(ROOT, "README.md")).read(), flag
        assert flag.split()[0] in open(os.path.join(ROOT, "INTEGRATION.md")).read(), flag
    assert "Lag, Nx, Ny, Origins, SumSteps, Samples, Overlap, Overlap2, Re, Im, Power, Chi4, S4" in source
    assert "fourpoint" not in USAGE  # the usage line stays as it is


NEEDS = "the four-point recorder needs the fused engine"
VEC = (C.c_int * 2)(1, 0)
REFUSED = [  # the host library's wrappers (HostSim has no methods for this recorder: a caller goes through host.lib())
    (lambda L, h: L.pbHostSetFourPoint(h, 0.05, 8, 0.5, 3, VEC, 1), "Particlebot::setFourPoint: " + NEEDS + "\n"),
    (lambda L, h: L.pbHostFourPointRecord(h), "Particlebot::fourPointRecord: " + NEEDS + "\n"),
    (lambda L, h: L.pbHostFourPointInfo(h, None, C.byref(C.c_uint(7)), None, None, None, None),
     "Particlebot::fourPointInfo: " + NEEDS + "\n"),
]


@pytest.mark.parametrize("call,line", REFUSED, ids=["set", "record", "info"])
def test_host_engine_has_no_four_point_recorder(capfd, call, line):
    from particlerobotsimulations_amd import _capi, host
    h = host.HostSim(CFG, engine="host")  # (the legacy engine needs a device: tests/test_gpu_fourpoint.py asks it)
    capfd.readouterr()
    lib = host.lib()
    assert call(lib, h._h) == -1
    assert capfd.readouterr() == ("", line)
    # a NULL list with a count, and a NULL count, are refused before the class is asked; a refused call writes nothing
    assert lib.pbHostSetFourPoint(h._h, 0.05, 8, 0.5, 3, None, 1) == -1 and lib.pbHostFourPointRows(h._h, None, 0, None) == -1
    assert capfd.readouterr() == ("", "")
    row, count = _capi.pbFourPointRow(lag=7), C.c_ulonglong(7)
    assert lib.pbHostFourPointRows(h._h, C.byref(row), 1, C.byref(count)) == -1 and (row.lag, count.value) == (7, 7)
    assert capfd.readouterr() == ("", "Particlebot::fourPointRows: " + NEEDS + "\n")
    h.close()
