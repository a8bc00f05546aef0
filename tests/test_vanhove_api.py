"""CPU side of the self van Hove function (pbSimSetVanHove / pbSimVanHoveRecord / pbSimGetVanHove, csrc/pb_vanhove.hip).

1. tests/vanhove_ref.py, the reference the GPU tests compare against: it equals a plain per-bot loop, gives hand-built
   known answers, agrees with tests/timecorr_ref.py on msd and samples, and drops exactly the unmeasured pairs.
2. The recipe of tests/test_gpu_vanhove.py fills a histogram: conditions on the inputs.
3. The C-ABI entries are declared, exported and reject bad arguments before they touch the device.
4. The runner knows --vanhove and its options; the placement-only host engine has no van Hove function.
5. van_hove_row and van_hove_summary on known integers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import timecorr_ref as TR
import vanhove_ref as VR
from test_runner_analysis_flags import USAGE
from test_series_api import recipe
from test_timecorr_api import BELOW, manual_records, unmeasured_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
ONE = 1 << 20
U = 2.0 ** -20
TOP = (1 << 31) - 128

# ---- what tests/test_gpu_vanhove.py records ----------------------------------------------------------------------------

MANUAL_LAGS, MANUAL_RECORDS = 3, 7
# a rigid shift per record on top of the per-bot steps, alternating so that nothing drifts: the lag-1 displacement of an
# axis spans [-4.25, 4.25] (68 bins of 0.125) and its length stays below 4.25 sqrt(2) < 8
RIGID = [(1.25, -1.25), (-1.25, 1.25)]
STEP = 3.0


def vanhove_records(n, records=MANUAL_RECORDS, center=(0.0, 0.0)):
    """`records` states of the recipe, as the time-correlation test's manual_records, but broad enough to fill a
    histogram: from one record to the next every bot takes a step of its own, a multiple of 2^-10 drawn uniformly in
    [-3, 3] per axis, on top of the rigid shift RIGID[k % 2]; velocities change by a multiple of 2^-6.  Returns
    [(pos, vel, rad)]."""
    pos, vel, rad = recipe(n, center)
    rng = np.random.default_rng(7000 + n)
    out = [(pos, vel, rad)]
    for k in range(1, records):
        step = rng.integers(-int(STEP * 1024), int(STEP * 1024) + 1, size=(n, 2)).astype(f32) / f32(1024.0)
        dv = rng.integers(-4, 5, size=(n, 2)).astype(f32) / f32(64.0)
        pos = (pos + np.array(RIGID[k % 2], f32) + step).astype(f32)
        out.append((pos, (vel + dv).astype(f32), rad))
    return out


KNOWN_WIDTH, KNOWN_BINS = 0.125, 8
QW = ONE // 8
# (dx, dy) of eight bots between two records
KNOWN_MOVES = [(0.375, 0.0),         # exactly 3 widths: the edge belongs to the upper bin, radial 3, x index 3 + 8
               (0.375 - U, 0.0),     # one quantum less: radial 2, x index 2 + 8
               (0.0, 0.0),           # at rest: radial 0, x and y index 8
               (-0.125, 0.0),        # minus one width: floor -1, x index 7; radial 1
               (-0.125 - U, 0.0),    # one quantum further: floor -2, x index 6; radial 1
               (1.0, 0.0),           # exactly bins widths: beyond in r and in x
               (0.0, -1.0),          # the lowest edge of y is inside: y index 0; beyond in r
               (0.0, -1.0 - U)]      # one quantum further: beyond in y too


def known_answer_records():
    then = np.array([[0.5 * k, 3.0 - 0.5 * k] for k in range(8)], f32)
    now = (then + np.array(KNOWN_MOVES, f32)).astype(f32)
    return [then, now]


def known_answer_rows():
    """The two rows of known_answer_records() with steps 0 and 10, written out by hand."""
    s = [(3 * QW) ** 2, (3 * QW - 1) ** 2, 0, QW ** 2, (QW + 1) ** 2, ONE ** 2, ONE ** 2, (ONE + 1) ** 2]
    lag0 = dict(VR.empty_row(0, 8), origins=2, samples=16, radial=[16] + [0] * 7,
                x=[0] * 8 + [16] + [0] * 7, y=[0] * 8 + [16] + [0] * 7)
    lag1 = dict(VR.empty_row(1, 8), origins=1, sum_steps=10, samples=8, beyond_r=3, beyond_x=1, beyond_y=1,
                msd=sum(s), q4=sum(v * v for v in s),
                radial=[1, 2, 1, 1, 0, 0, 0, 0],
                x=[0, 0, 0, 0, 0, 0, 1, 1, 3, 0, 1, 1, 0, 0, 0, 0],
                y=[1, 0, 0, 0, 0, 0, 0, 0, 6, 0, 0, 0, 0, 0, 0, 0])
    return [lag0, lag1]


def unmeasured_positions():
    """The positions of the time-correlation test's unmeasured_records(): NaN and the infinities in x and y at either
    instant, |dx| and |dy| exactly 2048, and just below.  Its out-of-range velocities do not matter here.  Returns the
    two position arrays, the bots unmeasured at lag 1 and per record the bots unmeasured at lag 0."""
    recs, _, _ = unmeasured_records()
    p = [recs[0][0], recs[1][0]]
    with np.errstate(invalid="ignore"):
        bad0 = [sorted(np.nonzero(~np.isfinite(q).all(1))[0]) for q in p]
        d = p[1] - p[0]
        bad1 = sorted(np.nonzero(~(np.abs(d) < f32(2048.0)).all(1))[0])
    return p, bad1, bad0


# ---- 1. the reference --------------------------------------------------------------------------------------------------

def plain_table(records_pos, steps, lags, width, bins):
    """The definition as a loop over records, lags and bots in Python floats and ints, with the edges walked one by one."""
    qw = int(np.rint(f32(width) * f32(1048576.0)))
    rows = [VR.empty_row(l, bins) for l in range(lags)]
    for r in range(len(records_pos)):
        for l in range(min(r, lags - 1) + 1):
            row = rows[l]
            row["origins"] += 1
            row["sum_steps"] += steps[r] - steps[r - l]
            for (xn, yn), (xt, yt) in zip(records_pos[r], records_pos[r - l]):
                with np.errstate(invalid="ignore"):
                    dx, dy = f32(xn) - f32(xt), f32(yn) - f32(yt)
                if not (abs(dx) < 2048.0 and abs(dy) < 2048.0):
                    continue
                qx, qy = int(np.rint(f32(dx * f32(1048576.0)))), int(np.rint(f32(dy * f32(1048576.0))))
                s = qx * qx + qy * qy
                row["samples"] += 1
                row["msd"] += s
                row["q4"] += s ** 2
                k = 0
                while k < bins and min(((k + 1) * qw) ** 2, 1 << 63) <= s:
                    k += 1
                if k < bins:
                    row["radial"][k] += 1
                else:
                    row["beyond_r"] += 1
                for name, q in (("x", qx), ("y", qy)):
                    b = q // qw if q >= 0 else -((-q + qw - 1) // qw)  # (non-negative operands only: no rounding rule)
                    if -bins <= b < bins:
                        row[name][b + bins] += 1
                    else:
                        row["beyond_" + name] += 1
    return rows


@pytest.mark.parametrize("width,bins", [(0.125, 64), (0.3, 1024), (2.0 ** -20, 1), (2047.5, 2), (0.125, 16)])
def test_reference_equals_a_plain_loop(width, bins):
    recs = [r[0] for r in vanhove_records(65, records=5)]
    steps = [0, 3, 4, 10, 11]
    got = VR.table(recs, steps, 3, width, bins)
    assert got == plain_table(recs, steps, 3, width, bins)
    assert all(VR.identities_hold(r) for r in got)
    assert [r["origins"] for r in got] == [5, 4, 3] and [r["sum_steps"] for r in got] == [0, 11, 18]
    assert [r["samples"] for r in got] == [5 * 65, 4 * 65, 3 * 65]


def test_edges_saturate_and_belong_to_the_upper_bin():
    assert VR.qw_of(0.125) == QW and VR.qw_of(2.0 ** -20) == 1 and VR.qw_of(2047.5) == 2047.5 * ONE
    assert VR.edges_of(QW, 3) == [0, QW ** 2, 4 * QW ** 2, 9 * QW ** 2]
    big = VR.edges_of(VR.qw_of(2047.5), 2)
    assert big == [0, (2047.5 * ONE) ** 2, 1 << 63]  # (2 x 2047.5 x 2^20)^2 is above 2^63: saturated
    row = VR.empty_row(0, 2)
    VR.add_pair(row, TOP, TOP, VR.qw_of(2047.5), 2, big)  # the largest s there is: below 2^63, so inside bin 1
    assert row["radial"] == [0, 1] and row["beyond_r"] == 0 and row["x"] == [0, 0, 0, 1]


def test_known_answers():
    rows = VR.table(known_answer_records(), [0, 10], 2, KNOWN_WIDTH, KNOWN_BINS)
    assert rows == known_answer_rows()
    assert all(VR.identities_hold(r) for r in rows)


def test_second_moment_is_the_time_correlation_s():
    recs = manual_records(257) + vanhove_records(257, records=3)[1:]  # narrow and broad; every velocity in range
    steps = list(range(0, 5 * len(recs), 5))
    tc = TR.table([(p, v) for p, v, _ in recs], steps, 4, 0.5)
    vh = VR.table([p for p, _, _ in recs], steps, 4, 0.25, 32)
    for a, b in zip(tc, vh):
        assert (a["samples"], a["msd"], a["origins"], a["sum_steps"]) == (b["samples"], b["msd"], b["origins"], b["sum_steps"])
        assert b["q4"] <= a["max_q2"] * b["msd"]
    assert vh[1]["msd"] > 0 and vh[1]["q4"] > 0


def test_unmeasured_pairs_take_part_in_nothing():
    p, bad1, bad0 = unmeasured_positions()
    assert len(bad1) == 14 and [len(b) for b in bad0] == [6, 6]
    rows = VR.table(p, [0, 0], 2, 64.0, 32)
    assert rows == plain_table(p, [0, 0], 2, 64.0, 32)
    assert rows[0]["samples"] == 2 * 257 - 12 and rows[1]["samples"] == 257 - 14
    assert all(VR.identities_hold(r) for r in rows)
    # |dx| just below 2048 is measured: qx = 2^31 - 128, bin 31 of width 64, and index 63 of x / index 0 of y
    assert p[1][100][0] == BELOW and p[0][101][1] == BELOW
    assert rows[1]["radial"][31] == 2 and rows[1]["x"][63] == 1 and rows[1]["y"][0] == 1
    assert rows[1]["q4"] >= 2 * TOP ** 4


# ---- 2. the GPU tests' recipe --------------------------------------------------------------------------------------------

def test_the_recipe_fills_the_histogram():
    recs = [r[0] for r in vanhove_records(1000)]
    assert len(recs) == MANUAL_RECORDS
    rows = VR.table(recs, [0] * MANUAL_RECORDS, MANUAL_LAGS, 0.125, 64)
    first, last = rows[1], rows[MANUAL_LAGS - 1]
    occupied = {k: sum(1 for c in first[k] if c) for k in ("radial", "x", "y")}
    print(occupied, first["beyond_r"], last["beyond_r"], last["samples"])
    assert occupied["radial"] >= 32 and occupied["x"] >= 64 and occupied["y"] >= 64 and first["beyond_r"] == 0
    assert 10 * last["beyond_r"] < last["samples"]
    narrow = VR.table(recs, [0] * MANUAL_RECORDS, MANUAL_LAGS, 0.125, 16)[1]
    assert 3 * narrow["beyond_r"] > narrow["samples"]


# ---- 3. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimSetVanHove", "pbSimVanHoveRecord", "pbSimGetVanHoveInfo", "pbSimGetVanHove", "pbSimGetVanHoveTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi, host
    import particlerobotsimulations_amd as pb
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbVanHoveRow) == 96
    assert "pbVanHoveRow" in header
    for line in ("#define PB_VANHOVE_MAX_LAGS 64u", "#define PB_VANHOVE_MAX_BINS 1024u", "#define PB_VANHOVE_BLOCKS 256u"):
        assert line in header
    assert (_capi.VANHOVE_MAX_LAGS, _capi.VANHOVE_MAX_BINS) == (64, 1024)
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_vanhove.hip")).read()
    assert "static_assert(sizeof(pbVanHoveRow) == 96" in source
    for name in ("pbHostSetVanHove", "pbHostVanHoveRecord", "pbHostVanHoveInfo", "pbHostVanHoveRows"):
        assert hasattr(host.lib(), name)
    for name in ("set_van_hove", "van_hove_record", "van_hove_info", "van_hove", "van_hove_times"):
        assert hasattr(pb.Sim, name)
    for name in ("set_van_hove", "van_hove_record", "van_hove_info", "van_hove"):
        assert hasattr(host.HostSim, name)
    assert "van_hove_summary" in pb.__all__


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    row = _capi.pbVanHoveRow(lag=7, samples=7)
    counts = (C.c_ulonglong * 5)(7, 7, 7, 7, 7)
    i, l, w, b, r, ms = C.c_float(7.0), C.c_uint(7), C.c_float(7.0), C.c_uint(7), C.c_ulonglong(7), C.c_float(7.0)

    def refused(rc, fn, word=None):
        msg = L.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and fn.encode() in msg and (word is None or word.encode() in msg), (rc, msg)

    fn = "pbSimSetVanHove"
    refused(L.pbSimSetVanHove(None, 0.05, 8, 0.125, 64), fn, "null")
    for bad in (-0.5, -2.0, -1e-30, np.nextafter(f32(-1.0), f32(0.0)), float("nan"), float("inf"), float("-inf")):
        refused(L.pbSimSetVanHove(fake, float(bad), 8, 0.125, 64), fn, "interval")
        refused(L.pbSimSetVanHove(fake, float(bad), 0, 0.125, 64), fn, "interval")  # switching off checks it too
    for bad in (65, 1 << 31):
        refused(L.pbSimSetVanHove(fake, 0.05, bad, 0.125, 64), fn, "lags")
        refused(L.pbSimSetVanHove(fake, -1.0, bad, 0.125, 64), fn, "lags")  # -1 is an interval
    for bad in (0, 1025, 1 << 31):
        refused(L.pbSimSetVanHove(fake, 0.0, 8, 0.125, bad), fn, "bins")
    for bad in (0.0, -0.125, 2048.0, 1e30, float("nan"), float("inf"), float("-inf")):
        refused(L.pbSimSetVanHove(fake, 0.0, 8, float(bad), 64), fn, "binWidth")
    for bad in (2.0 ** -21, 2.0 ** -22, 1e-30):  # rint(w 2^20) == 0 (a tie goes to even): no quantum
        refused(L.pbSimSetVanHove(fake, 0.0, 8, float(bad), 64), fn, "quantum")
    refused(L.pbSimVanHoveRecord(None), "pbSimVanHoveRecord", "null")
    refused(L.pbSimGetVanHoveInfo(None, C.byref(i), C.byref(l), C.byref(w), C.byref(b), C.byref(r)),
            "pbSimGetVanHoveInfo", "null")
    refused(L.pbSimGetVanHoveInfo(fake, None, None, None, None, None), "pbSimGetVanHoveInfo", "all null")
    refused(L.pbSimGetVanHove(None, C.byref(row), counts), "pbSimGetVanHove", "null")
    refused(L.pbSimGetVanHove(fake, None, None), "pbSimGetVanHove", "both null")
    refused(L.pbSimGetVanHoveTimes(None, C.byref(r), C.byref(ms)), "pbSimGetVanHoveTimes", "null")
    assert (i.value, l.value, w.value, b.value, r.value, ms.value) == (7.0, 7, 7.0, 7, 7, 7.0)
    assert row.lag == 7 and row.samples == 7 and list(counts) == [7] * 5


# ---- 4. the runner and the host engine ---------------------------------------------------------------------------------

NOT_A_NUMBER = ["", "abc", "-1", "-1e-30", "nan", "inf", "-inf", "0.1x"]
BAD_FLAGS = ([("--vanhove-interval", v) for v in NOT_A_NUMBER]
             + [("--vanhove-lags", v) for v in ("", "0", "-3", "1.5", "65", "many")]
             + [("--vanhove-width", v) for v in NOT_A_NUMBER + ["0", "2048", "1e30"]]
             + [("--vanhove-bins", v) for v in ("", "0", "-1", "1025", "2.5", "all")])


@pytest.mark.parametrize("flag,value", BAD_FLAGS, ids=[f"{f}={v!r}" for f, v in BAD_FLAGS])
def test_runner_refuses_a_bad_van_hove_value(tmp_path, flag, value):
    for args in ([flag, value], [CFG, "--vanhove", "f.csv", flag, value, "--quiet"]):
        r = subprocess.run([RUN] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), args
    assert not os.listdir(tmp_path)


def test_runner_van_hove_flags_need_their_values_and_the_fused_engine(tmp_path):
    flags = ("--vanhove", "--vanhove-interval", "--vanhove-lags", "--vanhove-width", "--vanhove-bins")
    for flag in flags:
        r = subprocess.run([RUN, CFG, flag], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), flag
    said = "--vanhove needs the fused engine (the recorder runs on its resident state)\n"
    for extra in ([], ["--vanhove-interval", "0"], ["--vanhove-interval", "3.4e38", "--vanhove-lags", "1"],
                  ["--vanhove-lags", "64", "--vanhove-bins", "1024"], ["--vanhove-width", "1e-6"],
                  ["--vanhove-width", "2047.9", "--vanhove-bins", "1"]):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--vanhove", "f.csv"] + extra, capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", said), extra
    # last in the engine-check table: any earlier analysis flag speaks first
    for flag, line in (("--scatter", "--scatter needs the fused engine (the recorder runs on its resident state)\n"),
                       ("--timecorr", "--timecorr needs the fused engine (the recorder runs on its resident state)\n"),
                       ("--sk", "--sk needs the fused engine (the analysis runs on its resident state)\n")):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--vanhove", "f.csv", flag, "a.csv"], capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stderr) == (2, line)
    assert not os.listdir(tmp_path)
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_runner.cpp")).read()
    for flag in ("--vanhove FILE", "--vanhove-interval T", "--vanhove-lags N", "--vanhove-width W", "--vanhove-bins B"):
        assert flag in source and flag in open(os.path.join(ROOT, "README.md")).read(), flag
        assert flag.split()[0] in open(os.path.join(ROOT, "INTEGRATION.md")).read(), flag
    assert "Lag, Origins, SumSteps, Samples, SumQ2, SumQ4, Alpha2, Axis, Bin, Lower, Count" in source
    assert "vanhove" not in USAGE  # the usage line stays as it is


NEEDS = "the van Hove function needs the fused engine"
REFUSED = [
    (lambda h: h.set_van_hove(0.05, 8, 0.125, 64),
     "set_van_hove: " + NEEDS + ", a finite interval >= 0 (or -1), lags <= 64, a width in (0, 2048) and 1 ... 1024 bins",
     "Particlebot::setVanHove: " + NEEDS + "\n"),
    (lambda h: h.van_hove_record(), "van_hove_record: " + NEEDS + " and the analysis on",
     "Particlebot::vanHoveRecord: " + NEEDS + "\n"),
    (lambda h: h.van_hove_info(), "van_hove_info: " + NEEDS, "Particlebot::vanHoveInfo: " + NEEDS + "\n"),
    (lambda h: h.van_hove(), "van_hove_info: " + NEEDS, "Particlebot::vanHoveInfo: " + NEEDS + "\n"),
]


@pytest.mark.parametrize("call,error,line", REFUSED, ids=["set", "record", "info", "rows"])
def test_host_engine_has_no_van_hove(capfd, call, error, line):
    from particlerobotsimulations_amd import _capi, host
    h = host.HostSim(CFG, engine="host")
    capfd.readouterr()
    with pytest.raises(RuntimeError) as caught:
        call(h)
    assert str(caught.value) == error
    assert capfd.readouterr() == ("", line)
    # the wrapper: a NULL count is refused before the class is asked; a refused call writes nothing
    L = host.lib()
    assert L.pbHostVanHoveRows(h._h, None, None, 0, None) == -1
    assert capfd.readouterr() == ("", "")
    row, counts, count = _capi.pbVanHoveRow(lag=7), (C.c_ulonglong * 5)(7, 7, 7, 7, 7), C.c_ulonglong(7)
    assert L.pbHostVanHoveRows(h._h, C.byref(row), counts, 1, C.byref(count)) == -1
    assert (row.lag, count.value, list(counts)) == (7, 7, [7] * 5)
    assert capfd.readouterr() == ("", "Particlebot::vanHoveRows: " + NEEDS + "\n")
    h.close()


# ---- 5. the pure-Python helpers ----------------------------------------------------------------------------------------

def test_van_hove_row_and_summary_on_known_integers():
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import _capi
    q4 = (5 << 130) + (3 << 64) + 9
    r = _capi.pbVanHoveRow(lag=3, reserved=0, origins=5, sum_steps=60, samples=16, beyond_r=1, beyond_x=2, beyond_y=3,
                           msd=_capi.pbMoment128(lo=7, hi=1 << 40), q4=(C.c_ulonglong * 3)(9, 3, 5 << 2))
    d = _capi.van_hove_row(r)
    assert d == {"lag": 3, "origins": 5, "sum_steps": 60, "samples": 16, "beyond_r": 1, "beyond_x": 2, "beyond_y": 3,
                 "msd": (1 << 72) + 7, "q4": q4}
    assert tuple(d) == VR.FIELDS
    # four bots that each moved by (1, 0): <r^2> = 1, <r^4> = 1, alpha2 = 1 / 2 - 1
    flat = {"samples": 4, "origins": 2, "sum_steps": 30, "msd": 4 << 40, "q4": 4 << 80}
    assert pb.van_hove_summary(flat, 0.5) == {"msd": 1.0, "msd_in_widths": 4.0, "alpha2": -0.5, "mean_lag_steps": 15.0}
    # two of four moved by (2, 0) and two stayed: <r^2> = 2, <r^4> = 8, alpha2 = 8 / 8 - 1 = 0
    half = dict(flat, msd=2 * (4 << 40), q4=2 * (16 << 80))
    assert pb.van_hove_summary(half, 1.0) == {"msd": 2.0, "msd_in_widths": 2.0, "alpha2": 0.0, "mean_lag_steps": 15.0}
    # the known answers' lag 1, from the integers
    row = known_answer_rows()[1]
    s = pb.van_hove_summary(row, KNOWN_WIDTH)
    assert s["msd"] == row["msd"] / 8 / 2.0 ** 40 and s["mean_lag_steps"] == 10.0
    assert s["alpha2"] == pytest.approx(row["q4"] * 8 / (2 * row["msd"] ** 2) - 1, rel=1e-15)
    rest = pb.van_hove_summary(dict(flat, msd=0, q4=0), 0.5)
    assert rest["msd"] == 0.0 and math.isnan(rest["alpha2"])
    none = pb.van_hove_summary(dict.fromkeys(VR.FIELDS, 0), 0.5)
    assert all(math.isnan(v) for v in none.values())
