"""CPU side of the time series (pbSimMoments / pbSimSetSeries / pbSimGetSeriesOf, csrc/pb_moments.hip).

1. tests/series_ref.py, the reference the GPU tests compare against: it equals a plain Python loop, gives hand-built
   known answers, keeps every bot of the GPU tests' recipes measured, and replays the fp32 clock and its gate.
2. The C-ABI entries are declared, exported and reject bad arguments before they touch the device; the runner knows
   --series and its options; the placement-only host engine has no series.
3. moments_summary on known integers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import series_ref as SR
from helpers import jittered_blob
from test_runner_analysis_flags import USAGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
ONE = 1 << 20
BELOW = np.nextafter(f32(2048.0), f32(0.0))

# the recipes of tests/test_gpu_series.py: (bots, centre)
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1025]
CORNER = (-2040.0, 2040.0)


def recipe(n, center=(0.0, 0.0)):
    rng = np.random.default_rng(3000 + n)
    return jittered_blob(n, 0.15, rng, center=center, jitter=0.3)


def known_answer_state():
    """Three bots at (+-2047.5, -+1000) and the origin, moving and of different radii."""
    pos = np.array([[2047.5, -1000.0], [-2047.5, 1000.0], [0.0, 0.0]], f32)
    vel = np.array([[1.5, -2.0], [0.25, 0.5], [0.0, -3.0]], f32)
    rad = np.array([0.125, 0.5, 1.0], f32)
    return pos, vel, rad


def tie_state():
    """Values half way between two integers of the 2^-20 grid: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> -0, -1.5 -> -2."""
    u = 2.0 ** -20
    pos = np.array([[1.5 * u, 2.5 * u], [0.5 * u, -1.5 * u], [-0.5 * u, 3.5 * u]], f32)
    vel = np.array([[2.5 * u, -2.5 * u], [1.5 * u, 0.5 * u], [0.0, 0.0]], f32)
    rad = np.array([1.5 * u, 2.5 * u, 3.5 * u], f32)
    return pos, vel, rad


def unmeasured_state():
    """257 bots of the recipe with one bot of every unmeasured kind: exactly 2048, NaN and an infinity in each of the
    five inputs; and bots just below the bound, which are measured.  Returns the state and the unmeasured indices."""
    pos, vel, rad = recipe(257)
    bad = {}
    for k, (arr, col) in enumerate([(pos, 0), (pos, 1), (vel, 0), (vel, 1), (rad, None)]):
        for j, v in enumerate((2048.0, -2048.0, np.nan, np.inf, -np.inf)):
            i = 10 + 5 * k + j
            if col is None:
                arr[i] = v
            else:
                arr[i, col] = v
            bad[i] = (k, v)
    pos[100, 0], pos[101, 1], vel[102, 0], vel[103, 1], rad[104] = BELOW, -BELOW, BELOW, -BELOW, BELOW
    return pos, vel, rad, sorted(bad)


# ---- 1. the reference --------------------------------------------------------------------------------------------------

def plain_loop(pos, vel, rad):
    """The definition, bot by bot, with the device's two accumulators per 128-bit sum."""
    row = dict.fromkeys(SR.FIELDS, 0)
    acc = {k: [0, 0] for k in SR.SQUARES}  # lo, hi
    box = None
    for (x, y), (vx, vy), r in zip(pos, vel, rad):
        vals = [f32(x), f32(y), f32(vx), f32(vy), f32(r)]
        if not all(np.isfinite(v) and abs(v) < f32(2048.0) for v in vals):
            continue
        qx, qy, wx, wy, qr = (int(np.rint(np.float64(v) * 2.0 ** 20)) for v in vals)  # float64: exact, ties to even
        row["measured"] += 1
        for k, q in (("sum_qx", qx), ("sum_qy", qy), ("sum_qr", qr), ("sum_wx", wx), ("sum_wy", wy)):
            row[k] += q
        for k, p in (("xx", qx * qx), ("yy", qy * qy), ("xy", qx * qy), ("rr", qr * qr), ("vv", wx * wx + wy * wy)):
            assert abs(p) < 1 << 63
            acc[k][0] += p & 0xFFFFFFFF  # (unsigned)p
            acc[k][1] += p >> 32         # arithmetic shift
        box = (qx, qx, qy, qy) if box is None else (min(box[0], qx), max(box[1], qx), min(box[2], qy), max(box[3], qy))
    for k in SR.SQUARES:
        row[k] = (acc[k][1] << 32) + acc[k][0]
    if box:
        row["min_qx"], row["max_qx"], row["min_qy"], row["max_qy"] = box
    return row, acc


def test_reference_equals_a_plain_loop():
    pos, vel, rad = recipe(300)
    pos[17, 0] = np.nan
    vel[18, 1] = 2048.0
    want, acc = plain_loop(pos, vel, rad)
    got = SR.moments(pos, vel, rad)
    assert got == want and got["measured"] == 298 and tuple(got) == SR.FIELDS
    assert all(lo >= 1 << 32 for lo, _ in acc.values())  # the low accumulators carry past 2^32
    assert got["xy"] != 0 and got["min_qx"] < 0 < got["max_qx"]
    pos, vel, rad = recipe(300, CORNER)
    want, acc = plain_loop(pos, vel, rad)
    assert SR.moments(pos, vel, rad) == want
    assert want["xy"] < 0 and acc["xy"][1] < 0 and want["xx"] > 1 << 64 and want["max_qx"] < 0 < want["min_qy"]


def test_known_answer_of_three_bots():
    got = SR.moments(*known_answer_state())
    qx, qy = 4095 << 19, 1000 << 20
    assert got == {
        "measured": 3, "sum_qx": 0, "sum_qy": 0, "sum_qr": ONE // 8 + ONE // 2 + ONE,
        "sum_wx": ONE * 7 // 4, "sum_wy": -ONE * 9 // 2,
        "min_qx": -qx, "max_qx": qx, "min_qy": -qy, "max_qy": qy,
        "xx": 2 * qx * qx, "yy": 2 * qy * qy, "xy": -2 * qx * qy,
        "rr": (ONE // 8) ** 2 + (ONE // 2) ** 2 + ONE ** 2,
        "vv": (ONE * 3 // 2) ** 2 + (2 * ONE) ** 2 + (ONE // 4) ** 2 + (ONE // 2) ** 2 + (3 * ONE) ** 2,
    }
    assert got["xx"] >> 32 > 1 << 30 and got["xy"] < 0  # a high part that matters, a negative signed sum
    assert got == plain_loop(*known_answer_state())[0]


def test_ties_round_to_even():
    pos, vel, rad = tie_state()
    got = SR.moments(pos, vel, rad)
    assert SR.quantise(pos[:, 0])[0] == [2, 0, 0] and SR.quantise(pos[:, 1])[0] == [2, -2, 4]
    assert SR.quantise(rad)[0] == [2, 2, 4] and SR.quantise(vel[:, 0])[0] == [2, 2, 0]
    assert got == plain_loop(pos, vel, rad)[0]
    assert (got["sum_qx"], got["sum_qy"], got["sum_qr"], got["xx"], got["yy"], got["xy"]) == (2, 4, 8, 4, 24, 4)


def test_unmeasured_bots_take_part_in_nothing():
    pos, vel, rad, bad = unmeasured_state()
    assert len(bad) == 25
    got = SR.moments(pos, vel, rad)
    keep = np.setdiff1d(np.arange(257), bad)
    assert got["measured"] == 257 - 25 and got == SR.moments(pos[keep], vel[keep], rad[keep])
    assert got == plain_loop(pos, vel, rad)[0]
    top = (1 << 31) - 128  # the largest q there is
    assert got["max_qx"] == top and got["min_qy"] == -top
    # each kind on its own
    base = recipe(8)
    for arr in range(3):
        for col in ((0, 1) if arr < 2 else (None,)):
            for v in (2048.0, np.nan, np.inf, -np.inf):
                st = [a.copy() for a in base]
                if col is None:
                    st[arr][3] = v
                else:
                    st[arr][3, col] = v
                assert SR.moments(*st)["measured"] == 7, (arr, col, v)


def test_no_measured_bot_gives_an_all_zero_row():
    pos, vel, rad = recipe(5)
    rad[:] = np.inf
    assert SR.moments(pos, vel, rad) == dict.fromkeys(SR.FIELDS, 0)
    assert SR.moments(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0)) == dict.fromkeys(SR.FIELDS, 0)


@pytest.mark.parametrize("n", SIZES + [300])
def test_the_gpu_tests_recipes_keep_every_bot_measured(n):
    for center in ((0.0, 0.0), CORNER):
        pos, vel, rad = recipe(n, center)
        row = SR.moments(pos, vel, rad)
        assert row["measured"] == n, (n, center)
        if center == CORNER and n > 1:
            assert row["xy"] < 0 < row["xx"] and row["sum_qx"] < 0 < row["sum_qy"]  # the signs mix
    if n == 1025:
        assert SR.moments(*recipe(n, CORNER))["xx"] >> 64 > 0  # the high parts fill


def test_gate_steps_replays_the_fp32_clock():
    got = SR.gate_steps(0.0, 0.01, 0.05, 100, 1e9)
    t, clock = f32(0.0), []
    for _ in range(100):
        clock.append(float(t))
        t = f32(t + f32(0.01))
    assert [c for _, c in got] == [clock[k] for k, _ in got]  # times are the accumulated clock's, bit for bit
    ks = [k for k, _ in got]
    assert ks[0] == 0 and 18 <= len(ks) <= 22 and all(3 <= b - a <= 7 for a, b in zip(ks, ks[1:]))
    assert ks == [k for k in range(100) if SR.gate(clock[k], 0.05, 0.01)]
    # every step at interval 0
    every = SR.gate_steps(0.0, 0.01, 0.0, 100, 1e9)
    assert [k for k, _ in every] == list(range(100)) and [c for _, c in every] == clock
    # a step whose start time exceeds max_time does not run
    short = SR.gate_steps(0.0, 0.01, 0.0, 100, 0.2)
    assert short == every[:len(short)] and 20 <= len(short) <= 22 and short[-1][1] <= float(f32(0.2))
    assert SR.gate_steps(1.0, 0.01, 0.0, 5, 0.5) == []
    late = SR.gate_steps(float(clock[37]), 0.01, 0.05, 63, 1e9)  # a later start continues the same clock
    assert [(k + 37, c) for k, c in late] == [g for g in got if g[0] >= 37]


# ---- 2. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimMoments", "pbSimSetSeries", "pbSimGetSeriesInfo", "pbSimGetSeriesOf", "pbSimGetSeriesTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi, host
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbMomentsRow) == 152 and C.sizeof(_capi.pbMoment128) == 16
    assert "pbMomentsRow" in header and "/* 152 bytes */" in header
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_moments.hip")).read()
    assert "static_assert(sizeof(pbMomentsRow) == 152" in source
    for name in ("pbHostMoments", "pbHostSetSeries", "pbHostSeriesInfo", "pbHostSeriesRows"):
        assert hasattr(host.lib(), name)
    ens = open(os.path.join(ROOT, "include", "particlebot_ensemble.h")).read()
    assert "Moments" not in ens and "Series" not in ens


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    row = _capi.pbMomentsRow(step=7, measured=7)
    i, c, r, ms = C.c_float(7.0), C.c_uint(7), C.c_ulonglong(7), C.c_float(7.0)

    def refused(rc, fn, word=None):
        msg = L.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and fn.encode() in msg and (word is None or word.encode() in msg), (rc, msg)

    refused(L.pbSimMoments(None, C.byref(row)), "pbSimMoments", "null")
    refused(L.pbSimMoments(fake, None), "pbSimMoments", "null")
    refused(L.pbSimSetSeries(None, 0.05, 16), "pbSimSetSeries", "null")
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        refused(L.pbSimSetSeries(fake, bad, 16), "pbSimSetSeries", "interval")
    refused(L.pbSimGetSeriesInfo(None, C.byref(i), C.byref(c), C.byref(r)), "pbSimGetSeriesInfo", "null")
    refused(L.pbSimGetSeriesInfo(fake, None, None, None), "pbSimGetSeriesInfo", "all null")
    refused(L.pbSimGetSeriesOf(None, 0, 0, 1, C.byref(row)), "pbSimGetSeriesOf", "null")
    refused(L.pbSimGetSeriesOf(fake, 0, 0, 1, None), "pbSimGetSeriesOf", "null")
    refused(L.pbSimGetSeriesOf(fake, 0, 0, 0, None), "pbSimGetSeriesOf", "null")
    refused(L.pbSimGetSeriesTimes(None, C.byref(r), C.byref(ms)), "pbSimGetSeriesTimes", "null")
    assert (i.value, c.value, r.value, ms.value) == (7.0, 7, 7, 7.0) and row.step == 7 and row.measured == 7


BAD_FLAGS = ([("--series-interval", v) for v in ("", "abc", "-1", "-1e-30", "nan", "inf", "-inf", "0.1x")]
             + [("--series-capacity", v) for v in ("", "0", "-3", "1.5", "1048577", "many")])


@pytest.mark.parametrize("flag,value", BAD_FLAGS, ids=[f"{f}={v!r}" for f, v in BAD_FLAGS])
def test_runner_refuses_a_bad_series_value(tmp_path, flag, value):
    for args in ([flag, value], [CFG, "--series", "s.csv", flag, value, "--quiet"]):
        r = subprocess.run([RUN] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), args
    assert not os.listdir(tmp_path)


def test_runner_series_flags_need_their_values_and_the_fused_engine(tmp_path):
    for flag in ("--series", "--series-interval", "--series-capacity"):
        r = subprocess.run([RUN, CFG, flag], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), flag
    said = "--series needs the fused engine (the recorder runs on its resident state)\n"
    for extra in ([], ["--series-interval", "0"], ["--series-interval", "3.4e38", "--series-capacity", "1"],
                  ["--series-capacity", "1048576"]):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--series", "s.csv"] + extra, capture_output=True, text=True,
                           timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", said), extra
    # last in the engine-check table: any other analysis flag speaks first
    r = subprocess.run([RUN, CFG, "--engine", "legacy", "--series", "s.csv", "--rearrange", "a.csv"], capture_output=True,
                       text=True, timeout=60, cwd=tmp_path)
    assert (r.returncode, r.stderr) == (2, "--rearrange needs the fused engine (the analysis runs on its resident state)\n")
    assert not os.listdir(tmp_path)
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_runner.cpp")).read()
    for flag in ("--series FILE", "--series-interval T", "--series-capacity N"):
        assert flag in source and flag in open(os.path.join(ROOT, "README.md")).read(), flag
        assert flag.split()[0] in open(os.path.join(ROOT, "INTEGRATION.md")).read(), flag


REFUSED = [
    (lambda h: h.moments(), "moments: the time series needs the fused engine",
     "Particlebot::moments: the time series needs the fused engine\n"),
    (lambda h: h.set_series(0.05, 16),
     "set_series: the time series needs the fused engine, a finite interval >= 0 and a ring of at most 2^31 bytes",
     "Particlebot::setSeries: the time series needs the fused engine\n"),
    (lambda h: h.series_info(), "series_info: the time series needs the fused engine",
     "Particlebot::seriesInfo: the time series needs the fused engine\n"),
    (lambda h: h.series_rows(), "series_info: the time series needs the fused engine",
     "Particlebot::seriesInfo: the time series needs the fused engine\n"),
]


@pytest.mark.parametrize("call,error,line", REFUSED, ids=["moments", "set_series", "series_info", "series_rows"])
def test_host_engine_has_no_series(capfd, call, error, line):
    from particlerobotsimulations_amd import _capi, host
    h = host.HostSim(CFG, engine="host")
    capfd.readouterr()
    with pytest.raises(RuntimeError) as caught:
        call(h)
    assert str(caught.value) == error
    assert capfd.readouterr() == ("", line)
    # the wrappers: a NULL row or count is refused before the class is asked; a refused call writes nothing
    L = host.lib()
    assert L.pbHostMoments(h._h, None) == -1 and L.pbHostSeriesRows(h._h, 0, None, 0, None) == -1
    assert capfd.readouterr() == ("", "")
    row, count = _capi.pbMomentsRow(step=7), C.c_ulonglong(7)
    assert L.pbHostSeriesRows(h._h, 0, C.byref(row), 1, C.byref(count)) == -1 and (row.step, count.value) == (7, 7)
    capfd.readouterr()
    h.close()


# ---- 3. the pure-Python helpers ----------------------------------------------------------------------------------------

def test_moments_row_composes_the_128_bit_sums():
    from particlerobotsimulations_amd import _capi
    r = _capi.pbMomentsRow(step=9, time=1.25, measured=3, sum_qx=-5, sum_qy=7, sum_qr=11, sum_wx=-13, sum_wy=17,
                           min_qx=-4, max_qx=2, min_qy=-1, max_qy=8)
    r.xx.lo, r.xx.hi = (1 << 33) + 5, 3         # a low accumulator beyond 2^32
    r.xy.lo, r.xy.hi = 6, -2                    # a negative signed sum
    r.vv.lo, r.vv.hi = (1 << 60) - 1, (1 << 59)
    d = _capi.row_dict(r)
    assert d["xx"] == (3 << 32) + (1 << 33) + 5 and d["xy"] == -(2 << 32) + 6 and d["yy"] == d["rr"] == 0
    assert d["vv"] == (1 << 91) + (1 << 60) - 1
    assert (d["step"], d["time"], d["measured"], d["sum_qx"], d["sum_wx"], d["min_qx"]) == (9, 1.25, 3, -5, -13, -4)
    assert set(d) == set(SR.FIELDS) | {"time", "step"} and "lo" not in d


def test_moments_summary_on_known_integers():
    import particlerobotsimulations_amd as pb
    assert "moments_summary" in pb.__all__
    # four bots at (1, 2), (3, 2), (1, 6), (3, 6) (+ (10, -20)), radii 1, 1, 3, 3, velocities (1, 0), (1, 0), (3, 4), (3, 4)
    pos = np.array([[1, 2], [3, 2], [1, 6], [3, 6]], f32) + np.array([10, -20], f32)
    vel = np.array([[1, 0], [1, 0], [3, 4], [3, 4]], f32)
    rad = np.array([1, 1, 3, 3], f32)
    s = pb.moments_summary(SR.moments(pos, vel, rad))
    assert s["centroid"] == (12.0, -16.0) and s["gyration"] == (1.0, 4.0, 0.0)
    assert s["gyration_eigenvalues"] == (4.0, 1.0) and s["major_axis_angle"] == math.pi / 2  # the long axis is y
    assert s["mean_radius"] == 2.0 and s["radius_variance"] == 1.0 and s["covered_area"] == math.pi * 20.0
    assert s["centroid_velocity"] == (2.0, 2.0) and s["velocity_variance"] == (1 + 1 + 25 + 25) / 4 - 8
    # a blob stretched along the diagonal x = y: the major axis at 45 degrees, the minor eigenvalue 0
    t = np.array([-3, -1, 1, 3], f32)
    d = pb.moments_summary(SR.moments(np.stack([t, t], 1), np.zeros((4, 2), f32), np.ones(4, f32)))
    assert d["gyration"] == (5.0, 5.0, 5.0) and d["gyration_eigenvalues"] == (10.0, 0.0)
    assert d["major_axis_angle"] == math.pi / 4 and d["radius_variance"] == 0.0 and d["velocity_variance"] == 0.0
    # far from the origin the differences of large integers are formed exactly: a float64 route would lose them
    far = np.array([[2047.0, -2047.0], [2047.0 + 2.0 ** -12, -2047.0]], f32)
    g = pb.moments_summary(SR.moments(far, np.zeros((2, 2), f32), np.ones(2, f32)))
    assert g["gyration"] == (2.0 ** -26, 0.0, 0.0) and g["centroid"] == (2047.0 + 2.0 ** -13, -2047.0)
    none = pb.moments_summary(dict.fromkeys(SR.FIELDS, 0))
    assert set(none) == set(s) and all(v is None for v in none.values())
