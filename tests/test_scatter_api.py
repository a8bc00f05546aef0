"""CPU side of the self-intermediate scattering function (pbSimSetScattering / pbSimScatteringRecord /
pbSimGetScattering, csrc/pb_scatter.hip).

1. tests/scatter_ref.py, the reference the GPU tests compare against: it equals a plain loop over bots, lags and vectors,
   its index of a difference of turns equals the index of the difference of positions, and it gives the known answers.
2. The recipes of tests/test_gpu_scatter.py keep every pair measured.
3. The C-ABI entries are declared, exported and reject bad arguments before they touch the device.
4. The runner knows --scatter and its options; the placement-only host engine has no scattering.
5. scattering_summary on known integers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import scatter_ref as XR
import series_ref as SR
import sfactor_ref as KR
from test_runner_analysis_flags import USAGE
from test_series_api import CORNER, recipe
from test_timecorr_api import batch_records, manual_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
ONE = 1 << 20
TOP = (1 << 31) - 1

# ---- what tests/test_gpu_scatter.py records ----------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
NVECS = [1, 3, 64, 65, 256]  # one lane per stripe, a padded non-power-of-two, the two sides of a padding step, all lanes
BOXES = [-8, 3, 12]
MANUAL_LAGS, MANUAL_RECORDS = 3, 7  # the ring wraps twice
BATCH_LAGS = 3


def vector_list(nvec):
    """`nvec` integer pairs: small vectors of both signs, and in every list that has room for them (0, 0), the extreme
    (2^31 - 1, -2^31) and a vector that occurs twice."""
    rng = np.random.default_rng(400 + nvec)
    v = rng.integers(-40, 41, size=(nvec, 2)).astype(np.int64)
    v[0] = (2, 1)
    if nvec >= 3:
        v[0], v[1], v[2] = (5, -3), (TOP, -TOP - 1), (5, -3)
    if nvec >= 4:
        v[3] = (0, 0)
    if nvec >= 64:
        v[nvec - 1] = v[7]  # the last lane that works repeats an earlier one
    return v.astype(np.int32)


def positions(records):
    return [r[0] for r in records]


def dyadic_positions(n=70):
    """Positions on a grid of 1/64 within +-100: every shift used below is exact in fp32 and in quanta."""
    rng = np.random.default_rng(88)
    return (rng.integers(-6400, 6401, size=(n, 2)).astype(f32) / f32(64.0)).astype(f32)


# the known answers: box 2^3, L = 8.  (shift, vector) -> (re, im) per sample, of a rigid shift between two records
L_LOG2, L = 3, 8.0


def known_cases():
    t = KR.table().astype(np.int64)
    u = 1 << 30
    return [((L / 4, 0.0), (1, 0), (0, u)),                      # a quarter turn
            ((L / 2, 0.0), (1, 0), (-u, 0)),                     # half a turn
            ((0.0, -L / 4), (0, 1), (0, -u)),                    # a quarter turn back, along y
            ((L / 8192, 0.0), (1, 0), (int(t[1, 0]), int(t[1, 1]))),   # exactly half a table step: rounds up, to step 1
            ((-L / 8192, 0.0), (1, 0), (u, 0)),                  # half a step below a whole turn: rounds up, to step 0
            ((L, 0.0), (1, 0), (u, 0)),                          # a whole box: lag 0's answer
            ((L, -3 * L), (7, -5), (u, 0)),                      # whole boxes along both axes, any vector
            ((L / 4, 0.0), (4, 9), (u, 0)),                      # n times a quarter turn is a whole one
            ((L / 4, 0.0), (0, 0), (u, 0))]                      # the zero vector sees no displacement


def unmeasured_records(n=257):
    """Three records of the recipe, each shifted a little, with one bot of every unmeasured kind in x or y at one record
    each: NaN, the infinities, +-2048 and beyond.  Returns the positions and, per record, the bad bots."""
    pos = recipe(n)[0]
    recs = [(pos + np.array(s, f32)).astype(f32) for s in ((0.0, 0.0), (0.25, -0.5), (-0.125, 0.75))]
    bad = [set(), set(), set()]
    i = 5
    for when in (0, 1, 2):
        for col in (0, 1):
            for val in (np.nan, np.inf, -np.inf, 2048.0, -2048.0, 3.0e9):
                recs[when][i, col] = val
                bad[when].add(i)
                i += 1
    assert i < 100
    below = np.nextafter(f32(2048.0), f32(0.0))
    recs[0][100], recs[1][101], recs[2][102] = (below, -below), (-below, 7.0), (7.0, below)  # just inside: measured
    return recs, [sorted(b) for b in bad]


def unmeasured_samples(n, bad, lags=3):
    """The samples per lag of three records whose bad bots are `bad` per record."""
    out = []
    for l in range(lags):
        out.append(sum(n - len(set(bad[r]) | set(bad[r - l])) for r in range(l, 3)))
    return out


def float64_records(n=1000):
    """Two records: random positions within +-3 and displacements within +-0.5."""
    rng = np.random.default_rng(64)
    a = rng.uniform(-3.0, 3.0, size=(n, 2)).astype(f32)
    b = (a + rng.uniform(-0.5, 0.5, size=(n, 2)).astype(f32)).astype(f32)
    return [a, b]


def phase_bound(nx, ny, box_log2):
    """The header's bound on |re / (2^30 samples) - mean cos(k . dr)|: the table step, two position quanta of 2^-21 per
    axis and instant, and the entry's rounding."""
    return math.pi / 4096 + 2 * math.pi * (abs(nx) + abs(ny)) * 2.0 ** -20 / 2.0 ** box_log2 + 2.0 ** -30


# ---- 1. the reference --------------------------------------------------------------------------------------------------

def plain_loop(records, steps, lags, vectors, box_log2):
    """The definition, record by record, lag by lag, vector by vector and bot by bot, in Python ints mod 2^32."""
    tab = KR.table()
    quant = lambda v: int(np.rint(np.float64(v) * 2.0 ** 20))  # float64: exact, ties to even
    snaps = [[(quant(x), quant(y)) if abs(x) < 2048.0 and abs(y) < 2048.0 else None for x, y in np.asarray(p, f32)]
             for p in records]
    rows = [[dict(dict.fromkeys(XR.FIELDS, 0), lag=l, nx=int(nx), ny=int(ny)) for nx, ny in vectors] for l in range(lags)]
    for r in range(len(snaps)):
        for l in range(min(r, lags - 1) + 1):
            for row in rows[l]:
                row["origins"] += 1
                row["sum_steps"] += steps[r] - steps[r - l]
                for now, then in zip(snaps[r], snaps[r - l]):
                    if now is None or then is None:
                        continue
                    u = (row["nx"] * (now[0] - then[0]) + row["ny"] * (now[1] - then[1])) & 0xFFFFFFFF
                    t = (u << (12 - box_log2)) & 0xFFFFFFFF
                    idx = (((t + 0x80000) & 0xFFFFFFFF) >> 20) & 4095
                    row["samples"] += 1
                    row["re"] += int(tab[idx, 0])
                    row["im"] += int(tab[idx, 1])
    return rows


def test_reference_equals_a_plain_loop():
    recs = positions(manual_records(65, CORNER, records=5))
    recs[1][17, 0] = np.nan
    recs[3][18, 1] = -2048.0
    vectors = vector_list(3).tolist() + [[0, 0], [-7, 11]]
    steps = [0, 4, 9, 15, 16]
    for box in (-8, 3, 12):
        got = XR.table(recs, steps, 3, vectors, box)
        assert got == plain_loop(recs, steps, 3, vectors, box), box
        assert all(tuple(g) == XR.FIELDS for row in got for g in row)
    assert [row[0]["origins"] for row in got] == [5, 4, 3] and [row[0]["sum_steps"] for row in got] == [0, 16, 27]
    assert [row[0]["samples"] for row in got] == [5 * 65 - 2, 4 * 65 - 4, 3 * 65 - 2]
    assert all(g["samples"] == row[0]["samples"] for row in got for g in row)  # the same for every vector of a lag
    assert got[0][0]["re"] == got[0][0]["samples"] << 30 and got[0][0]["im"] == 0
    assert got[1][0]["re"] != got[1][0]["samples"] << 30 and got[1][0]["im"] != 0
    assert got[1][0] == got[1][2]  # the repeated vector


def test_index_of_the_difference_of_turns_is_the_index_of_the_difference_of_positions():
    rng = np.random.default_rng(12)
    top = (1 << 31) - 128
    q = rng.integers(-top, top + 1, size=(4, 4096))  # qx_now, qy_now, qx_then, qy_then over the whole measured range
    q[:, :4] = [[top, -top, top, -top], [-top, top, top, -top], [-top, top, -top, top], [top, -top, -top, top]]
    vecs = [(1, 0), (0, 1), (3, -2), (TOP, -TOP - 1), (-TOP - 1, TOP), (65536, 65537), (0, 0)] \
        + rng.integers(-(1 << 31), 1 << 31, size=(8, 2)).tolist()
    m = 0xFFFFFFFF
    for nx, ny in vecs:
        for box in (-8, 0, 3, 12):
            shift = 12 - box
            u_now = (nx * q[0] + ny * q[1]) & m
            u_then = (nx * q[2] + ny * q[3]) & m
            t = (((u_now - u_then) & m) << shift) & m
            want = (((t + 0x80000) & m) >> 20) & 4095
            got = KR.index(nx, ny, q[0] - q[2], q[1] - q[3], box)
            assert np.array_equal(got.astype(np.int64), want), (nx, ny, box)
            # the shift staged with the pair, as the kernel does: the same turn mod 2^32
            staged = (nx * (((q[0] - q[2]) << shift) & m) + ny * (((q[1] - q[3]) << shift) & m)) & m
            assert np.array_equal((((staged + 0x80000) & m) >> 20) & 4095, want), (nx, ny, box)


def test_known_answers_on_dyadic_positions():
    pos = dyadic_positions()
    n = len(pos)
    for shift, vec, (re, im) in known_cases():
        moved = (pos + np.array(shift, f32)).astype(f32)
        assert np.array_equal(moved.astype(np.float64), pos.astype(np.float64) + np.array(shift)), shift  # exact in fp32
        rows = XR.table([pos, moved], [0, 5], 2, [vec], L_LOG2)
        assert rows[0][0] == {"lag": 0, "nx": vec[0], "ny": vec[1], "origins": 2, "sum_steps": 0, "samples": 2 * n,
                              "re": (2 * n) << 30, "im": 0}, (shift, vec)
        assert rows[1][0] == {"lag": 1, "nx": vec[0], "ny": vec[1], "origins": 1, "sum_steps": 5, "samples": n,
                              "re": n * re, "im": n * im}, (shift, vec)
    t = KR.table()
    assert 0 < int(t[1, 1]) < int(t[1, 0]) < 1 << 30 and int(t[1024, 0]) == 0 and int(t[2048, 1]) == 0


def test_unmeasured_bots_drop_out_of_exactly_the_lags_that_pair_their_record():
    recs, bad = unmeasured_records()
    assert [len(b) for b in bad] == [12, 12, 12]
    vectors = vector_list(3)
    rows = XR.table(recs, [0, 1, 2], 3, vectors, 3)
    assert rows == plain_loop(recs, [0, 1, 2], 3, vectors.tolist(), 3)
    assert [r[0]["samples"] for r in rows] == unmeasured_samples(257, bad) == [3 * 257 - 36, 2 * 257 - 48, 257 - 24]
    keep = np.setdiff1d(np.arange(257), bad[0] + bad[2])
    assert XR.table([recs[0][keep], recs[2][keep]], [0, 2], 2, vectors, 3)[1] == [dict(r, lag=1) for r in rows[2]]
    # no measured pair: zeros with the right origins
    far = np.full((5, 2), 3000.0, f32)
    got = XR.table([far, far], [3, 9], 2, [(1, 0)], 3)
    zero = dict(dict.fromkeys(XR.FIELDS, 0), nx=1)
    assert got == [[dict(zero, lag=0, origins=2)], [dict(zero, lag=1, origins=1, sum_steps=6)]]


def test_ring_wrap_counts_every_origin():
    rng = np.random.default_rng(11)
    recs = [(rng.integers(-64, 65, (5, 2)) / 16.0).astype(f32) for _ in range(8)]
    steps = [0, 3, 7, 8, 20, 21, 30, 44]
    got = XR.table(recs, steps, 3, [(1, 1), (0, 2)], 4)
    assert [g[1]["origins"] for g in got] == [8, 7, 6] and [g[0]["samples"] for g in got] == [40, 35, 30]
    assert [g[0]["sum_steps"] for g in got] == [0, 44, sum(steps[r] - steps[r - 2] for r in range(2, 8))]
    assert got == plain_loop(recs, steps, 3, [(1, 1), (0, 2)], 4)


def test_float64_bound_holds_for_the_reference():
    recs = float64_records()
    import particlerobotsimulations_amd as pb
    vectors = pb.half_plane_vectors(3)
    rows = XR.table(recs, [0, 1], 2, vectors, 3)[1]
    dr = recs[1].astype(np.float64) - recs[0].astype(np.float64)
    worst = 0.0
    for row in rows:
        phase = 2 * np.pi / 8.0 * (row["nx"] * dr[:, 0] + row["ny"] * dr[:, 1])
        bound = phase_bound(row["nx"], row["ny"], 3)
        for got, want in ((row["re"], np.cos(phase).mean()), (row["im"], np.sin(phase).mean())):
            err = abs(got / 2.0 ** 30 / row["samples"] - want)
            worst = max(worst, err / bound)
            assert err <= bound, (row, err, bound)
    assert row["samples"] == 1000 and 0.0 < worst < 1.0


# ---- 2. the GPU tests' recipes -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_the_gpu_tests_recipes_keep_every_pair_measured(n):
    for center in ((0.0, 0.0), CORNER):
        recs = positions(manual_records(n, center, records=MANUAL_RECORDS))
        for p in recs:
            assert XR.snapshot(p)[2].all(), (n, center)
        rows = XR.table(recs, [0] * MANUAL_RECORDS, MANUAL_LAGS, vector_list(3), 3)
        assert [r[0]["origins"] for r in rows] == [7, 6, 5]
        assert [r[0]["samples"] for r in rows] == [7 * n, 6 * n, 5 * n], (n, center)
    for nvec in NVECS:
        v = vector_list(nvec)
        assert v.shape == (nvec, 2) and v.dtype == np.int32
        if nvec >= 4:
            assert [0, 0] in v.tolist() and [TOP, -TOP - 1] in v.tolist() and v[0].tolist() == v[2].tolist()


def test_the_gpu_tests_batch_large_and_float64_records_keep_every_pair_measured():
    for recs in batch_records():
        assert all(XR.snapshot(p)[2].all() for p in positions(recs))
    big = positions(manual_records(256 * 256 + 321, (-300.0, 700.0), records=3))
    assert all(XR.snapshot(p)[2].all() for p in big)
    assert all(XR.snapshot(p)[2].all() for p in float64_records())
    assert XR.snapshot(dyadic_positions())[2].all()


# ---- 3. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimSetScattering", "pbSimScatteringRecord", "pbSimGetScatteringInfo", "pbSimGetScattering",
         "pbSimGetScatteringTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi, host
    import particlerobotsimulations_amd as pb
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbScatteringRow) == 56
    assert "pbScatteringRow" in header and "/* 56 bytes */" in header
    for line in ("#define PB_SCATTER_MAX_LAGS 64u", "#define PB_SCATTER_MAX_VECTORS 256u", "#define PB_SCATTER_BLOCKS 256u"):
        assert line in header
    assert (_capi.SCATTER_MAX_LAGS, _capi.SCATTER_MAX_VECTORS) == (64, 256)
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_scatter.hip")).read()
    assert "static_assert(sizeof(pbScatteringRow) == 56" in source
    for name in ("pbHostSetScattering", "pbHostScatteringRecord", "pbHostScatteringInfo", "pbHostScatteringRows"):
        assert hasattr(host.lib(), name)
    for name in ("set_scattering", "scattering_record", "scattering_info", "scattering", "scattering_times"):
        assert hasattr(pb.Sim, name)
    assert "scattering_summary" in pb.__all__
    block = header.split("Self-intermediate scattering on the device")[1].split("#define PB_SCATTER_MAX_LAGS")[0]
    for word in ("DIFFERENCE OF THE QUANTISED POSITIONS", "pi / 4096  +  2 pi (|nx| + |ny|) 2^-20 / L", "derived, not measured",
                 "coherent F(k, tau)", "chi_4", "weights other than 1", "logarithmic lag spacing", "summary rows",
                 "the legacy engine", "series, time correlation, scattering"):
        assert word in block, word
    # the two sentences that used to list it as out of scope point here now
    flat = re.sub(r"\s*\n \* ", " ", header)
    assert "the self-intermediate scattering function and" not in flat
    assert flat.count("pbSimSetScattering, below") == 2


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    row = _capi.pbScatteringRow(lag=7, samples=7)
    vec = (C.c_int * 4)(1, 0, 0, 1)
    i, l, e, k, r, ms = C.c_float(7.0), C.c_uint(7), C.c_int(7), C.c_uint(7), C.c_ulonglong(7), C.c_float(7.0)

    def refused(rc, fn, word=None):
        msg = L.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and fn.encode() in msg and (word is None or word.encode() in msg), (rc, msg)

    fn = "pbSimSetScattering"
    refused(L.pbSimSetScattering(None, 0.05, 8, 3, vec, 2), fn, "null")
    refused(L.pbSimSetScattering(fake, 0.05, 8, 3, None, 2), fn, "null vectors")
    for bad in (-0.5, -2.0, -1e-30, np.nextafter(f32(-1.0), f32(0.0)), float("nan"), float("inf"), float("-inf")):
        refused(L.pbSimSetScattering(fake, float(bad), 8, 3, vec, 2), fn, "interval")
        refused(L.pbSimSetScattering(fake, float(bad), 0, 3, vec, 2), fn, "interval")  # switching off checks it too
    for bad in (65, 1 << 31):
        refused(L.pbSimSetScattering(fake, 0.05, bad, 3, vec, 2), fn, "lags")
        refused(L.pbSimSetScattering(fake, -1.0, bad, 3, vec, 2), fn, "lags")  # -1 is an interval
    for bad in (-9, 13, -(1 << 31), (1 << 31) - 1):
        refused(L.pbSimSetScattering(fake, 0.0, 8, bad, vec, 2), fn, "boxLog2")
    for bad in (0, 257, 1 << 31):
        refused(L.pbSimSetScattering(fake, 0.0, 8, 3, vec, bad), fn, "nvec")
    refused(L.pbSimScatteringRecord(None), "pbSimScatteringRecord", "null")
    refused(L.pbSimGetScatteringInfo(None, C.byref(i), C.byref(l), C.byref(e), C.byref(k), C.byref(r)),
            "pbSimGetScatteringInfo", "null")
    refused(L.pbSimGetScatteringInfo(fake, None, None, None, None, None), "pbSimGetScatteringInfo", "all null")
    refused(L.pbSimGetScattering(None, C.byref(row)), "pbSimGetScattering", "null")
    refused(L.pbSimGetScattering(fake, None), "pbSimGetScattering", "null")
    refused(L.pbSimGetScatteringTimes(None, C.byref(r), C.byref(ms)), "pbSimGetScatteringTimes", "null")
    assert (i.value, l.value, e.value, k.value, r.value, ms.value) == (7.0, 7, 7, 7, 7, 7.0)
    assert row.lag == 7 and row.samples == 7


# ---- 4. the runner and the host engine ---------------------------------------------------------------------------------

NOT_A_NUMBER = ["", "abc", "-1", "-1e-30", "nan", "inf", "-inf", "0.1x"]
BAD_FLAGS = ([("--scatter-interval", v) for v in NOT_A_NUMBER]
             + [("--scatter-lags", v) for v in ("", "0", "-3", "1.5", "65", "many")]
             + [("--scatter-box-log2", v) for v in ("", "-9", "13", "1.5", "big")]
             + [("--scatter-nmax", v) for v in ("", "0", "-1", "11", "2.5", "all")])  # 11: 264 vectors, past 256


@pytest.mark.parametrize("flag,value", BAD_FLAGS, ids=[f"{f}={v!r}" for f, v in BAD_FLAGS])
def test_runner_refuses_a_bad_scatter_value(tmp_path, flag, value):
    for args in ([flag, value], [CFG, "--scatter", "f.csv", flag, value, "--quiet"]):
        r = subprocess.run([RUN] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), args
    assert not os.listdir(tmp_path)


def test_runner_scatter_flags_need_their_values_and_the_fused_engine(tmp_path):
    flags = ("--scatter", "--scatter-interval", "--scatter-lags", "--scatter-box-log2", "--scatter-nmax")
    for flag in flags:
        r = subprocess.run([RUN, CFG, flag], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), flag
    said = "--scatter needs the fused engine (the recorder runs on its resident state)\n"
    for extra in ([], ["--scatter-interval", "0"], ["--scatter-interval", "3.4e38", "--scatter-lags", "1"],
                  ["--scatter-lags", "64", "--scatter-nmax", "10"], ["--scatter-box-log2", "-8"],
                  ["--scatter-box-log2", "12", "--scatter-nmax", "1"]):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--scatter", "f.csv"] + extra, capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", said), extra
    # last in the engine-check table: any earlier analysis flag speaks first
    for flag, line in (("--timecorr", "--timecorr needs the fused engine (the recorder runs on its resident state)\n"),
                       ("--sk", "--sk needs the fused engine (the analysis runs on its resident state)\n")):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--scatter", "f.csv", flag, "a.csv"], capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stderr) == (2, line)
    assert not os.listdir(tmp_path)
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_runner.cpp")).read()
    for flag in ("--scatter FILE", "--scatter-interval T", "--scatter-lags N", "--scatter-box-log2 E", "--scatter-nmax M"):
        assert flag in source and flag in open(os.path.join(ROOT, "README.md")).read(), flag
        assert flag.split()[0] in open(os.path.join(ROOT, "INTEGRATION.md")).read(), flag
    assert "Lag, Nx, Ny, Origins, SumSteps, Samples, Re, Im, FsRe, FsIm" in source
    assert "scatter" not in USAGE  # the usage line stays as it is
    import particlerobotsimulations_amd as pb
    assert len(pb.half_plane_vectors(3)) == 24 and len(pb.half_plane_vectors(10)) == 220 < 256 < len(pb.half_plane_vectors(11))


NEEDS = "the scattering needs the fused engine"
REFUSED = [
    (lambda h: h.set_scattering(0.05, 8, 3, [[1, 0]]),
     "set_scattering: " + NEEDS + ", a finite interval >= 0 (or -1), at most 64 lags, box_log2 in -8 ... 12 and "
     "1 ... 256 vectors", "Particlebot::setScattering: " + NEEDS + "\n"),
    (lambda h: h.scattering_record(), "scattering_record: " + NEEDS + " and the scattering on",
     "Particlebot::scatteringRecord: " + NEEDS + "\n"),
    (lambda h: h.scattering_info(), "scattering_info: " + NEEDS, "Particlebot::scatteringInfo: " + NEEDS + "\n"),
    (lambda h: h.scattering(), "scattering_info: " + NEEDS, "Particlebot::scatteringInfo: " + NEEDS + "\n"),
]


@pytest.mark.parametrize("call,error,line", REFUSED, ids=["set", "record", "info", "rows"])
def test_host_engine_has_no_scattering(capfd, call, error, line):
    from particlerobotsimulations_amd import _capi, host
    h = host.HostSim(CFG, engine="host")
    capfd.readouterr()
    with pytest.raises(RuntimeError) as caught:
        call(h)
    assert str(caught.value) == error
    assert capfd.readouterr() == ("", line)
    # the wrapper: a NULL count is refused before the class is asked; a refused call writes nothing
    L = host.lib()
    assert L.pbHostScatteringRows(h._h, None, 0, None) == -1
    assert capfd.readouterr() == ("", "")
    row, count = _capi.pbScatteringRow(lag=7), C.c_ulonglong(7)
    assert L.pbHostScatteringRows(h._h, C.byref(row), 1, C.byref(count)) == -1 and (row.lag, count.value) == (7, 7)
    assert capfd.readouterr() == ("", "Particlebot::scatteringRows: " + NEEDS + "\n")
    h.close()


# ---- 5. the pure-Python helpers ----------------------------------------------------------------------------------------

def test_scattering_row_and_summary_on_known_integers():
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import _capi
    r = _capi.pbScatteringRow(lag=3, nx=-2, ny=5, reserved=0, origins=5, sum_steps=60, samples=16, re=-(3 << 30), im=1 << 29)
    d = _capi.row_dict(r)
    assert d == {"lag": 3, "nx": -2, "ny": 5, "origins": 5, "sum_steps": 60, "samples": 16, "re": -(3 << 30), "im": 1 << 29}
    assert tuple(d) == XR.FIELDS
    assert pb.scattering_summary(d) == {"fs_re": -3 / 16, "fs_im": 1 / 32, "mean_lag_steps": 12.0}
    pos = dyadic_positions()
    rows = XR.table([pos, (pos + np.array([2.0, 0.0], f32)).astype(f32)], [0, 10], 2, [(1, 0)], L_LOG2)
    assert pb.scattering_summary(rows[0][0]) == {"fs_re": 1.0, "fs_im": 0.0, "mean_lag_steps": 0.0}
    assert pb.scattering_summary(rows[1][0]) == {"fs_re": 0.0, "fs_im": 1.0, "mean_lag_steps": 10.0}
    # formed as one exact fraction: 2^61 - 1 over 2^61 is not 1.0 minus a float64's rounding of the numerator
    big = dict(d, samples=(1 << 31) - 1, re=((1 << 31) - 1) << 30, im=-1)
    s = pb.scattering_summary(big)
    assert s["fs_re"] == 1.0 and s["fs_im"] == -1.0 / (((1 << 31) - 1) << 30)
    none = pb.scattering_summary(dict.fromkeys(XR.FIELDS, 0))
    assert none == {"fs_re": None, "fs_im": None, "mean_lag_steps": None}
