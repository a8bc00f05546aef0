"""CPU side of the coherent intermediate scattering function (pbSimSetCoherent / pbSimCoherentRecord / pbSimGetCoherent,
csrc/pb_coherent.hip).

1. tests/coherent_ref.py, the reference the GPU tests compare against: it equals a plain double loop, its lag 0 and its
   modes are what the header says they are, it gives the known answers, drops unmeasured bots from exactly their
   records, wraps the ring, composes negative sums and stays inside the header's float64 bound.
2. The C-ABI entries are declared, exported and reject bad arguments before they touch the device.
3. The runner knows --coherent and its options; the host library's wrappers refuse on the placement-only host engine.
4. coherent_scattering_summary on known integers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import coherent_ref as CR
import sfactor_ref as KR
from test_runner_analysis_flags import USAGE
from test_scatter_api import (L, L_LOG2, TOP, dyadic_positions, float64_records, positions, unmeasured_records,
                              vector_list)
from test_series_api import CORNER
from test_timecorr_api import manual_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32
UNIT = 1 << 60


def eps(nx, ny, box_log2):
    """The per-bot bound of pbSimStructureFactor's block: the table step, one position quantum of 2^-21 per axis, and
    the entry's rounding."""
    return math.pi / 4096 + 2 * math.pi * (abs(nx) + abs(ny)) * 2.0 ** -21 / 2.0 ** box_log2 + 2.0 ** -30


def product_bound(nx, ny, box_log2, bots_now, bots_then):
    """The header's bound on |device product / 2^60 - float64 product| of one origin, in re and in im."""
    e = eps(nx, ny, box_log2)
    return bots_now * bots_then * (2 * e + e * e)


def float64_products(records, vectors, box_log2):
    """rho_now conj(rho_then) of records 1 and 0 in float64 from the fp32 positions: one complex number per vector."""
    a, b = (np.asarray(r, np.float64) for r in records)
    out = []
    for nx, ny in np.asarray(vectors).tolist():
        k = 2 * np.pi / 2.0 ** box_log2 * np.array([nx, ny], np.float64)
        out.append(np.exp(1j * (b @ k)).sum() * np.conj(np.exp(1j * (a @ k)).sum()))
    return out


# ---- 1. the reference --------------------------------------------------------------------------------------------------

def plain_loop(records, steps, lags, vectors, box_log2):
    """The definition: per record and vector the mode bot by bot in Python ints mod 2^32, then record by record and lag by
    lag the product of two modes."""
    tab = KR.table()
    quant = lambda v: int(np.rint(np.float64(v) * 2.0 ** 20))  # float64: exact, ties to even
    recs = []
    for p in records:
        bots = [(quant(x), quant(y)) for x, y in np.asarray(p, f32) if abs(x) < 2048.0 and abs(y) < 2048.0]
        mode = []
        for nx, ny in vectors:
            c = s = 0
            for qx, qy in bots:
                u = (nx * qx + ny * qy) & 0xFFFFFFFF
                t = (u << (12 - box_log2)) & 0xFFFFFFFF
                idx = (((t + 0x80000) & 0xFFFFFFFF) >> 20) & 4095
                c += int(tab[idx, 0])
                s += int(tab[idx, 1])
            mode.append((c, s))
        recs.append((len(bots), mode))
    rows = [[dict(dict.fromkeys(CR.FIELDS, 0), lag=l, nx=int(nx), ny=int(ny)) for nx, ny in vectors] for l in range(lags)]
    for r in range(len(recs)):
        for l in range(min(r, lags - 1) + 1):
            for k, row in enumerate(rows[l]):
                (cn, sn), (ct, st) = recs[r][1][k], recs[r - l][1][k]
                row["origins"] += 1
                row["sum_steps"] += steps[r] - steps[r - l]
                row["bots_now"] += recs[r][0]
                row["bots_then"] += recs[r - l][0]
                row["re"] += cn * ct + sn * st
                row["im"] += sn * ct - cn * st
    return rows


def test_reference_equals_a_plain_double_loop():
    recs = positions(manual_records(65, CORNER, records=5))
    recs[1][17, 0] = np.nan
    recs[3][18, 1] = -2048.0
    vectors = vector_list(3).tolist() + [[0, 0], [-7, 11]]
    steps = [0, 4, 9, 15, 16]
    for box in (-8, 3, 12):
        got = CR.table(recs, steps, 3, vectors, box)
        assert got == plain_loop(recs, steps, 3, vectors, box), box
        assert all(tuple(g) == CR.FIELDS for row in got for g in row)
    assert [row[0]["origins"] for row in got] == [5, 4, 3] and [row[0]["sum_steps"] for row in got] == [0, 16, 27]
    assert [row[0]["bots_now"] for row in got] == [5 * 65 - 2, 4 * 65 - 2, 3 * 65 - 1]
    assert [row[0]["bots_then"] for row in got] == [5 * 65 - 2, 4 * 65 - 2, 3 * 65 - 1]  # (records 1 and 3 are in both sums)
    assert all(g["bots_then"] == row[0]["bots_then"] for row in got for g in row)  # the same for every vector of a lag
    assert got[1][0] == got[1][2]  # the repeated vector
    assert got[1][3]["re"] == sum((65 - (r in (1, 3))) * (65 - (r - 1 in (1, 3))) for r in range(1, 5)) << 60  # (0, 0)
    assert got[1][3]["im"] == 0 and got[1][0]["im"] != 0


def test_lag_zero_is_the_summed_square_and_has_no_imaginary_part():
    recs = positions(manual_records(257, (1.5, -2.25), records=4))
    vectors = vector_list(65)
    rows = CR.table(recs, [0, 1, 2, 3], 2, vectors, 3)
    modes = [CR.modes(p, vectors, 3) for p in recs]
    for k, row in enumerate(rows[0]):
        assert row["im"] == 0 and row["re"] == sum(m[1][k][0] ** 2 + m[1][k][1] ** 2 for m in modes), k
        assert row["bots_now"] == row["bots_then"] == 4 * 257
    assert any(r["im"] != 0 for r in rows[1])


def test_a_mode_is_the_density_structure_factor_of_the_same_state():
    recs, _ = unmeasured_records()
    zeros = np.zeros((257, 2), f32)
    for nvec, box in ((3, -8), (65, 3), (256, 12)):
        vectors = vector_list(nvec)
        for p in recs:
            measured, mode = CR.modes(p, vectors, box)
            want = KR.structure_factor(p, zeros, np.full(257, 0.1, f32), vectors, box, "density")
            assert [(w["re"], w["im"]) for w in want] == mode and {w["measured"] for w in want} == {measured}
    assert measured == 257 - 12


def test_known_answers_on_dyadic_positions():
    n = 70
    point = np.zeros((n, 2), f32)
    moved = (point + np.array([L / 4, 0.0], f32)).astype(f32)
    for vec in ((1, 0), (0, 1), (5, -3), (TOP, -TOP - 1)):  # all bots on the origin: every vector sees the table's step 0
        rows = CR.table([point, point], [0, 5], 2, [vec], L_LOG2)
        assert rows[0][0] == {"lag": 0, "nx": vec[0], "ny": vec[1], "origins": 2, "sum_steps": 0, "bots_now": 2 * n,
                              "bots_then": 2 * n, "re": 2 * n * n * UNIT, "im": 0}
        assert rows[1][0] == {"lag": 1, "nx": vec[0], "ny": vec[1], "origins": 1, "sum_steps": 5, "bots_now": n,
                              "bots_then": n, "re": n * n * UNIT, "im": 0}
    # moved a quarter box along x: a quarter turn for k = (1, 0), none for k = (0, 1), a whole one for k = (4, 9)
    rows = CR.table([point, moved], [0, 5], 2, [(1, 0), (0, 1), (4, 9), (2, 0)], L_LOG2)
    assert [(r["re"], r["im"]) for r in rows[1]] == [(0, n * n * UNIT), (n * n * UNIT, 0), (n * n * UNIT, 0),
                                                     (-n * n * UNIT, 0)]
    assert all(r["re"] == 2 * n * n * UNIT and r["im"] == 0 for r in rows[0])
    # a rigid shift of any dyadic blob by a quarter box turns every mode by a quarter turn: F(lag 1) = i S(k)
    pos = dyadic_positions()
    rows = CR.table([pos, (pos + np.array([L / 4, 0.0], f32)).astype(f32)], [0, 1], 2, [(1, 0)], L_LOG2)
    (_, [(c, s)]) = CR.modes(pos, [(1, 0)], L_LOG2)
    assert rows[1][0]["re"] == 0 and rows[1][0]["im"] == c * c + s * s > 0


def test_an_unmeasured_bot_drops_out_of_exactly_the_records_it_is_bad_in():
    recs, bad = unmeasured_records()
    assert [len(b) for b in bad] == [12, 12, 12]
    vectors = vector_list(3)
    rows = CR.table(recs, [0, 1, 2], 3, vectors, 3)
    assert rows == plain_loop(recs, [0, 1, 2], 3, vectors.tolist(), 3)
    m = [257 - 12] * 3
    assert [r[0]["bots_now"] for r in rows] == [sum(m), m[1] + m[2], m[2]]
    assert [r[0]["bots_then"] for r in rows] == [sum(m), m[0] + m[1], m[0]]
    # a record's mode is that of its measured bots alone, whatever the other record lacks: unlike the self part, a bot
    # that is bad in one record still counts in the other
    keep = [np.setdiff1d(np.arange(257), b) for b in bad]
    assert CR.table([recs[0][keep[0]][:200], recs[0][keep[0]][200:]], [0, 0], 1, vectors, 3)[0][0]["bots_now"] == 245
    two = CR.table_of_modes([CR.modes(recs[0][keep[0]], vectors, 3), CR.modes(recs[2][keep[2]], vectors, 3)], [0, 2], 2,
                            vectors)
    assert two[1] == [dict(r, lag=1) for r in rows[2]]
    # no measured bot: zeros with the right origins
    far = np.full((5, 2), 3000.0, f32)
    got = CR.table([far, far], [3, 9], 2, [(1, 0)], 3)
    zero = dict(dict.fromkeys(CR.FIELDS, 0), nx=1)
    assert got == [[dict(zero, lag=0, origins=2)], [dict(zero, lag=1, origins=1, sum_steps=6)]]


def test_ring_wrap_counts_every_origin():
    recs = positions(manual_records(5, (0.0, 0.0), records=7))
    steps = [0, 3, 7, 8, 20, 21, 30]
    got = CR.table(recs, steps, 3, [(1, 1), (0, 2)], 4)
    assert [g[1]["origins"] for g in got] == [7, 6, 5] and [g[0]["bots_then"] for g in got] == [35, 30, 25]
    assert [g[0]["sum_steps"] for g in got] == [0, 30, sum(steps[r] - steps[r - 2] for r in range(2, 7))]
    assert got == plain_loop(recs, steps, 3, [(1, 1), (0, 2)], 4)


def test_negative_sums_compose_from_their_limbs():
    from particlerobotsimulations_amd import _capi
    ones = (1 << 64) - 1
    assert CR.limbs(-1) == [ones, ones, ones] and CR.limbs(-5) == [ones - 4, ones, ones]  # all-ones upper limbs
    assert CR.limbs(0) == [0, 0, 0] and CR.limbs(1 << 64) == [0, 1, 0] and CR.limbs(-(1 << 64)) == [0, ones, ones]
    assert CR.limbs(-(1 << 128) - 1) == [ones, ones, ones - 1] and CR.limbs((1 << 191) - 1) == [ones, ones, ones >> 1]
    most = ((1 << 31) - 1) * 2 * ((1 << 58) - 1) ** 2  # the largest sum there is: below 2^148
    for v in (0, 1, -1, 70 * 70 * UNIT, -70 * 70 * UNIT, (1 << 64) - 1, -(1 << 64), 1 << 127, -(1 << 128), most, -most,
              (1 << 191) - 1, -(1 << 191)):
        assert _capi.signed_192(CR.limbs(v)) == v, v
    assert most < 1 << 148
    row = _capi.pbCoherentRow(lag=2, nx=-2, ny=5, reserved=9, origins=5, sum_steps=60, bots_now=16, bots_then=12,
                              re=(C.c_ulonglong * 3)(*CR.limbs(-3 * UNIT)), im=(C.c_ulonglong * 3)(*CR.limbs(most)))
    d = _capi.coherent_row(row)
    assert d == {"lag": 2, "nx": -2, "ny": 5, "origins": 5, "sum_steps": 60, "bots_now": 16, "bots_then": 12,
                 "re": -3 * UNIT, "im": most}
    assert tuple(d) == CR.FIELDS
    # a lag whose density wave runs backwards: the reference's negative sums go through the same limbs
    rows = CR.table([np.zeros((3, 2), f32), np.array([[L / 2, 0.0]] * 3, f32)], [0, 1], 2, [(1, 0)], L_LOG2)
    assert rows[1][0]["re"] == -9 * UNIT and CR.limbs(rows[1][0]["re"]) == [(1 << 64) - 9 * UNIT, ones, ones]


def test_float64_bound_holds_for_the_reference():
    recs = float64_records()
    import particlerobotsimulations_amd as pb
    vectors = pb.half_plane_vectors(3)
    rows = CR.table(recs, [0, 1], 2, vectors, 3)[1]
    worst = 0.0
    for row, want in zip(rows, float64_products(recs, vectors, 3)):
        bound = product_bound(row["nx"], row["ny"], 3, 1000, 1000)
        for got, ref in ((row["re"], want.real), (row["im"], want.imag)):
            err = abs(got / 2.0 ** 60 - ref)
            worst = max(worst, err / bound)
            assert err <= bound, (row, err, bound)
    assert row["bots_now"] == row["bots_then"] == 1000 and 0.0 < worst < 1.0


# ---- 2. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimSetCoherent", "pbSimCoherentRecord", "pbSimGetCoherentInfo", "pbSimGetCoherent", "pbSimGetCoherentTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _analysis, _capi, host
    import particlerobotsimulations_amd as pb
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbCoherentRow) == 96
    assert "pbCoherentRow" in header and "typedef struct pbCoherentRow {         /* 96 bytes */" in header
    for line in ("#define PB_COHERENT_MAX_LAGS 64u", "#define PB_COHERENT_MAX_VECTORS 256u", "#define PB_COHERENT_BLOCKS 256u"):
        assert line in header
    assert (_capi.COHERENT_MAX_LAGS, _capi.COHERENT_MAX_VECTORS) == (64, 256)
    csrc = os.path.join(ROOT, "particlerobotsimulations_amd", "csrc")
    source = open(os.path.join(csrc, "pb_coherent.hip")).read()
    assert "static_assert(sizeof(pbCoherentRow) == 96" in source and '#include "pb_coherent.hpp"' in source
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert " pb_coherent.hip" in makefile and " pb_coherent.hpp" in makefile
    for name in ("pbHostSetCoherent", "pbHostCoherentRecord", "pbHostCoherentInfo", "pbHostCoherentRows"):
        assert hasattr(host.lib(), name)
    for name in ("set_coherent_scattering", "coherent_scattering_record", "coherent_scattering_info",
                 "coherent_scattering", "coherent_scattering_times"):
        assert hasattr(pb.Sim, name) and hasattr(pb.Ensemble, name)
    assert "coherent_scattering_summary" in pb.__all__
    assert [k for k, _ in _analysis.COHERENT_INFO] == ["interval", "lags", "box_log2", "nvec", "records"]
    block = header.split("Coherent intermediate scattering on the device")[1].split("#define PB_COHERENT_MAX_LAGS")[0]
    for word in ("rho_k(t + tau) conj(rho_k(t))", "PB_SK_DENSITY", "below 2^116", "below 2^117", "below 2^148",
                 "signed 192-bit", "a lag holds 2^31 origins or more", "derived, not measured", "(2 eps + eps^2)",
                 "distinct van Hove, coherent scattering", "never waits for the device", "not part of a checkpoint",
                 "(16 + 48)", "65535 members", "2^28 bots", "Current correlations".lower(), "256-bit products", "chi_4",
                 "logarithmic lag spacing", "radial averaging", "summary rows", "legacy engine"):
        assert word in block or word in re.sub(r"\s*\n \* ", " ", block), word
    # the two lists that used to name it as out of scope point here now
    flat = re.sub(r"\s*\n \* ", " ", header)
    assert "a caller can form it from pbSimStructureFactor per record" not in flat
    assert flat.count("pbSimSetCoherent, below") == 2 and "the coherent F(k, tau);" not in flat


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    lib = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    row = _capi.pbCoherentRow(lag=7, bots_now=7)
    vec = (C.c_int * 4)(1, 0, 0, 1)
    i, l, e, k, r, ms = C.c_float(7.0), C.c_uint(7), C.c_int(7), C.c_uint(7), C.c_ulonglong(7), C.c_float(7.0)

    def refused(rc, fn, word=None):
        msg = lib.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and fn.encode() in msg and (word is None or word.encode() in msg), (rc, msg)

    fn = "pbSimSetCoherent"
    refused(lib.pbSimSetCoherent(None, 0.05, 8, 3, vec, 2), fn, "null")
    refused(lib.pbSimSetCoherent(fake, 0.05, 8, 3, None, 2), fn, "null vectors")
    for bad in (-0.5, -2.0, -1e-30, np.nextafter(f32(-1.0), f32(0.0)), float("nan"), float("inf"), float("-inf")):
        refused(lib.pbSimSetCoherent(fake, float(bad), 8, 3, vec, 2), fn, "interval")
        refused(lib.pbSimSetCoherent(fake, float(bad), 0, 3, vec, 2), fn, "interval")  # switching off checks it too
    for bad in (65, 1 << 31):
        refused(lib.pbSimSetCoherent(fake, 0.05, bad, 3, vec, 2), fn, "lags")
        refused(lib.pbSimSetCoherent(fake, -1.0, bad, 3, vec, 2), fn, "lags")  # -1 is an interval
    for bad in (-9, 13, -(1 << 31), (1 << 31) - 1):
        refused(lib.pbSimSetCoherent(fake, 0.0, 8, bad, vec, 2), fn, "boxLog2")
    for bad in (0, 257, 1 << 31):
        refused(lib.pbSimSetCoherent(fake, 0.0, 8, 3, vec, bad), fn, "nvec")
    refused(lib.pbSimCoherentRecord(None), "pbSimCoherentRecord", "null")
    refused(lib.pbSimGetCoherentInfo(None, C.byref(i), C.byref(l), C.byref(e), C.byref(k), C.byref(r)),
            "pbSimGetCoherentInfo", "null")
    refused(lib.pbSimGetCoherentInfo(fake, None, None, None, None, None), "pbSimGetCoherentInfo", "all null")
    refused(lib.pbSimGetCoherent(None, C.byref(row)), "pbSimGetCoherent", "null")
    refused(lib.pbSimGetCoherent(fake, None), "pbSimGetCoherent", "null")
    refused(lib.pbSimGetCoherentTimes(None, C.byref(r), C.byref(ms)), "pbSimGetCoherentTimes", "null")
    assert (i.value, l.value, e.value, k.value, r.value, ms.value) == (7.0, 7, 7, 7, 7, 7.0)
    assert row.lag == 7 and row.bots_now == 7


# ---- 3. the runner and the host engine ---------------------------------------------------------------------------------

NOT_A_NUMBER = ["", "abc", "-1", "-1e-30", "nan", "inf", "-inf", "0.1x"]
BAD_FLAGS = ([("--coherent-interval", v) for v in NOT_A_NUMBER]
             + [("--coherent-lags", v) for v in ("", "0", "-3", "1.5", "65", "many")]
             + [("--coherent-box-log2", v) for v in ("", "-9", "13", "1.5", "big")]
             + [("--coherent-nmax", v) for v in ("", "0", "-1", "11", "2.5", "all")])  # 11: 264 vectors, past 256


@pytest.mark.parametrize("flag,value", BAD_FLAGS, ids=[f"{f}={v!r}" for f, v in BAD_FLAGS])
def test_runner_refuses_a_bad_coherent_value(tmp_path, flag, value):
    for args in ([flag, value], [CFG, "--coherent", "f.csv", flag, value, "--quiet"]):
        r = subprocess.run([RUN] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), args
    assert not os.listdir(tmp_path)


def test_runner_coherent_flags_need_their_values_and_the_fused_engine(tmp_path):
    flags = ("--coherent", "--coherent-interval", "--coherent-lags", "--coherent-box-log2", "--coherent-nmax")
    for flag in flags:
        r = subprocess.run([RUN, CFG, flag], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), flag
    said = "--coherent needs the fused engine (the recorder runs on its resident state)\n"
    for extra in ([], ["--coherent-interval", "0"], ["--coherent-interval", "3.4e38", "--coherent-lags", "1"],
                  ["--coherent-lags", "64", "--coherent-nmax", "10"], ["--coherent-box-log2", "-8"],
                  ["--coherent-box-log2", "12", "--coherent-nmax", "1"]):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--coherent", "f.csv"] + extra, capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", said), extra
    # last in the engine-check table: any earlier file flag speaks first
    for flag, line in (("--scatter", "--scatter needs the fused engine (the recorder runs on its resident state)\n"),
                       ("--vanhove-distinct",
                        "--vanhove-distinct needs the fused engine (the recorder runs on its resident state)\n")):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--coherent", "f.csv", flag, "a.csv"], capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stderr) == (2, line)
    assert not os.listdir(tmp_path)
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_runner.cpp")).read()
    for flag in ("--coherent FILE", "--coherent-interval T", "--coherent-lags N", "--coherent-box-log2 E", "--coherent-nmax M"):
        assert flag in source and flag in open(os.path.join(ROOT, "README.md")).read(), flag
        assert flag.split()[0] in open(os.path.join(ROOT, "INTEGRATION.md")).read(), flag
    assert "Lag, Nx, Ny, Origins, SumSteps, BotsNow, BotsThen, Re, Im, FRe, FIm" in source
    assert "coherent" not in USAGE  # the usage line stays as it is


NEEDS = "the coherent scattering needs the fused engine"
VEC = (C.c_int * 2)(1, 0)
REFUSED = [  # the host library's wrappers (HostSim has no methods for this recorder: a caller goes through host.lib())
    (lambda L, h: L.pbHostSetCoherent(h, 0.05, 8, 3, VEC, 1), "Particlebot::setCoherent: " + NEEDS + "\n"),
    (lambda L, h: L.pbHostCoherentRecord(h), "Particlebot::coherentRecord: " + NEEDS + "\n"),
    (lambda L, h: L.pbHostCoherentInfo(h, None, C.byref(C.c_uint(7)), None, None, None),
     "Particlebot::coherentInfo: " + NEEDS + "\n"),
]


@pytest.mark.parametrize("call,line", REFUSED, ids=["set", "record", "info"])
def test_host_engine_has_no_coherent_scattering(capfd, call, line):
    from particlerobotsimulations_amd import _capi, host
    h = host.HostSim(CFG, engine="host")
    capfd.readouterr()
    lib = host.lib()
    assert call(lib, h._h) == -1
    assert capfd.readouterr() == ("", line)
    # a NULL list with a count, and a NULL count, are refused before the class is asked; a refused call writes nothing
    assert lib.pbHostSetCoherent(h._h, 0.05, 8, 3, None, 1) == -1 and lib.pbHostCoherentRows(h._h, None, 0, None) == -1
    assert capfd.readouterr() == ("", "")
    row, count = _capi.pbCoherentRow(lag=7), C.c_ulonglong(7)
    assert lib.pbHostCoherentRows(h._h, C.byref(row), 1, C.byref(count)) == -1 and (row.lag, count.value) == (7, 7)
    assert capfd.readouterr() == ("", "Particlebot::coherentRows: " + NEEDS + "\n")
    h.close()


# ---- 4. the pure-Python helpers ----------------------------------------------------------------------------------------

def test_coherent_summary_on_known_integers():
    import particlerobotsimulations_amd as pb
    d = {"lag": 3, "nx": -2, "ny": 5, "origins": 5, "sum_steps": 60, "bots_now": 20, "bots_then": 16, "re": -3 * UNIT,
         "im": UNIT >> 1}
    assert pb.coherent_scattering_summary(d) == {"f_re": -3 / 16, "f_im": 1 / 32, "mean_lag_steps": 12.0}
    n = 70
    point = np.zeros((n, 2), f32)
    rows = CR.table([point, (point + np.array([2.0, 0.0], f32)).astype(f32)], [0, 10], 2, [(1, 0)], L_LOG2)
    assert pb.coherent_scattering_summary(rows[0][0]) == {"f_re": float(n), "f_im": 0.0, "mean_lag_steps": 0.0}  # S(k) = N
    assert pb.coherent_scattering_summary(rows[1][0]) == {"f_re": 0.0, "f_im": float(n), "mean_lag_steps": 10.0}
    # formed as one exact fraction from a 148-bit integer
    big = dict(d, bots_then=(1 << 28) - 1, re=((1 << 28) - 1) * UNIT * 3, im=-1)
    s = pb.coherent_scattering_summary(big)
    assert s["f_re"] == 3.0 and s["f_im"] == -1.0 / (((1 << 28) - 1) * UNIT)
    none = pb.coherent_scattering_summary(dict.fromkeys(CR.FIELDS, 0))
    assert none == {"f_re": None, "f_im": None, "mean_lag_steps": None}
