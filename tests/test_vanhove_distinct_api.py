"""CPU side of the distinct van Hove function (pbSimSetVanHoveDistinct / pbSimVanHoveDistinctRecord /
pbSimGetVanHoveDistinct, csrc/pb_vanhove_distinct.hip).

1. The radial bin rules the kernel can be built with agree with the binary search: tests/pb_vanhove_distinct_check.cpp
   as a stand-alone program, built plainly and under AddressSanitizer and UBSan.
2. The C-ABI entries are declared, exported and reject bad arguments before they touch the device.
3. The runner knows --vanhove-distinct and its options; the placement-only host engine has no such analysis.
4. row_dict on a pbVanHoveDistinctRow and van_hove_distinct_lists on known integers.
(tests/test_vanhove_distinct_ref.py holds the reference's own tests.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_runner_analysis_flags import USAGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "particlerobotsimulations_amd", "csrc")
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")
f32 = np.float32


# ---- 1. the bin rules ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []],
                         ids=["sanitized", "plain"])
def test_every_bin_rule_equals_the_binary_search(tmp_path, flags):
    exe = tmp_path / "pb_vanhove_distinct_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", *flags,
                    os.path.join(ROOT, "tests", "pb_vanhove_distinct_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pb_vanhove_distinct_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout


def test_the_kernel_file_is_built_as_the_issue_lays_it_out():
    source = open(os.path.join(CSRC, "pb_vanhove_distinct.hip")).read()
    for include in ('#include "pb_cluster.hpp"', '#include "pb_vanhove.hpp"', '#include "pb_fixed.hpp"'):
        assert include in source
    for rule in ("pbVhRadialBin(", "pbVhRadialBinFrom(", "pbVhRadialBinRoot("):  # all three behind one switch
        assert rule in source
    assert "#if PB_VHD_BIN_RULE == 0" in source and "#if PB_VHD_COMBINE" in source
    assert "pbWalkNine<false>" in source and "pbClusterFile(S, R / 1048576.0, 0.0)" in source
    assert "pb_vanhove_distinct.hip" in open(os.path.join(CSRC, "Makefile")).read()
    cluster = open(os.path.join(CSRC, "pb_cluster.hip")).read()
    assert cluster.count("int ensureScratch(") == 1 and "int pbClusterEnsureScratch(pbSim *S)" in cluster
    assert "ensureScratch" not in source.replace("pbClusterEnsureScratch", "")  # exposed, not duplicated
    engine = open(os.path.join(CSRC, "pb_engine.hip")).read()
    assert engine.index("pbVanHoveRecord(B)") < engine.index("pbVanHoveDistinctRecord(B)") < engine.index("trailRecord}")


# ---- 2. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimSetVanHoveDistinct", "pbSimVanHoveDistinctRecord", "pbSimGetVanHoveDistinctInfo",
         "pbSimGetVanHoveDistinct", "pbSimGetVanHoveDistinctTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi, host
    import particlerobotsimulations_amd as pb
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbVanHoveDistinctRow) == 48
    assert "pbVanHoveDistinctRow" in header and "Out of scope: the distinct part G_d" not in header
    source = open(os.path.join(CSRC, "pb_vanhove_distinct.hip")).read()
    assert "static_assert(sizeof(pbVanHoveDistinctRow) == 48" in source
    for name in ("pbHostSetVanHoveDistinct", "pbHostVanHoveDistinctRecord", "pbHostVanHoveDistinctInfo",
                 "pbHostVanHoveDistinctRows"):
        assert hasattr(host.lib(), name)
    for name in ("set_van_hove_distinct", "van_hove_distinct_record", "van_hove_distinct_info", "van_hove_distinct",
                 "van_hove_distinct_times"):
        assert hasattr(pb.Sim, name)
    for name in ("set_van_hove_distinct", "van_hove_distinct_record", "van_hove_distinct_info", "van_hove_distinct"):
        assert hasattr(host.HostSim, name)
    klass = open(os.path.join(ROOT, "include", "particlebot.h")).read()
    for name in ("setVanHoveDistinct(", "vanHoveDistinctRecord(", "vanHoveDistinctInfo(", "vanHoveDistinctRows("):
        assert name in klass


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    row = _capi.pbVanHoveDistinctRow(lag=7, centres=7)
    counts = (C.c_ulonglong * 5)(7, 7, 7, 7, 7)
    i, l, w, b, r, ms = C.c_float(7.0), C.c_uint(7), C.c_float(7.0), C.c_uint(7), C.c_ulonglong(7), C.c_float(7.0)

    def refused(rc, fn, word=None):
        msg = L.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and fn.encode() in msg and (word is None or word.encode() in msg), (rc, msg)

    fn = "pbSimSetVanHoveDistinct"
    refused(L.pbSimSetVanHoveDistinct(None, 0.05, 8, 0.125, 64), fn, "null")
    for bad in (-0.5, -2.0, -1e-30, np.nextafter(f32(-1.0), f32(0.0)), float("nan"), float("inf"), float("-inf")):
        refused(L.pbSimSetVanHoveDistinct(fake, float(bad), 8, 0.125, 64), fn, "interval")
        refused(L.pbSimSetVanHoveDistinct(fake, float(bad), 0, 0.125, 64), fn, "interval")  # switching off checks it too
    for bad in (65, 1 << 31):
        refused(L.pbSimSetVanHoveDistinct(fake, 0.05, bad, 0.125, 64), fn, "lags")
        refused(L.pbSimSetVanHoveDistinct(fake, -1.0, bad, 0.125, 64), fn, "lags")  # -1 is an interval
    for bad in (0, 1025, 1 << 31):
        refused(L.pbSimSetVanHoveDistinct(fake, 0.0, 8, 0.125, bad), fn, "bins")
    for bad in (0.0, -0.125, 2048.0, 1e30, float("nan"), float("inf"), float("-inf")):
        refused(L.pbSimSetVanHoveDistinct(fake, 0.0, 8, float(bad), 64), fn, "binWidth")
    for bad in (2.0 ** -21, 2.0 ** -22, 1e-30):  # rint(w 2^20) == 0 (a tie goes to even): no quantum
        refused(L.pbSimSetVanHoveDistinct(fake, 0.0, 8, float(bad), 64), fn, "quantum")
    # qw bins >= 2^31: rMax would reach 2048
    for width, bins in ((32.0, 64), (2.0, 1024), (1024.0, 2), (2047.5, 2), (2.0 + 2.0 ** -8, 1023), (2047.99, 2)):
        refused(L.pbSimSetVanHoveDistinct(fake, 0.0, 8, width, bins), fn, "below 2048")
    refused(L.pbSimVanHoveDistinctRecord(None), "pbSimVanHoveDistinctRecord", "null")
    refused(L.pbSimGetVanHoveDistinctInfo(None, C.byref(i), C.byref(l), C.byref(w), C.byref(b), C.byref(r)),
            "pbSimGetVanHoveDistinctInfo", "null")
    refused(L.pbSimGetVanHoveDistinctInfo(fake, None, None, None, None, None), "pbSimGetVanHoveDistinctInfo", "all null")
    refused(L.pbSimGetVanHoveDistinct(None, C.byref(row), counts), "pbSimGetVanHoveDistinct", "null")
    refused(L.pbSimGetVanHoveDistinct(fake, None, None), "pbSimGetVanHoveDistinct", "both null")
    refused(L.pbSimGetVanHoveDistinctTimes(None, C.byref(r), C.byref(ms)), "pbSimGetVanHoveDistinctTimes", "null")
    assert (i.value, l.value, w.value, b.value, r.value, ms.value) == (7.0, 7, 7.0, 7, 7, 7.0)
    assert row.lag == 7 and row.centres == 7 and list(counts) == [7] * 5


# ---- 3. the runner and the host engine ---------------------------------------------------------------------------------

NOT_A_NUMBER = ["", "abc", "-1", "-1e-30", "nan", "inf", "-inf", "0.1x"]
BAD_FLAGS = ([("--vanhove-distinct-interval", v) for v in NOT_A_NUMBER]
             + [("--vanhove-distinct-lags", v) for v in ("", "0", "-3", "1.5", "65", "many")]
             + [("--vanhove-distinct-width", v) for v in NOT_A_NUMBER + ["0", "2048", "1e30"]]
             + [("--vanhove-distinct-bins", v) for v in ("", "0", "-1", "1025", "2.5", "all")])


@pytest.mark.parametrize("flag,value", BAD_FLAGS, ids=[f"{f}={v!r}" for f, v in BAD_FLAGS])
def test_runner_refuses_a_bad_value(tmp_path, flag, value):
    for args in ([flag, value], [CFG, "--vanhove-distinct", "f.csv", flag, value, "--quiet"]):
        r = subprocess.run([RUN] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), args
    assert not os.listdir(tmp_path)


def test_runner_flags_need_their_values_and_the_fused_engine(tmp_path):
    flags = ("--vanhove-distinct", "--vanhove-distinct-interval", "--vanhove-distinct-lags", "--vanhove-distinct-width",
             "--vanhove-distinct-bins")
    for flag in flags:
        r = subprocess.run([RUN, CFG, flag], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), flag
    said = "--vanhove-distinct needs the fused engine (the recorder runs on its resident state)\n"
    for extra in ([], ["--vanhove-distinct-interval", "0"], ["--vanhove-distinct-lags", "64", "--vanhove-distinct-bins", "1024"],
                  ["--vanhove-distinct-width", "1e-6"], ["--vanhove-distinct-width", "2047.9", "--vanhove-distinct-bins", "1"]):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--vanhove-distinct", "f.csv"] + extra, capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", said), extra
    # last in the engine-check table: any earlier recorder speaks first
    for flag, line in (("--vanhove", "--vanhove needs the fused engine (the recorder runs on its resident state)\n"),
                       ("--timecorr", "--timecorr needs the fused engine (the recorder runs on its resident state)\n")):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--vanhove-distinct", "f.csv", flag, "a.csv"],
                           capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stderr) == (2, line)
    assert not os.listdir(tmp_path)
    source = open(os.path.join(CSRC, "pb_runner.cpp")).read()
    for flag in ("--vanhove-distinct FILE", "--vanhove-distinct-interval T", "--vanhove-distinct-lags N",
                 "--vanhove-distinct-width W", "--vanhove-distinct-bins B"):
        assert flag in source and flag in open(os.path.join(ROOT, "README.md")).read(), flag
        assert flag.split()[0] in open(os.path.join(ROOT, "INTEGRATION.md")).read(), flag
    assert "Lag, Origins, SumSteps, Centres, Partners, Pairs, Bin, Lower, Count" in source
    assert "vanhove" not in USAGE  # the usage line stays as it is


NEEDS = "the distinct van Hove function needs the fused engine"
REFUSED = [
    (lambda h: h.set_van_hove_distinct(0.05, 8, 0.125, 64),
     "set_van_hove_distinct: " + NEEDS + ", a finite interval >= 0 (or -1), lags <= 64, 1 ... 1024 bins and a width "
     "with bins * width < 2048", "Particlebot::setVanHoveDistinct: " + NEEDS + "\n"),
    (lambda h: h.van_hove_distinct_record(), "van_hove_distinct_record: " + NEEDS + " and the analysis on",
     "Particlebot::vanHoveDistinctRecord: " + NEEDS + "\n"),
    (lambda h: h.van_hove_distinct_info(), "van_hove_distinct_info: " + NEEDS,
     "Particlebot::vanHoveDistinctInfo: " + NEEDS + "\n"),
    (lambda h: h.van_hove_distinct(), "van_hove_distinct_info: " + NEEDS,
     "Particlebot::vanHoveDistinctInfo: " + NEEDS + "\n"),
]


@pytest.mark.parametrize("call,error,line", REFUSED, ids=["set", "record", "info", "rows"])
def test_host_engine_has_no_distinct_van_hove(capfd, call, error, line):
    from particlerobotsimulations_amd import _capi, host
    h = host.HostSim(CFG, engine="host")
    capfd.readouterr()
    with pytest.raises(RuntimeError) as caught:
        call(h)
    assert str(caught.value) == error
    assert capfd.readouterr() == ("", line)
    # the wrapper: a NULL count is refused before the class is asked; a refused call writes nothing
    L = host.lib()
    assert L.pbHostVanHoveDistinctRows(h._h, None, None, 0, None) == -1
    assert capfd.readouterr() == ("", "")
    row, counts, count = _capi.pbVanHoveDistinctRow(lag=7), (C.c_ulonglong * 5)(7, 7, 7, 7, 7), C.c_ulonglong(7)
    assert L.pbHostVanHoveDistinctRows(h._h, C.byref(row), counts, 1, C.byref(count)) == -1
    assert (row.lag, count.value, list(counts)) == (7, 7, [7] * 5)
    assert capfd.readouterr() == ("", "Particlebot::vanHoveDistinctRows: " + NEEDS + "\n")
    h.close()


# ---- 4. the pure-Python helpers ----------------------------------------------------------------------------------------

def test_rows_and_lists_on_known_integers():
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import _capi
    import vanhove_distinct_ref as DR
    rows = (_capi.pbVanHoveDistinctRow * 4)()
    for g in range(4):
        rows[g] = _capi.pbVanHoveDistinctRow(lag=g % 2, reserved=0, origins=5 - g % 2, sum_steps=60 * (g % 2),
                                             centres=(1 << 40) + g, partners=(1 << 33) + g, pairs=9 * g + 3)
    counts = (C.c_ulonglong * 12)(*range(12))
    d = _capi.row_dict(rows[3])
    assert d == {"lag": 1, "origins": 4, "sum_steps": 60, "centres": (1 << 40) + 3, "partners": (1 << 33) + 3, "pairs": 30}
    assert tuple(d) == DR.FIELDS
    out = pb.van_hove_distinct_lists(rows, counts, 2, 2, 3)
    assert [[r["counts"] for r in member] for member in out] == [[[0, 1, 2], [3, 4, 5]], [[6, 7, 8], [9, 10, 11]]]
    assert out[1][1] == dict(d, counts=[9, 10, 11]) and all(r["pairs"] == sum(r["counts"]) for m in out for r in m)
