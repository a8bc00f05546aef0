"""CPU side of the strain analysis (pbSimStrainStats / pbSimStrainOf, csrc/pb_strain.hip and pb_strain.hpp).

1. tests/strain_ref.py, the reference the GPU tests compare against: it equals an O(n^2) brute force written
   independently (Python ints and Python floats, no shared code), and gives hand-built known answers.
2. The shared fit function as plain C++ (tests/pb_strain_check.cpp), over a table of moments the reference also
   evaluates: the doubles are compared as bit patterns.
3. The C-ABI entries are declared, exported and reject bad arguments before they touch the device; the runner knows
   --strain and its option; the placement-only host engine has no analysis.
4. deformation_gradient and mean_d2min on known integers."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import cluster_ref as CR
import dynamics_ref as DR
import strain_ref as SR
from helpers import jittered_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "particlerobotsimulations_amd", "csrc")
f32 = np.float32
GAPS = [0.0, 0.0019, 0.3]


def cfg_path(name):
    return os.path.join(ROOT, "examples", name)


# ---- 1. the reference --------------------------------------------------------------------------------------------------

def brute(pos0, rad0, pos1, gap):
    """Per bot (moments as Python ints, dropped, fitted, J, d2) with nothing of strain_ref in it: the links from the
    cluster reference's pair predicate over all pairs, the quantiser as Python's round (ties to even) of the exact
    product, the fit in Python floats."""
    pos0 = np.asarray(pos0, f32).reshape(-1, 2)
    pos1 = np.asarray(pos1, f32).reshape(-1, 2)
    rad0 = np.asarray(rad0, f32)
    n = rad0.size
    ok = np.isfinite(pos0).all(axis=1) & np.isfinite(rad0)
    out = []
    for i in range(n):
        hit = np.zeros(n, bool)
        if ok[i]:
            hit = CR.linked(pos0[i, 0], pos0[i, 1], rad0[i], pos0[:, 0], pos0[:, 1], rad0, gap) & ok
            hit[i] = False
        m, dropped = [0] * 9, 0
        for j in np.flatnonzero(hit):
            with np.errstate(all="ignore"):
                d = [float(f32(pos0[j, 0] - pos0[i, 0])), float(f32(pos0[j, 1] - pos0[i, 1])),
                     float(f32(pos1[j, 0] - pos1[i, 0])), float(f32(pos1[j, 1] - pos1[i, 1]))]
            if not all(abs(v) < 8.0 for v in d):  # (a NaN fails the comparison)
                dropped += 1
                continue
            a, b, x, y = (round(v * 1048576.0) for v in d)  # exact product, ties to even
            for k, v in enumerate((1, a * a, a * b, b * b, x * a, x * b, y * a, y * b, x * x + y * y)):
                m[k] += v
        A, B, Cc, xxx, xxy, xyx, xyy, w = (float(v) for v in m[1:])
        det = A * Cc - B * B
        fitted = m[0] >= 3 and det > 0
        J, d2 = (0.0, 0.0, 0.0, 0.0), 0.0
        if fitted:
            J = ((xxx * Cc - xxy * B) / det, (xxy * A - xxx * B) / det, (xyx * Cc - xyy * B) / det,
                 (xyy * A - xyx * B) / det)
            d2 = w - ((J[0] * xxx + J[1] * xxy) + (J[2] * xyx + J[3] * xyy))
            d2 = d2 if d2 > 0 else 0.0
        out.append((m, dropped, fitted, J, d2))
    return out


def bits(v):
    return struct.pack("<d", float(v))


def test_reference_equals_brute_force():
    rng = np.random.default_rng(2300)
    pos, _, rad = jittered_blob(300, 0.15, rng, jitter=0.3)
    pos1 = DR.perturbed(pos, rng)
    pos1[17] = np.nan          # a bot that is lost on the way: its partners drop their bond to it
    pos1[40, 0] += f32(9.0)    # a bot carried away
    for gap in GAPS:
        row, bots = SR.analyse(pos, rad, pos1, gap, threshold=0.0005)
        want = brute(pos, rad, pos1, gap)
        for i, (m, dropped, fitted, J, d2) in enumerate(want):
            assert [int(v) for v in bots["moments"][i]] == m, (gap, i)
            assert int(bots["dropped"][i]) == dropped and bool(bots["fitted"][i]) == fitted, (gap, i)
            assert [bits(v) for v in bots["gradient"][i].reshape(-1)] == [bits(v) for v in J], (gap, i)
            assert bits(bots["d2min"][i]) == bits(d2), (gap, i)
        assert row["fitted"] == sum(w[2] for w in want) and row["fitted"] + row["unfitted"] == 300
        assert row["bonds_used"] == sum(w[0][0] for w in want) and row["bonds_dropped"] == sum(w[1] for w in want)
        for k, name in enumerate(SR.MOMENTS):
            if k:
                assert row[name] == sum(w[0][k] for w in want), (gap, name)
        e = [int(round(w[4])) for w in want if w[2]]
        assert row["sum_d2"] == sum(e) and row["max_d2"] == max(e)
        assert row["above"] == sum(1 for w in want if w[2] and w[4] > float(f32(0.0005)) * 2.0 ** 40)
        assert 0 < row["above"] <= row["fitted"] and row["bonds_dropped"] > 0, (gap, row)
        assert row["above"] < row["fitted"] or gap == 0.3, (gap, row)  # (long lists: every bot has some residual)
        assert int(bots["moments"][17, 0]) == 0 and not bots["fitted"][17]
        # the scalar statement of the fit and the array one are the same function
        for i in (0, 17, 40, 150, 299):
            ok, J, d2 = SR.fit([int(v) for v in bots["moments"][i]])
            assert ok == bool(bots["fitted"][i]) and bits(d2) == bits(bots["d2min"][i])
            assert [bits(v) for v in J] == [bits(v) for v in bots["gradient"][i].reshape(-1)]


@pytest.mark.parametrize("n", [63, 257, 1025])
def test_the_gpu_tests_recipe_populates_every_class(n):
    rng = np.random.default_rng(2000 + n)
    pos, _, rad = jittered_blob(n, 0.15, rng, jitter=0.3)
    row, _ = SR.analyse(pos, rad, DR.perturbed(pos, rng), 0.0019)
    assert 0 < row["fitted"] < n and 0 < row["unfitted"] and row["sum_d2"] > 0 and row["bonds_dropped"] == 0


def square_lattice(side, spacing=0.25):
    ij = np.array([(i, j) for j in range(side) for i in range(side)], np.float64)
    return (ij * spacing).astype(f32), np.full(side * side, spacing / 2, f32)


def test_the_identity_gives_the_unit_gradient_and_no_residual():
    rng = np.random.default_rng(7)
    pos, _, rad = jittered_blob(200, 0.15, rng, jitter=0.3)
    row, bots = SR.analyse(pos, rad, pos, 0.05)
    fit = bots["fitted"]
    assert 100 < row["fitted"] == int(fit.sum()) and row["sum_d2"] == 0 and row["max_d2"] == 0 and row["above"] == 0
    assert (bots["gradient"][fit] == np.eye(2)).all() and (bots["d2min"] == 0.0).all()
    assert (bots["gradient"][~fit] == 0.0).all()
    assert row["yxx"] == row["xxx"] and row["yxy"] == row["xxy"] == row["xyx"] and row["yyy"] == row["xyy"]
    assert row["w"] == row["yxx"] + row["yyy"]


def test_a_collinear_triple_and_a_bot_with_two_bonds_are_unfitted():
    # five bots in a row: the inner ones have 2 bonds, and with a gap that reaches the second neighbour 3 or 4, all
    # collinear: det = 0
    rad = np.full(5, 0.1, f32)
    pos = np.zeros((5, 2), f32)
    pos[:, 0] = np.arange(5) * 0.25
    for gap, most in ((0.1, 2), (0.35, 4)):
        row, bots = SR.analyse(pos, rad, pos * f32(1.5), gap)
        assert int(bots["moments"][:, 0].max()) == most and row["fitted"] == 0 and row["unfitted"] == 5
        assert (bots["moments"][:, 2] == 0).all() and (bots["moments"][:, 3] == 0).all()  # Yxy = Yyy = 0
        assert (bots["gradient"] == 0.0).all() and (bots["d2min"] == 0.0).all() and row["sum_d2"] == 0
        assert row["bonds_used"] == int(bots["moments"][:, 0].sum()) > 0 and row["w"] > 0
    # an L: the corner has two bonds that span the plane and is unfitted all the same (k < 3)
    pos = np.array([[0.0, 0.0], [0.25, 0.0], [0.0, 0.25]], f32)
    row, bots = SR.analyse(pos, rad[:3], pos, 0.1)
    assert bots["moments"][0, 0] == 2 and row["fitted"] == 0
    a = 1 << 18
    assert [int(v) for v in bots["moments"][0]] == [2, a * a, 0, a * a, a * a, 0, 0, a * a, 2 * a * a]


def test_a_lattice_under_an_exactly_representable_shear_has_no_residual():
    pos, rad = square_lattice(6)
    shear = np.array([[1.0, 0.5], [0.0, 1.0]])                       # x' = x + y / 2: exact in fp32 on this lattice
    pos1 = (pos.astype(np.float64) @ shear.T + np.array([3.0, -2.0])).astype(f32)
    row, bots = SR.analyse(pos, rad, pos1, 0.01)
    k = bots["moments"][:, 0]
    assert sorted(set(k.tolist())) == [2, 3, 4] and row["bonds_dropped"] == 0
    fit = bots["fitted"]
    assert np.array_equal(fit, k >= 3) and row["fitted"] == 32 and row["unfitted"] == 4   # the four corners
    assert (bots["gradient"][fit] == shear).all() and (bots["d2min"] == 0.0).all() and row["sum_d2"] == 0
    import particlerobotsimulations_amd as pb
    assert (pb.deformation_gradient(row) == shear).all() and pb.mean_d2min(row) == 0.0
    # a rotation by 90 degrees and a dilation, exact too
    for F in (np.array([[0.0, -1.0], [1.0, 0.0]]), np.array([[2.0, 0.0], [0.0, 2.0]])):
        row, bots = SR.analyse(pos, rad, (pos.astype(np.float64) @ F.T).astype(f32), 0.01)
        assert (bots["gradient"][fit] == F).all() and row["sum_d2"] == 0 and (pb.deformation_gradient(row) == F).all()
    # one bot of the sheared lattice pushed aside: it and its four partners, and nobody else, get a residual
    pos2 = pos1.copy()
    pos2[14] += np.array([0.0625, 0.0], f32)
    row, bots = SR.analyse(pos, rad, pos2, 0.01, threshold=0.0)
    assert sorted(np.flatnonzero(bots["d2min"] > 0).tolist()) == [8, 13, 14, 15, 20] and row["above"] == 5


def test_the_reach_of_a_bond():
    below = np.nextafter(f32(8.0), f32(0.0))
    rad = np.full(4, 0.1, f32)
    pos = np.array([[0.0, 0.0], [0.2, 0.0], [0.0, 0.2], [-0.2, 0.0]], f32)   # bot 0 with three partners
    for reach, used in ((f32(8.0), 2), (below, 3)):
        pos1 = pos.copy()
        pos1[1, 0] = reach       # dx of the bond 0-1 is exactly `reach`
        row, bots = SR.analyse(pos, rad, pos1, 0.01)
        assert int(bots["moments"][0, 0]) == used and int(bots["dropped"][0]) == 3 - used
        assert bool(bots["fitted"][0]) == (used == 3)
    assert int(np.rint(below * f32(1048576.0))) == 1 << 23  # the largest q: the tie goes to even
    assert int(bots["moments"][0, 8]) >= (1 << 46)


# ---- 2. the shared fit function, as plain C++ -----------------------------------------------------------------------------

def moment_table():
    rng = np.random.default_rng(99)
    pos, _, rad = jittered_blob(400, 0.15, rng, jitter=0.3)
    table = []
    for gap, pos1 in ((0.0019, DR.perturbed(pos, rng)), (0.3, DR.perturbed(pos, rng, shift=-3.0)), (0.05, pos),
                      (0.3, pos * f32(12.0))):
        table += [[int(v) for v in m] for m in SR.analyse(pos, rad, pos1, gap)[1]["moments"]]
    q = 1 << 23
    table += [[0] * 9, [3, 5, 0, 5, 5, 0, 0, 5, 10], [2, 5, 0, 5, 5, 0, 0, 5, 10], [3, 4, 2, 1, 9, 9, 9, 9, 100],
              [3, 1, 0, 1, -7, 3, 2, -5, 0],                              # a W too small for the fit: d2 clamps to 0
              [65535, 65535 * q * q, 0, 65535 * q * q, -65535 * q * q, 0, 0, -65535 * q * q, 2 * 65535 * q * q],
              [4, (1 << 62) + 1, (1 << 61) + 3, (1 << 60) + 1, -(1 << 62) + 5, 12345, -(1 << 59) - 1, 7, (1 << 62) - 1],
              [3, 1 << 62, (1 << 62) - 1024, 1 << 62, 1 << 62, -(1 << 62), 1 << 61, 1 << 60, 5]]  # ill-conditioned
    return table


@pytest.mark.parametrize("flags", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], []],
                         ids=["sanitized", "plain"])
def test_the_fit_as_plain_cpp_equals_the_reference_bit_for_bit(tmp_path, flags):
    exe = tmp_path / "pb_strain_check"
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", *flags,
                    os.path.join(ROOT, "tests", "pb_strain_check.cpp"), "-o", str(exe)], check=True)
    table = moment_table()
    text = "".join(" ".join(str(v) for v in m) + "\n" for m in table)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == f"pb_strain_check ok: {len(table)} rows" and "FAILED" not in r.stdout
    fitted = 0
    for m, line in zip(table, lines):
        ok, J, d2 = SR.fit(m)
        want = "%d %s %s %s %s %s %d" % (ok, *[bits(v)[::-1].hex() for v in (*J, d2)], SR.units(d2) if ok else 0)
        assert line == want, (m, line, want)
        fitted += ok
    assert 1000 < fitted < len(table) - 10
    assert SR.fit(table[-4])[0] and SR.fit(table[-4])[2] == 0.0
    # (the program checks its own units at 2^63 and beyond; the reference's are the same)
    assert SR.units(np.float64(2.0 ** 63)) == SR.units(np.float64(1e300)) == 1 << 63 and SR.units(np.float64(2.5)) == 2


# ---- 3. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimStrainStats", "pbSimStrainOf", "pbSimGetStrainTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi, host
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbStrainStats) == 184 and "pbStrainStats" in header and "/* 184 bytes */" in header
    assert "#define PB_STRAIN_REACH 8.0f" in header
    source = open(os.path.join(CSRC, "pb_strain.hip")).read()
    assert "static_assert(sizeof(pbStrainStats) == 184" in source and "pbClusterFile" not in source
    for name in ("pbHostStrainStats", "pbHostStrainOf"):
        assert hasattr(host.lib(), name)
    ens = open(os.path.join(ROOT, "include", "particlebot_ensemble.h")).read()
    assert "Strain" not in ens
    assert tuple(n for n, _ in _capi.pbStrainStats._fields_ if n != "reserved") == SR.FIELDS
    assert _capi.PB_STRAIN_MOMENTS == SR.MOMENTS


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    row = _capi.pbStrainStats()
    mom = np.zeros(9, np.int64)
    runs, ms = C.c_ulonglong(7), C.c_float(7.0)

    def refused(rc, fn, word=None):
        msg = L.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and fn.encode() in msg and (word is None or word.encode() in msg), (rc, msg)

    refused(L.pbSimStrainStats(None, 0.0, C.byref(row)), "pbSimStrainStats")
    refused(L.pbSimStrainStats(fake, 0.0, None), "pbSimStrainStats")
    for t in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        refused(L.pbSimStrainStats(fake, t, C.byref(row)), "pbSimStrainStats", "d2Threshold")
    refused(L.pbSimStrainOf(None, 0, _capi.np_ptr(mom), None, None), "pbSimStrainOf")
    refused(L.pbSimStrainOf(fake, 0, None, None, None), "pbSimStrainOf", "all null")
    refused(L.pbSimGetStrainTimes(None, C.byref(runs), C.byref(ms)), "pbSimGetStrainTimes")
    assert runs.value == 7 and ms.value == 7.0 and not mom.any() and row.fitted == 0 and row.max_d2 == 0


def test_runner_knows_the_strain_flags(tmp_path):
    exe = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
    source = open(os.path.join(CSRC, "pb_runner.cpp")).read()
    synopsis = source[:source.index("#include")]
    assert "[--strain FILE [--strain-threshold T]" in synopsis
    assert '{"--strain", &RunOptions::strainPath, "analysis"}' in source and '{"--strain-threshold"' in source
    for extra in ([], ["--rearrange-window"], ["--strain-threshold", "0.001"], ["--rearrange-gap", "0.0019"]):
        r = subprocess.run([exe, cfg_path("example.cfg"), "--engine", "legacy", "--strain", "a.csv"] + extra,
                           capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "--strain needs the fused engine" in r.stderr and not os.listdir(tmp_path)
    for bad in ("-1", "wide", "nan", "inf", "0.1x"):
        r = subprocess.run([exe, cfg_path("example.cfg"), "--strain", "a.csv", "--strain-threshold", bad],
                           capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "usage" in r.stderr, bad
        assert not os.listdir(tmp_path)
    r = subprocess.run([exe, cfg_path("example.cfg"), "--strain"], capture_output=True, text=True, timeout=60,
                       cwd=tmp_path)
    assert r.returncode == 2 and "usage" in r.stderr and not os.listdir(tmp_path)


def test_host_engine_has_no_strain_analysis():
    from particlerobotsimulations_amd import host
    h = host.HostSim(cfg_path("example.cfg"), engine="host")
    with pytest.raises(RuntimeError):
        h.strain()
    with pytest.raises(RuntimeError):
        h.strain_of()
    with pytest.raises(IndexError):
        h.strain_of(member=1)


# ---- 4. the pure-Python helpers ----------------------------------------------------------------------------------------

def test_deformation_gradient_and_mean_d2min_on_known_integers():
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import _capi
    assert "deformation_gradient" in pb.__all__ and "mean_d2min" in pb.__all__
    one = 1 << 40
    # Y = diag(8, 2), X = F Y with F = [[1.5, -0.25], [0.5, 2]]
    row = {"yxx": 8 * one, "yxy": 0, "yyy": 2 * one, "xxx": 12 * one, "xxy": -one // 2, "xyx": 4 * one, "xyy": 4 * one,
           "fitted": 4, "sum_d2": 3 * one}
    assert (pb.deformation_gradient(row) == np.array([[1.5, -0.25], [0.5, 2.0]])).all()
    assert pb.mean_d2min(row) == 0.75
    # beyond 2^64 and beyond what a double holds exactly: the quotients are formed from the integers
    big = (1 << 70) + 1
    row = {"yxx": big, "yxy": 0, "yyy": big, "xxx": 3 * big, "xxy": 0, "xyx": 0, "xyy": -big, "fitted": 1 << 20,
           "sum_d2": big << 20}
    assert (pb.deformation_gradient(row) == np.array([[3.0, 0.0], [0.0, -1.0]])).all()
    assert pb.mean_d2min(row) == float(big) / 2.0 ** 40
    flat = dict(row, yyy=0)
    assert np.isnan(pb.deformation_gradient(flat)).all() and np.isnan(pb.mean_d2min(dict(row, fitted=0)))
    r = _capi.pbStrainStats(fitted=5, unfitted=2, above=1, reserved=0, bonds_used=30, bonds_dropped=3, max_d2=11)
    r.xxy.lo, r.xxy.hi = 7, -1
    r.w.lo, r.w.hi = 9, 1 << 40
    d = _capi.row_dict(r)
    assert d["xxy"] == 7 - (1 << 32) and d["w"] == (1 << 72) + 9 and d["fitted"] == 5 and d["bonds_dropped"] == 3
    assert tuple(d) == SR.FIELDS
