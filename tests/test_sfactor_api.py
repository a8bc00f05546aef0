"""CPU side of the structure factor (pbSimStructureFactor / pbSimStructureFactorOf, csrc/pb_sfactor.hip): the C-ABI
entries are declared, exported and reject bad arguments before they touch the device; the Python wrappers check and pass
on their arguments; the runner knows --sk and its options; the placement-only host engine has no structure factor.
(The refusals that read the batch -- a member out of range, members x nvec x 80 bytes above 2^31 -- need a batch and are
in tests/test_gpu_sfactor.py; a batch of 2^28 bots is not built anywhere in the suite, as for the other analyses.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sfactor_ref as KR
from test_runner_analysis_flags import USAGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
CFG = os.path.join(ROOT, "examples", "example.cfg")

NAMES = ("pbSimStructureFactor", "pbSimStructureFactorOf", "pbSimGetStructureFactorTimes", "pbPhasorTable")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi, host
    import particlerobotsimulations_amd as pb
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbStructureFactorRow) == 80 and _capi.SK_ROW_DTYPE.itemsize == 80
    for text in ("#define PB_SK_MAX_VECTORS 4096u", "/* 80 bytes */", "PB_SK_MIN_LOG2 = -8", "PB_SK_MAX_LOG2 = 12",
                 "#define PB_SK_BLOCKS 256u", "#define PB_PHASOR_BITS 12",
                 "enum { PB_SK_DENSITY = 0, PB_SK_RADIUS = 1, PB_SK_VELOCITY = 2 }", "3228437924"):
        assert text in header, text
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_sfactor.hip")).read()
    assert "static_assert(sizeof(pbStructureFactorRow) == 80" in source
    assert hasattr(host.lib(), "pbHostStructureFactor")
    for name in ("structure_factor_values", "half_plane_vectors", "phasor_table"):
        assert name in pb.__all__
    block = header.split("Structure factor on the device")[1].split("#define PB_SK_MAX_VECTORS")[0]
    for word in ("self-intermediate scattering", "phase moments", "finer table", "radial averaging", "series ring",
                 "summary rows", "the legacy engine", "pi / 4096 + 2 pi (|nx| + |ny|) 2^-21 / L + 2^-30"):
        assert word in block, word


BAD = {
    "kind -1": dict(kind=-1), "kind 3": dict(kind=3), "boxLog2 -9": dict(e=-9), "boxLog2 13": dict(e=13),
    "nvec 0": dict(nvec=0), "nvec 4097": dict(nvec=4097),
}


@pytest.mark.parametrize("name", list(BAD))
def test_a_bad_argument_is_rejected_before_the_device_is_touched(name):
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    a = dict(kind=0, e=4, nvec=2)
    a.update(BAD[name])
    vec = (C.c_int * (2 * 4097))()
    row = _capi.pbStructureFactorRow(measured=7)
    rc = L.pbSimStructureFactor(fake, a["kind"], a["e"], vec, a["nvec"], C.byref(row))
    assert rc == 2 and b"pbSimStructureFactor:" in L.pbGetLastErrorString(), (name, rc, L.pbGetLastErrorString())
    rc = L.pbSimStructureFactorOf(fake, 0, a["kind"], a["e"], vec, a["nvec"], C.byref(row))
    assert rc == 2 and b"pbSimStructureFactorOf:" in L.pbGetLastErrorString(), (name, rc, L.pbGetLastErrorString())
    assert row.measured == 7


def test_null_arguments_are_rejected():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    fake = C.c_void_p(1)
    vec, row = (C.c_int * 4)(), _capi.pbStructureFactorRow(measured=7)
    n, ms = C.c_ulonglong(7), C.c_float(7.0)
    for rc in (L.pbSimStructureFactor(None, 0, 4, vec, 2, C.byref(row)),
               L.pbSimStructureFactor(fake, 0, 4, None, 2, C.byref(row)),
               L.pbSimStructureFactor(fake, 0, 4, vec, 2, None),
               L.pbSimStructureFactorOf(None, 0, 0, 4, vec, 2, C.byref(row)),
               L.pbSimStructureFactorOf(fake, 0, 0, 4, None, 2, C.byref(row)),
               L.pbSimStructureFactorOf(fake, 0, 0, 4, vec, 2, None),
               L.pbSimGetStructureFactorTimes(None, C.byref(n), C.byref(ms)),
               L.pbPhasorTable(None, 8192)):
        assert rc == 2 and b"null" in L.pbGetLastErrorString()
    assert (row.measured, n.value, ms.value) == (7, 7, 7.0)
    small = (C.c_int * 8191)()
    assert L.pbPhasorTable(small, 8191) == 2 and b"8192" in L.pbGetLastErrorString()


class FakeBatch:
    """A Sim or an Ensemble around a handle that is never dereferenced: what the wrappers do before the engine's own
    checks, and that they pass the engine's refusals on."""

    def __init__(self, cls, nsims=None):
        self.obj = object.__new__(cls)
        self.obj._h = C.c_void_p(1)
        if nsims is not None:
            self.obj.nsims = nsims

    def __enter__(self):
        return self.obj

    def __exit__(self, *exc):
        self.obj._h = None  # (nothing to destroy)


@pytest.mark.parametrize("which", ["Sim", "Ensemble"])
def test_wrappers_check_and_pass_on_their_arguments(which):
    import particlerobotsimulations_amd as pb
    with FakeBatch(getattr(pb, which), None if which == "Sim" else 3) as sim:
        for bad in ([1, 2, 3], [[1.5, 2.0]], [[1, 2, 3]], [[1 << 31, 0]], [[0, -(1 << 31) - 1]], 7):
            with pytest.raises(ValueError, match="structure_factor: "):
                sim.structure_factor(bad, 4)
        with pytest.raises(ValueError, match="kind must be 'density', 'radius' or 'velocity'"):
            sim.structure_factor([[1, 0]], 4, kind="charge")
        for member in (None, 0):
            fn = "pbSimStructureFactor" if member is None else "pbSimStructureFactorOf"
            with pytest.raises(RuntimeError, match="code 2.*%s: kind" % fn):
                sim.structure_factor([[1, 0]], 4, kind=5, member=member)
            with pytest.raises(RuntimeError, match="code 2.*%s: boxLog2 must be -8 ... 12" % fn):
                sim.structure_factor([[1, 0]], 13, member=member)
            with pytest.raises(RuntimeError, match="code 2.*%s: boxLog2" % fn):
                sim.structure_factor([[1, 0]], -9, kind="radius", member=member)
            with pytest.raises(RuntimeError, match="code 2.*%s: nvec must be 1 ... 4096" % fn):
                sim.structure_factor(np.zeros((0, 2), np.int32), 4, member=member)
            with pytest.raises(RuntimeError, match="code 2.*%s: nvec" % fn):
                sim.structure_factor(np.zeros((4097, 2), np.int64), 4, kind="velocity", member=member)


def test_half_plane_vectors():
    import particlerobotsimulations_amd as pb
    v = pb.half_plane_vectors(16)
    assert v.shape == (544, 2) and v.dtype == np.int32
    seen = set(map(tuple, v.tolist()))
    assert len(seen) == 544 and (0, 0) not in seen
    assert all((-nx, -ny) not in seen for nx, ny in seen)
    assert all(abs(nx) <= 16 and abs(ny) <= 16 and (ny > 0 or (ny == 0 and nx > 0)) for nx, ny in seen)
    # with the negatives and the origin: the whole square
    assert len(seen | {(-nx, -ny) for nx, ny in seen} | {(0, 0)}) == 33 * 33
    for nmax in (0, 1, 2, 44, 45):
        assert len(pb.half_plane_vectors(nmax)) == 2 * nmax * nmax + 2 * nmax
    assert len(pb.half_plane_vectors(44)) <= 4096 < len(pb.half_plane_vectors(45))  # why the runner refuses M above 44
    assert pb.half_plane_vectors(1).tolist() == [[1, 0], [-1, 1], [0, 1], [1, 1]]
    with pytest.raises(ValueError):
        pb.half_plane_vectors(-1)


def test_structure_factor_values_composes_the_128_bit_sums():
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import _capi
    rows = np.zeros((2, 3), _capi.SK_ROW_DTYPE)
    rows[1, 2] = (3, -4, 5, 0, (1 << 32) - 1, 3, 6, -1, 0, 1 << 27, 7, -(1 << 27))
    rows[0, 1] = (1, 0, 4, 0, 0, 1 << 29, 0, 0, 0, 0, 0, 0)  # re = 2^61 over 4 bots: s = 2^122 / (2^60 * 4)
    v = pb.structure_factor_values(rows)
    assert v["re"].shape == (2, 3) and v["re"][1, 2] == (3 << 32) + (1 << 32) - 1 and v["im"][1, 2] == 6 - (1 << 32)
    assert v["re2"][1, 2] == 1 << 59 and v["im2"][1, 2] == 7 - (1 << 59) and isinstance(v["im2"][1, 2], int)
    assert (v["nx"][1, 2], v["ny"][1, 2], v["measured"][1, 2]) == (3, -4, 5)
    assert v["s"][0, 1] == (1 << 122) / ((1 << 60) * 4) and np.isnan(v["s"][0, 0])
    assert KR.from_device(rows[1])[2] == {"nx": 3, "ny": -4, "measured": 5, "re": (3 << 32) + (1 << 32) - 1,
                                          "im": 6 - (1 << 32), "re2": 1 << 59, "im2": 7 - (1 << 59)}
    # N bots on top of each other: S(k) = N for every k
    rows[0, 0] = (1, 1, 9, 0, 0, (9 << 30) >> 32, 0, 0, 0, 0, 0, 0)
    rows[0, 0]["re_lo"] = (9 << 30) & 0xFFFFFFFF
    assert pb.structure_factor_values(rows)["s"][0, 0] == 9.0


BAD_FLAGS = ([("--sk-kind", v) for v in ("", "charge", "Density", "0")]
             + [("--sk-box-log2", v) for v in ("", "-9", "13", "1.5", "two", "4x")]
             + [("--sk-nmax", v) for v in ("", "0", "45", "-1", "1.5", "many")])


@pytest.mark.parametrize("flag,value", BAD_FLAGS, ids=[f"{f}={v!r}" for f, v in BAD_FLAGS])
def test_runner_refuses_a_bad_sk_value(tmp_path, flag, value):
    for args in ([flag, value], [CFG, "--sk", "s.csv", flag, value, "--quiet"]):
        r = subprocess.run([RUN] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), args
    assert not os.listdir(tmp_path)


def test_runner_sk_flags_need_their_values_and_the_fused_engine(tmp_path):
    for flag in ("--sk", "--sk-kind", "--sk-box-log2", "--sk-nmax"):
        r = subprocess.run([RUN, CFG, flag], capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE), flag
    said = "--sk needs the fused engine (the analysis runs on its resident state)\n"
    for extra in ([], ["--sk-nmax", "44"], ["--sk-kind", "velocity", "--sk-box-log2", "-8"]):
        r = subprocess.run([RUN, CFG, "--engine", "legacy", "--sk", "s.csv"] + extra, capture_output=True, text=True,
                           timeout=60, cwd=tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "", said), extra
    assert not os.listdir(tmp_path)
    source = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_runner.cpp")).read()
    for flag in ("--sk FILE", "--sk-kind density|radius|velocity", "--sk-box-log2 E", "--sk-nmax M"):
        assert flag in source and flag in open(os.path.join(ROOT, "README.md")).read(), flag
        assert flag.split()[0] in open(os.path.join(ROOT, "INTEGRATION.md")).read(), flag


def test_host_engine_has_no_structure_factor(capfd):
    from particlerobotsimulations_amd import _capi, host
    h = host.HostSim(CFG, engine="host")
    capfd.readouterr()
    with pytest.raises(RuntimeError) as caught:
        h.structure_factor([[1, 0], [0, 1]], 4)
    assert str(caught.value).startswith("structure_factor: the structure factor needs the fused engine")
    assert capfd.readouterr() == ("", "Particlebot::structureFactor: the structure factor needs the fused engine\n")
    # the wrapper: NULL vectors or rows are refused before the class is asked; a refused call writes nothing
    L = host.lib()
    vec, row = (C.c_int * 4)(), _capi.pbStructureFactorRow(measured=7)
    assert L.pbHostStructureFactor(h._h, 0, 4, None, 2, C.byref(row)) == -1
    assert L.pbHostStructureFactor(h._h, 0, 4, vec, 2, None) == -1
    assert capfd.readouterr() == ("", "")
    assert L.pbHostStructureFactor(h._h, 0, 4, vec, 2, C.byref(row)) == -1 and row.measured == 7
    capfd.readouterr()
    h.close()
