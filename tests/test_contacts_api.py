"""CPU side of the contact export (pbSimContactsOf / pbSimContactVirialOf, csrc/pb_contacts.hip).

1. tests/contacts_ref.py, the reference the GPU tests compare against: its topology equals an O(n^2) brute force, its
   forces are exactly antisymmetric and its gaps bit-equal in the two directions, and the state the GPU tests use holds
   entries of all four regimes of the pair law.
2. The C-ABI entries are declared, exported and reject bad arguments before they touch the device; the runner knows
   --contacts and --contact-gap; the placement-only host engine has no export.
3. The code objects of pb_contacts.hip use no scratch and are what profiles/contact_network.txt records."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_ref as CR
import contacts_ref as KR
from helpers import assert_bit_equal, jittered_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAPS = [0.0, 0.0019, 0.05]
f32 = np.float32


def cfg_path(name):
    return os.path.join(ROOT, "examples", name)


def state_700():
    """The state the one-member GPU test uses."""
    return jittered_blob(700, 0.2, np.random.default_rng(100), jitter=0.3)


# ---- 1. the reference --------------------------------------------------------------------------------------------------

def brute_topology(pos, rad, gap):
    pos = np.asarray(pos, f32).reshape(-1, 2)
    rad = np.asarray(rad, f32)
    n = rad.size
    ok = np.isfinite(pos).all(axis=1) & np.isfinite(rad)
    offsets, other = [0], []
    for i in range(n):
        if ok[i]:
            hit = CR.linked(pos[i, 0], pos[i, 1], rad[i], pos[:, 0], pos[:, 1], rad, gap) & ok
            hit[i] = False
            other += np.flatnonzero(hit).tolist()  # ascending
        offsets.append(len(other))
    return np.array(offsets, np.uint32), np.array(other, np.int64)


def test_reference_topology_equals_brute_force():
    pos, _, rad = jittered_blob(300, 0.2, np.random.default_rng(7), jitter=0.3)
    for gap in GAPS:
        offsets, owner, other = KR.topology(pos, rad, gap)
        want_off, want_other = brute_topology(pos, rad, gap)
        assert np.array_equal(offsets, want_off), gap
        assert np.array_equal(other, want_other), gap
        assert np.array_equal(owner, np.repeat(np.arange(300), np.diff(want_off.astype(np.int64)))), gap
        assert np.array_equal(np.diff(offsets.astype(np.int64)), CR.analyse(pos, rad, gap)[2]), gap
        assert other.size > 0


def reverse_of(net):
    """Index of the entry (other -> owner) for every entry (owner -> other)."""
    off = net["offsets"].astype(np.int64)
    owner = np.repeat(np.arange(off.size - 1), np.diff(off))
    where = {(int(a), int(b)): e for e, (a, b) in enumerate(zip(owner, net["other"]))}
    return np.array([where[(int(b), int(a))] for a, b in zip(owner, net["other"])], np.int64)


def test_reference_forces_are_antisymmetric_and_gaps_symmetric(orc):
    pos, vel, rad = jittered_blob(300, 0.2, np.random.default_rng(7), jitter=0.3)
    P = orc.default_params(nCells=300, nDead=0, seed=1)
    for gap in GAPS:
        net = KR.network(orc, P, pos, vel, rad, gap)
        back = reverse_of(net)
        assert_bit_equal(net["gap"], net["gap"][back], "gap in the two directions")
        f, g = net["force"], net["force"][back]
        assert np.isfinite(f).all()
        assert (f == -g).all(), gap


def regimes(gap):
    gap = np.asarray(gap, f32)
    return {"contact": int((gap < 0).sum()), "band": int(((gap >= 0) & (gap < f32(0.0009))).sum()),
            "linear": int(((gap >= f32(0.0009)) & (gap < f32(0.0019))).sum()), "far": int((gap >= f32(0.0019)).sum())}


def test_the_gpu_tests_state_holds_all_four_regimes(orc):
    pos, vel, rad = state_700()
    _, owner, other = KR.topology(pos, rad, 0.05)
    g, _, _ = KR.gaps_of(pos, rad, owner, other)
    undirected = regimes(g[owner < other])
    print(undirected)
    for k, v in undirected.items():
        assert v > 0, (k, undirected)
    assert undirected == {"contact": 819, "band": 17, "linear": 16, "far": 707}


# ---- 2. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimContactsOf", "pbSimContactVirialOf", "pbSimGetContactTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi, host
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbContactLink) == 16 and _capi.CONTACT_LINK_DTYPE.itemsize == 16
    assert "pbContactLink" in header
    for name in ("pbHostContacts", "pbHostContactVirial"):
        assert hasattr(host.lib(), name)


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    count = C.c_ulonglong(77)
    vir = np.zeros(16, np.float64)
    off = np.zeros(5, np.uint32)
    assert L.pbSimContactsOf(None, 0, 0.0, _capi.np_ptr(off), None, 0, C.byref(count)) == PB_ERR_ARG
    assert b"pbSimContactsOf" in L.pbGetLastErrorString()
    assert L.pbSimContactsOf(fake, 0, 0.0, _capi.np_ptr(off), None, 0, None) == PB_ERR_ARG
    assert b"pbSimContactsOf" in L.pbGetLastErrorString()
    assert L.pbSimContactVirialOf(None, 0, 0.0, _capi.np_ptr(vir)) == PB_ERR_ARG
    assert b"pbSimContactVirialOf" in L.pbGetLastErrorString()
    assert L.pbSimContactVirialOf(fake, 0, 0.0, None) == PB_ERR_ARG
    assert b"pbSimContactVirialOf" in L.pbGetLastErrorString()
    for gap in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert L.pbSimContactsOf(fake, 0, gap, _capi.np_ptr(off), None, 0, C.byref(count)) == PB_ERR_ARG, gap
        assert b"pbSimContactsOf" in L.pbGetLastErrorString() and b"linkGap" in L.pbGetLastErrorString()
        assert L.pbSimContactVirialOf(fake, 0, gap, _capi.np_ptr(vir)) == PB_ERR_ARG, gap
        assert b"pbSimContactVirialOf" in L.pbGetLastErrorString() and b"linkGap" in L.pbGetLastErrorString()
    assert L.pbSimGetContactTimes(None, None, None) == PB_ERR_ARG
    assert b"pbSimGetContactTimes" in L.pbGetLastErrorString()
    assert not vir.any() and not off.any() and count.value == 77


def test_runner_knows_the_contact_flags(tmp_path):
    exe = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert "--contacts FILE" in r.stdout + r.stderr and "--contact-gap G" in r.stdout + r.stderr
    r = subprocess.run([exe, cfg_path("example.cfg"), "--engine", "legacy", "--contacts", "c.csv"], capture_output=True,
                       text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and "--contacts needs the fused engine" in r.stderr and not os.listdir(tmp_path)
    for bad in ("-1", "wide", "nan", "inf", "0.1x"):
        r = subprocess.run([exe, cfg_path("example.cfg"), "--contacts", "c.csv", "--contact-gap", bad],
                           capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "usage" in r.stderr, bad
        assert not os.listdir(tmp_path)


def test_host_engine_has_no_contact_export():
    from particlerobotsimulations_amd import host
    h = host.HostSim(cfg_path("example.cfg"), engine="host")
    with pytest.raises(RuntimeError):
        h.contacts()
    with pytest.raises(RuntimeError):
        h.contact_virial(0.0019)


# ---- 3. the code objects -----------------------------------------------------------------------------------------------

KERNELS = ["k_contact_fill", "k_contact_gather_vel", "k_contact_order", "k_contact_scan"]


def test_contact_kernels_have_no_scratch_and_match_the_profile():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    assert regs, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    mine = {k: tuple(int(x) for x in v) for k, v in regs.items() if k.startswith("k_contact_")}
    assert sorted(mine) == KERNELS
    for k, (vgpr, sgpr, lds, scratch) in mine.items():
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
    rec = {}
    for line in open(os.path.join(ROOT, "profiles", "contact_network.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rec[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    assert rec == mine  # the counts the profile file records are those of this build
