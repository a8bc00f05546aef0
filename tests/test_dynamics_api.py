"""CPU side of the rearrangement analysis (pbSimMarkReference / pbSimRearrangementStats / pbSimRearrangementOf,
csrc/pb_dynamics.hip).

1. tests/dynamics_ref.py, the reference the GPU tests compare against: it equals an O(n^2) brute force, gives hand-built
   known answers, and reproduces the figures of the GPU tests' recipe.
2. The C-ABI entries are declared, exported and reject bad arguments before they touch the device; the runner knows
   --rearrange and its options; the placement-only host engine has no analysis.
3. mean_squared_displacement on known integers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_ref as CR
import dynamics_ref as DR
from helpers import jittered_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GAPS = [0.0, 0.0019, 0.3]


def cfg_path(name):
    return os.path.join(ROOT, "examples", name)


# ---- 1. the reference --------------------------------------------------------------------------------------------------

def brute_sets(pos, rad, gap):
    pos = np.asarray(pos, f32).reshape(-1, 2)
    rad = np.asarray(rad, f32)
    ok = np.isfinite(pos).all(axis=1) & np.isfinite(rad)
    out = []
    for i in range(rad.size):
        hit = np.zeros(rad.size, bool)
        if ok[i]:
            hit = CR.linked(pos[i, 0], pos[i, 1], rad[i], pos[:, 0], pos[:, 1], rad, gap) & ok
            hit[i] = False
        out.append(set(np.flatnonzero(hit).tolist()))
    return out


def brute(pos0, rad0, pos1, rad1, gap):
    a, b = brute_sets(pos0, rad0, gap), brute_sets(pos1, rad1, gap)
    marked = np.array([len(s) for s in a])
    now = np.array([len(s) for s in b])
    kept = np.array([len(s & t) for s, t in zip(a, b)])
    return marked, now, kept


def test_reference_equals_brute_force():
    rng = np.random.default_rng(2300)
    pos, _, rad = jittered_blob(300, 0.15, rng, jitter=0.3)
    pos1 = DR.perturbed(pos, rng)
    pos1[17] = np.nan  # a bot that is lost on the way
    for gap in GAPS:
        row, bots = DR.analyse(pos, rad, pos1, rad, gap)
        marked, now, kept = brute(pos, rad, pos1, rad, gap)
        assert np.array_equal(bots["marked"], marked) and np.array_equal(bots["now"], now), gap
        assert np.array_equal(bots["kept"], kept), gap
        assert row["bonds_marked"] == marked.sum() and row["bonds_now"] == now.sum() and row["bonds_kept"] == kept.sum()
        assert 0 < row["bonds_kept"] < min(row["bonds_marked"], row["bonds_now"]), gap
        assert bots["now"][17] == 0 and bots["kept"][17] == 0 and row["measured"] == 299
        # the sums against a float64 evaluation of the same fp32 displacements
        d = bots["disp"].astype(np.float64)
        d[17] = 0.0
        q = np.rint(d * 2.0 ** 20)
        assert row["sum_qx"] == int(q[:, 0].sum()) and row["sum_qy"] == int(q[:, 1].sum())
        assert row["sum_q2"] == int((q ** 2).sum()) and row["max_q2"] == int((q ** 2).sum(axis=1).max())


@pytest.mark.parametrize("n, want", [(63, (284, 276, 234, 15)), (257, (1278, 1208, 1018, 32)),
                                     (1025, (5354, 5188, 4306, 147))])
def test_the_gpu_tests_recipe_populates_every_class(n, want):
    rng = np.random.default_rng(2000 + n)
    pos, _, rad = jittered_blob(n, 0.15, rng, jitter=0.3)
    pos1 = DR.perturbed(pos, rng)
    row, bots = DR.analyse(pos, rad, pos1, rad, 0.0019)
    assert (row["bonds_marked"], row["bonds_now"], row["bonds_kept"], row["bots_unchanged"]) == want
    assert 0 < row["bots_lost"] < n and 0 < row["bots_gained"] < n and row["measured"] == n
    if n == 1025:
        assert int(bots["marked"].max()) == 9  # a list longer than 8


def test_chain_in_which_one_bond_breaks_and_one_forms():
    rad = np.full(4, 0.1, f32)
    pos0 = np.array([[0.0, 0.0], [0.19, 0.0], [0.38, 0.0], [0.70, 0.0]], f32)   # 0-1, 1-2; 3 apart
    pos1 = np.array([[-0.2, 0.0], [0.19, 0.0], [0.38, 0.0], [0.57, 0.0]], f32)  # 0 leaves, 3 arrives: 1-2, 2-3
    row, bots = DR.analyse(pos0, rad, pos1, rad, 0.0)
    assert bots["marked"].tolist() == [1, 2, 1, 0] and bots["now"].tolist() == [0, 1, 2, 1]
    assert bots["kept"].tolist() == [0, 1, 1, 0]
    assert (row["bonds_marked"], row["bonds_now"], row["bonds_kept"]) == (4, 4, 2)
    assert (row["bots_unchanged"], row["bots_lost"], row["bots_gained"], row["measured"]) == (0, 2, 2, 4)
    qa, qb = int(np.rint(np.float64(f32(-0.2)) * 2 ** 20)), int(np.rint(np.float64(f32(0.57) - f32(0.70)) * 2 ** 20))
    assert row["sum_qx"] == qa + qb and row["sum_qy"] == 0
    assert row["sum_q2"] == qa * qa + qb * qb and row["max_q2"] == max(qa * qa, qb * qb)
    same, _ = DR.analyse(pos0, rad, pos0, rad, 0.0)
    assert same["bonds_kept"] == same["bonds_marked"] == same["bonds_now"] == 4 and same["bots_unchanged"] == 4
    assert same["sum_q2"] == 0 and same["max_q2"] == 0 and same["measured"] == 4


def test_a_displacement_of_exactly_2048_is_not_measured():
    below = np.nextafter(f32(2048.0), f32(0.0))
    rad = np.full(3, 0.1, f32)
    pos0 = np.zeros((3, 2), f32)
    pos0[:, 1] = [0.0, 10.0, 20.0]
    pos1 = pos0.copy()
    pos1[0, 0] = 2048.0
    pos1[1, 0] = below
    pos1[2, 1] = f32(20.0) - below
    row, bots = DR.analyse(pos0, rad, pos1, rad, 0.0)
    assert bots["disp"][:, 0].tolist() == [2048.0, float(below), 0.0] and row["measured"] == 2
    q = (1 << 31) - 128
    assert int(np.float64(below) * 2 ** 20) == q
    assert row["sum_qx"] == q and row["sum_qy"] == -q and row["sum_q2"] == 2 * q * q and row["max_q2"] == q * q


def test_a_sum_beyond_two_to_the_64():
    n = 8
    rad = np.full(n, 0.1, f32)
    pos0 = np.zeros((n, 2), f32)
    pos0[:, 1] = np.arange(n)
    pos1 = pos0 + np.array([2000.0, -2000.0], f32)
    row, _ = DR.analyse(pos0, rad, pos1, rad, 0.0)
    q = 2000 << 20
    assert row["sum_q2"] == n * 2 * q * q and row["sum_q2"] > 1 << 64 and row["max_q2"] == 2 * q * q < 1 << 63
    assert row["sum_qx"] == n * q and row["sum_qy"] == -n * q


# ---- 2. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimMarkReference", "pbSimClearReference", "pbSimGetReferenceInfo", "pbSimRearrangementStats",
         "pbSimRearrangementOf", "pbSimGetRearrangementTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi, host
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbRearrangementStats) == 80 and "pbRearrangementStats" in header
    for name in ("pbHostMarkReference", "pbHostRearrangementStats", "pbHostRearrangementOf"):
        assert hasattr(host.lib(), name)
    ens = open(os.path.join(ROOT, "include", "particlebot_ensemble.h")).read()
    assert "Rearrangement" not in ens and "MarkReference" not in ens


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    row = _capi.pbRearrangementStats()
    disp = np.zeros(8, f32)
    cnt = np.zeros(4, np.uint32)
    held, gap, t, e = C.c_int(7), C.c_float(7.0), C.c_float(7.0), C.c_ulonglong(7)

    def refused(rc, fn, word=None):
        msg = L.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and fn.encode() in msg and (word is None or word.encode() in msg), (rc, msg)

    refused(L.pbSimMarkReference(None, 0.0), "pbSimMarkReference")
    for g in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        refused(L.pbSimMarkReference(fake, g), "pbSimMarkReference", "linkGap")
    refused(L.pbSimClearReference(None), "pbSimClearReference")
    refused(L.pbSimGetReferenceInfo(None, C.byref(held), C.byref(gap), C.byref(t), C.byref(e)), "pbSimGetReferenceInfo")
    refused(L.pbSimRearrangementStats(None, C.byref(row)), "pbSimRearrangementStats")
    refused(L.pbSimRearrangementStats(fake, None), "pbSimRearrangementStats")
    refused(L.pbSimRearrangementOf(None, 0, _capi.np_ptr(disp), _capi.np_ptr(cnt), None, None), "pbSimRearrangementOf")
    refused(L.pbSimRearrangementOf(fake, 0, None, None, None, None), "pbSimRearrangementOf")
    refused(L.pbSimGetRearrangementTimes(None, None, None), "pbSimGetRearrangementTimes")
    assert held.value == 7 and gap.value == 7.0 and t.value == 7.0 and e.value == 7
    assert not disp.any() and not cnt.any() and row.bonds_marked == 0 and row.max_q2 == 0


def test_runner_knows_the_rearrange_flags(tmp_path):
    exe = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    for flag in ("--rearrange FILE", "--rearrange-gap G", "--rearrange-window"):
        assert flag in r.stdout + r.stderr, flag
    for extra in ([], ["--rearrange-window"], ["--rearrange-gap", "0.0019"]):
        r = subprocess.run([exe, cfg_path("example.cfg"), "--engine", "legacy", "--rearrange", "a.csv"] + extra,
                           capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "--rearrange needs the fused engine" in r.stderr and not os.listdir(tmp_path)
    for bad in ("-1", "wide", "nan", "inf", "0.1x"):
        r = subprocess.run([exe, cfg_path("example.cfg"), "--rearrange", "a.csv", "--rearrange-gap", bad],
                           capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "usage" in r.stderr, bad
        assert not os.listdir(tmp_path)


def test_host_engine_has_no_rearrangement_analysis():
    from particlerobotsimulations_amd import host
    h = host.HostSim(cfg_path("example.cfg"), engine="host")
    with pytest.raises(RuntimeError):
        h.mark_reference(0.0019)
    with pytest.raises(RuntimeError):
        h.rearrangement()
    with pytest.raises(RuntimeError):
        h.rearrangement_of()


# ---- 3. the pure-Python helpers ----------------------------------------------------------------------------------------

def test_mean_squared_displacement_on_known_integers():
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import _capi
    assert "mean_squared_displacement" in pb.__all__
    one = 1 << 20  # a displacement of 1.0
    # four bots moved by (3, 4), (3, 4), (-1, 0), (-1, 0): msd (25 + 25 + 1 + 1) / 4 = 13, drift (1, 2): 13 - 5 = 8
    row = {"measured": 4, "sum_qx": 4 * one, "sum_qy": 8 * one, "sum_q2": 52 * one * one}
    assert pb.mean_squared_displacement(row) == 13.0
    assert pb.mean_squared_displacement(row, subtract_drift=True) == 8.0
    # beyond 2^64 and beyond what a double holds exactly: the fraction is formed from the integers
    q = 2000 * one + 1
    big = {"measured": 3, "sum_qx": 3 * q, "sum_qy": -3 * q, "sum_q2": 6 * q * q}
    assert big["sum_q2"] > 1 << 64
    assert pb.mean_squared_displacement(big) == 2.0 * (q / one) ** 2
    assert pb.mean_squared_displacement(big, subtract_drift=True) == 0.0
    assert np.isnan(pb.mean_squared_displacement({"measured": 0, "sum_qx": 0, "sum_qy": 0, "sum_q2": 0}))
    r = _capi.pbRearrangementStats(bonds_marked=6, bonds_now=4, bonds_kept=2, bots_unchanged=1, bots_lost=2,
                                   bots_gained=1, measured=3, sum_qx=-5, sum_qy=7, sum_q2_lo=9, sum_q2_hi=2, max_q2=11)
    d = _capi.rearrangement_row(r)
    assert d["sum_q2"] == (2 << 64) + 9 and d["sum_qx"] == -5 and d["bonds_kept"] == 2 and "sum_q2_lo" not in d
    assert set(d) == set(DR.FIELDS)
