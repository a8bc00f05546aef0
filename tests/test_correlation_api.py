"""CPU side of the pair correlations (pbSimPairCorrelation, csrc/pb_correlate.hip).

1. tests/correlation_ref.py, the brute-force numpy reference the GPU tests compare against, gives the known answers of
   hand-made cases: exact products, negative sums and their normalised form, the extremes of the fixed point, exact bin
   edges, the identities that tie the bins to the totals, and the radial counts of the structure reference.
2. The C-ABI entries are declared, exported and reject bad arguments before they touch the device; the runner knows
   --correlate; the placement-only host engine has no analysis; C(r) from the integers is plain arithmetic."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import correlation_ref as KR
import structure_ref as SR
from helpers import jittered_blob
from test_contacts_api import state_700

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def cfg_path(name):
    return os.path.join(ROOT, "examples", name)


def two_bots(v0, v1, gap=0.25):
    pos = np.array([[1.0, 2.0], [1.0 + gap, 2.0]], f32)
    return pos, np.array([v0, v1], f32), np.full(2, 0.1, f32)


# ---- 1. the reference ------------------------------------------------------------------------------------------------

def test_two_bots_give_exact_products():
    pos, vel, rad = two_bots((1.0, 0.0), (0.5, 0.0))
    ref = KR.pair_correlation("velocity", pos, vel, rad, 1.0, 4)
    assert ref["pairs"] == [0, 2, 0, 0]  # 0.25 is in bin 1
    assert ref["dot"] == [0, 1 << 40, 0, 0] and KR.normalised(ref["dot"][1]) == (0, 256)
    assert ref["ax"] == [0, 1572864, 0, 0] and ref["ay"] == [0, 0, 0, 0]
    assert ref["totals"] == {"measured": 2, "sum_ax": 1572864, "sum_ay": 0, "sum_a2": (1 << 40) + (1 << 38), "pairs": 2}


def test_negative_sums_are_normalised_with_a_floor_quotient():
    tiny = 2.0 ** -20
    pos, vel, rad = two_bots((tiny, 0.0), (-tiny, 0.0))
    ref = KR.pair_correlation("velocity", pos, vel, rad, 1.0, 4)
    assert ref["dot"][1] == -2 and KR.normalised(-2) == ((1 << 32) - 2, -1)
    assert ref["ax"][1] == 0 and ref["totals"]["sum_a2"] == 2
    for v in (0, 1, -1, (1 << 32) - 1, 1 << 32, -(1 << 32), -(1 << 32) - 1, -(1 << 64), (1 << 94) - 1):
        lo, hi = KR.normalised(v)
        assert 0 <= lo < 1 << 32 and hi * (1 << 32) + lo == v


def test_extreme_velocities_reach_two_to_the_64():
    pos, vel, rad = two_bots((2047.9, 2047.9), (-2047.9, -2047.9))
    a, measured = KR.vector_of("velocity", pos, vel, rad)
    assert measured.all() and a[0, 0] == -a[1, 0] and (1 << 31) - (1 << 18) < a[0, 0] < 1 << 31
    ref = KR.correlate(pos, a, measured, 1.0, 4)
    q = int(a[0, 0])
    assert ref["dot"][1] == -4 * q * q and -(1 << 64) < ref["dot"][1] < -(1 << 64) + (1 << 52)
    lo, hi = KR.normalised(ref["dot"][1])
    assert hi < -(1 << 31) and hi * (1 << 32) + lo == ref["dot"][1]
    assert ref["ax"][1] == 0 and ref["totals"]["sum_a2"] == 4 * q * q
    # 2048 itself, NaN and infinity are not measured
    for bad in (2048.0, -2048.0, np.nan, np.inf):
        pos, vel, rad = two_bots((bad, 0.0), (1.0, 0.0))
        ref = KR.pair_correlation("velocity", pos, vel, rad, 1.0, 4)
        assert ref["pairs"] == [0] * 4 and ref["totals"]["measured"] == 1 and ref["totals"]["sum_ax"] == 1 << 20


def test_exact_bin_edges():
    pos, vel, rad = two_bots((1.0, 0.5), (1.0, 0.5), gap=1.0)  # distance exactly rMax: not counted
    assert KR.pair_correlation("velocity", pos, vel, rad, 1.0, 4)["pairs"] == [0] * 4
    pos, vel, rad = two_bots((1.0, 0.5), (1.0, 0.5), gap=0.0)  # coincident: bin 0
    ref = KR.pair_correlation("velocity", pos, vel, rad, 1.0, 4)
    assert ref["pairs"] == [2, 0, 0, 0] and ref["dot"][0] == 2 * ((1 << 40) + (1 << 38))


def test_radius_and_displacement_vectors():
    pos, vel, rad = jittered_blob(50, 0.15, np.random.default_rng(2), jitter=0.3)
    a, measured = KR.vector_of("radius", pos, vel, rad)
    assert measured.all() and not a[:, 1].any() and np.array_equal(a[:, 0], np.rint(rad.astype(np.float64) * 2 ** 20))
    pos0 = pos - f32(0.125)
    pos0[3] = np.nan
    pos0[4, 1] = pos[4, 1] - f32(3000.0)
    a, measured = KR.vector_of("displacement", pos, vel, rad, pos0)
    assert measured.sum() == 48 and not measured[3] and not measured[4]
    assert (a[measured] == 1 << 17).all() and not a[~measured].any()


def connected_numerator(ref, b):
    t = ref["totals"]
    m = t["measured"]
    return (ref["dot"][b] * m * m - 2 * m * (t["sum_ax"] * ref["ax"][b] + t["sum_ay"] * ref["ay"][b]) +
            (t["sum_ax"] ** 2 + t["sum_ay"] ** 2) * ref["pairs"][b])


def test_rigid_translation_has_no_connected_correlation():
    pos, vel, rad = jittered_blob(120, 0.15, np.random.default_rng(4), jitter=0.3)
    vel[:] = (0.375, -1.25)
    ref = KR.pair_correlation("velocity", pos, vel, rad, 0.6, 16)
    assert sum(ref["pairs"]) > 120 and min(ref["dot"]) >= 0
    for b in range(16):
        assert connected_numerator(ref, b) == 0, b


def test_bins_sum_to_the_totals_when_rmax_covers_the_blob():
    n = 200
    pos, vel, rad = jittered_blob(n, 0.15, np.random.default_rng(9), jitter=0.3)
    ref = KR.pair_correlation("velocity", pos, vel, rad, 100.0, 37)
    t = ref["totals"]
    assert t["measured"] == n and sum(ref["pairs"]) == n * (n - 1) == t["pairs"]
    assert sum(ref["dot"]) == t["sum_ax"] ** 2 + t["sum_ay"] ** 2 - t["sum_a2"]
    assert sum(ref["ax"]) == (n - 1) * t["sum_ax"] and sum(ref["ay"]) == (n - 1) * t["sum_ay"]
    assert min(ref["dot"]) < 0 < max(ref["dot"])


def test_pairs_are_the_radial_counts_on_the_700_bot_state():
    pos, vel, rad = state_700()
    want = SR.radial_counts(pos, rad, 0.6, 64)
    ref = KR.pair_correlation("velocity", pos, vel, rad, 0.6, 64)
    assert ref["totals"]["measured"] == 700 and ref["pairs"] == want.tolist() and want.sum() > 700
    # a bot with a NaN velocity is a node of the radial counts, and in no pair here
    vel = vel.copy()
    vel[350, 1] = np.nan
    ref = KR.pair_correlation("velocity", pos, vel, rad, 0.6, 64)
    assert ref["totals"]["measured"] == 699 and sum(ref["pairs"]) < int(want.sum())
    keep = np.arange(700) != 350
    assert ref["pairs"] == SR.radial_counts(pos[keep], rad[keep], 0.6, 64).tolist()
    assert np.array_equal(SR.radial_counts(pos, rad, 0.6, 64), want)
    # a non-finite position or radius: in nothing, whatever the vector
    rad2 = rad.copy()
    rad2[10] = np.inf
    ref = KR.pair_correlation("radius", pos, vel, rad2, 0.6, 64)
    assert ref["totals"]["measured"] == 699 and ref["pairs"] == SR.radial_counts(pos, rad2, 0.6, 64).tolist()


def test_rows_of_gives_the_library_layout():
    from particlerobotsimulations_amd import _capi, correlation_values
    pos, vel, rad = two_bots((2.0 ** -20, 0.0), (-(2.0 ** -20), 0.0))
    ref = KR.pair_correlation("velocity", pos, vel, rad, 1.0, 4)
    rows = KR.rows_of(ref, _capi.CORRELATION_BIN_DTYPE)
    assert rows["dot_lo"].tolist() == [0, (1 << 32) - 2, 0, 0] and rows["dot_hi"].tolist() == [0, -1, 0, 0]
    back = correlation_values(rows)
    assert all(back[k] == ref[k] for k in ("pairs", "dot", "ax", "ay"))


# ---- 2. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimPairCorrelation", "pbSimGetCorrelationTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi, host
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbCorrelationBin) == 56 and C.sizeof(_capi.pbCorrelationTotals) == 48
    assert _capi.CORRELATION_BIN_DTYPE.itemsize == 56
    assert "PB_CORR_MAX_BINS 1024u" in header and "2^31 ordered pairs" in header
    assert hasattr(host.lib(), "pbHostPairCorrelation")


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    rows = np.zeros(8, _capi.CORRELATION_BIN_DTYPE)
    tot = _capi.pbCorrelationTotals()

    def refused(rc, word=None):
        msg = L.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and b"pbSimPairCorrelation" in msg and (word is None or word.encode() in msg), (rc, msg)

    refused(L.pbSimPairCorrelation(None, 0, 1.0, 4, _capi.np_ptr(rows), C.byref(tot)), "null")
    refused(L.pbSimPairCorrelation(fake, 0, 1.0, 4, None, C.byref(tot)), "null")
    for kind in (-1, 3, 1 << 20):
        refused(L.pbSimPairCorrelation(fake, kind, 1.0, 4, _capi.np_ptr(rows), None), "kind")
    for r_max in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        for kind in (0, 1, 2):
            refused(L.pbSimPairCorrelation(fake, kind, r_max, 4, _capi.np_ptr(rows), None), "rMax")
    for bins in (0, 1025, 4096, 1 << 31):
        refused(L.pbSimPairCorrelation(fake, 2, 1.0, bins, _capi.np_ptr(rows), C.byref(tot)), "bins")
    assert L.pbSimGetCorrelationTimes(None, None, None) == PB_ERR_ARG
    assert b"pbSimGetCorrelationTimes" in L.pbGetLastErrorString()
    assert not rows.view(np.uint8).any() and tot.measured == 0 and tot.pairs == 0


def test_kind_names():
    from particlerobotsimulations_amd import _capi
    assert [_capi.correlation_kind(k) for k in ("velocity", "displacement", "radius", 2, 0)] == [0, 1, 2, 2, 0]
    with pytest.raises(ValueError):
        _capi.correlation_kind("phase")


def test_runner_knows_the_correlate_flags(tmp_path):
    exe = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
    good = ["--correlate", "k.csv", "--correlate-kind", "radius", "--correlate-rmax", "1.5", "--correlate-bins", "1024"]
    r = subprocess.run([exe, cfg_path("example.cfg"), "--engine", "legacy"] + good, capture_output=True, text=True,
                       timeout=60, cwd=tmp_path)  # every flag is parsed before the engine is looked at
    assert r.returncode == 2 and not os.listdir(tmp_path)
    assert r.stderr == "--correlate needs the fused engine (the analysis runs on its resident state)\n"
    r = subprocess.run([exe, cfg_path("example.cfg"), "--engine", "legacy", "--series", "s.csv", "--correlate", "k.csv"],
                       capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and r.stderr.startswith("--series needs the fused engine")  # --correlate comes last
    bad = [("--correlate-kind", v) for v in ("displacement", "phase", "0", "Velocity")]
    bad += [("--correlate-rmax", v) for v in ("0", "-1", "wide", "nan", "inf", "2x")]
    bad += [("--correlate-bins", v) for v in ("0", "1025", "-3", "many", "10.5")]
    for flag, value in bad:
        r = subprocess.run([exe, cfg_path("example.cfg"), "--correlate", "k.csv", flag, value], capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and r.stderr.startswith("usage: "), (flag, value)
        assert "--correlate" not in r.stderr  # the usage line is the one printed before
        assert not os.listdir(tmp_path)
    src = open(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "pb_runner.cpp")).read()
    head = src[:src.index("#include")]
    for flag in ("--correlate FILE", "--correlate-kind velocity|radius", "--correlate-rmax R", "--correlate-bins B"):
        assert flag in head, flag


def test_host_engine_has_no_correlation_analysis(capfd):
    from particlerobotsimulations_amd import _capi, host
    h = host.HostSim(cfg_path("example.cfg"), engine="host")
    capfd.readouterr()
    with pytest.raises(RuntimeError) as caught:
        h.pair_correlation("velocity", 1.0, 8)
    assert str(caught.value) == ("pair_correlation: the correlation analysis needs the fused engine, a known kind, a "
                                 "finite r_max > 0 and 1 ... 1024 bins")
    assert capfd.readouterr() == ("", "Particlebot::pairCorrelation: the correlation analysis needs the fused engine\n")
    rows = np.full(8 * 56, 0xAB, np.uint8)
    tot = np.full(48, 0xAB, np.uint8)
    L = host.lib()
    assert L.pbHostPairCorrelation(h._h, 0, 1.0, 8, None, _capi.np_ptr(tot)) == -1
    assert capfd.readouterr() == ("", "")  # NULL rows: refused before the class is asked
    assert L.pbHostPairCorrelation(h._h, 0, 1.0, 8, _capi.np_ptr(rows), _capi.np_ptr(tot)) == -1
    assert (rows == 0xAB).all() and (tot == 0xAB).all()
    with pytest.raises(ValueError):
        h.pair_correlation("phase", 1.0, 8)
    h.close()


def test_connected_correlation_from_the_integers():
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import _capi
    n = 150
    pos, vel, rad = jittered_blob(n, 0.15, np.random.default_rng(12), jitter=0.3)
    vel = vel + f32(0.5)  # a common drift, which the connected form takes out
    ref = KR.pair_correlation("velocity", pos, vel, rad, 0.6, 12)
    rows = KR.rows_of(ref, _capi.CORRELATION_BIN_DTYPE)
    c, ratio = pb.connected_correlation(rows, ref["totals"])
    # against float64 on the fixed-point vectors themselves
    a, measured = KR.vector_of("velocity", pos, vel, rad)
    w = a.astype(np.float64) / 2.0 ** 20
    w -= w.mean(axis=0)
    c0 = (w * w).sum() / n
    with np.errstate(all="ignore"):
        scale = f32(12) / f32(0.6)
        for b in range(12):
            tot, cnt = 0.0, 0
            for i in range(n):
                d = np.sqrt(((pos - pos[i]) ** 2).sum(axis=1).astype(f32))
                hit = ((d * scale).astype(f32) < 12) & ((d * scale).astype(np.int64) == b)
                hit[i] = False
                tot += float((w[hit] @ w[i]).sum())
                cnt += int(hit.sum())
            if cnt == 0:
                assert np.isnan(c[b]) and np.isnan(ratio[b])
            else:  # float64 sums of at most 22 350 terms of magnitude < 1: far inside 1e-9
                assert cnt == ref["pairs"][b]
                assert c[b] == pytest.approx(tot / cnt, rel=1e-9, abs=1e-12), b
                assert ratio[b] == pytest.approx(tot / cnt / c0, rel=1e-9, abs=1e-9), b
    assert np.isfinite(c).sum() >= 8
    empty = np.zeros(3, _capi.CORRELATION_BIN_DTYPE)
    c, ratio = pb.connected_correlation(empty, {"measured": 0, "sum_ax": 0, "sum_ay": 0, "sum_a2": 0, "pairs": 0})
    assert np.isnan(c).all() and np.isnan(ratio).all()
    with pytest.raises(ValueError):
        pb.correlation_values(np.zeros((2, 3), _capi.CORRELATION_BIN_DTYPE))
