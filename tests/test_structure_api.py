"""CPU side of the structure analysis (pbSimRadialCounts / pbSimStructureStats / pbSimHexaticOf, csrc/pb_structure.hip).

1. tests/structure_ref.py, the brute-force numpy reference the GPU tests compare against, gives the known answers of
   hand-made cases: lattices whose sixth powers cancel or add up, exact bin edges, and the cluster reference's degrees.
2. The C-ABI entries are declared, exported and reject bad arguments before they touch the device; the runner knows
   --structure and --rdf; the placement-only host engine has no analysis; g(r) from counts is plain arithmetic."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_ref as CR
import structure_ref as SR
from helpers import jittered_blob
from test_contacts_api import state_700

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def cfg_path(name):
    return os.path.join(ROOT, "examples", name)


# ---- 1. the reference ------------------------------------------------------------------------------------------------

def square_lattice():
    """3 x 3 bots of radius 0.125 at pitch 0.25, the contact pitch; bot 4 is the centre."""
    pos = np.array([[0.25 * i, 0.25 * j] for j in range(3) for i in range(3)], f32)
    return pos, np.full(9, 0.125, f32)


def test_square_lattice_centre_cancels_exactly():
    pos, rad = square_lattice()
    tiny = float(np.nextafter(f32(0), f32(1)))  # tangent bots bond under the smallest gap, not under 0
    sre, sim, nb = SR.hexatic_sums(pos, rad, tiny)
    assert nb[4] == 4 and sre[4] == 0 and sim[4] == 0  # u^6 = +1, -1, +1, -1 along the axes
    assert nb.tolist() == [2, 3, 2, 3, 4, 3, 2, 3, 2]
    assert SR.hexatic_sums(pos, rad, 0.0)[2].tolist() == [0] * 9
    stats, psi, _ = SR.analyse(pos, rad, tiny)
    assert stats["bonds"] == 24 and stats["coordination"] == [0, 0, 4, 4, 1, 0, 0, 0] and sum(stats["coordination"]) == 9
    assert psi[4].tolist() == [0.0, 0.0]
    # a gap that also bonds the diagonals (0.3536 - 0.25 = 0.1036)
    sre, sim, nb = SR.hexatic_sums(pos, rad, 0.11)
    assert nb[4] == 8 and nb.tolist() == [3, 5, 3, 5, 8, 5, 3, 5, 3]
    assert SR.stats_of(sre, sim, nb)["coordination"] == [0, 0, 0, 4, 0, 4, 0, 1]


def test_hexagon_centre_has_unit_order():
    ang = np.arange(6) * (np.pi / 3.0) + 0.2
    pos = np.concatenate([[[0.0, 0.0]], 0.25 * np.stack([np.cos(ang), np.sin(ang)], axis=1)]).astype(f32)
    rad = np.full(7, 0.125, f32)
    stats, psi, nb = SR.analyse(pos, rad, 0.001)
    assert nb[0] == 6 and nb[1:].tolist() == [3] * 6
    want = np.exp(6j * 0.2)
    got = complex(psi[0, 0], psi[0, 1])
    # positions rounded to fp32 turn a bond by <= 2^-24 (x 6), and six fp32 operations of <= 2^-24 each follow: < 1e-6
    assert abs(abs(got) - 1.0) < 1e-6 and abs(got - want) < 1e-6
    assert stats["bonds"] == 24 and sum(stats["coordination"]) == 7


def test_sixth_power_against_float64():
    rng = np.random.default_rng(3)
    ang = rng.uniform(0, 2 * np.pi, 1000)
    dist = rng.uniform(0.05, 0.3, 1000).astype(f32)
    rx, ry = (dist * np.cos(ang)).astype(f32), (dist * np.sin(ang)).astype(f32)
    d = np.sqrt(rx * rx + ry * ry)
    qre, qim = SR.bond_terms(rx, ry, d)
    true = np.exp(6j * np.arctan2(ry.astype(np.float64), rx.astype(np.float64)))
    assert qre.dtype == np.int64 and np.abs((qre + 1j * qim) / 2.0 ** 30 - true).max() < 2e-6
    assert SR.q30([0.5, -0.5, 1.5 / 2 ** 30, 2.5 / 2 ** 30, -1.0]).tolist() == [1 << 29, -(1 << 29), 2, 2, -(1 << 30)]


def test_exact_bin_edges_and_even_counts():
    rad = np.full(2, 0.1, f32)
    assert SR.radial_counts([[1.0, 2.0], [1.25, 2.0]], rad, 1.0, 4).tolist() == [0, 2, 0, 0]  # 0.25 is in bin 1
    assert SR.radial_counts([[-3.0, 0.5], [-3.0, 1.5]], rad, 1.0, 4).tolist() == [0, 0, 0, 0]  # 1.0 is not counted
    assert SR.radial_counts([[3.0, -2.0], [3.0, -2.0]], rad, 1.0, 4).tolist() == [2, 0, 0, 0]  # coincident: bin 0
    pos, _, rad = jittered_blob(300, 0.15, np.random.default_rng(7), jitter=0.3)
    for r_max, bins in ((0.6, 64), (3.0, 7), (100.0, 1)):
        c = SR.radial_counts(pos, rad, r_max, bins)
        assert c.dtype == np.uint64 and not (c & np.uint64(1)).any() and c.sum() > 0
    assert SR.radial_counts(pos, rad, 100.0, 1).tolist() == [300 * 299]
    # against float64 distances, away from the edges
    d = np.sqrt(((pos[:, None, :].astype(np.float64) - pos[None, :, :]) ** 2).sum(-1))[~np.eye(300, dtype=bool)]
    frac = d * (64 / 0.6)
    clear = np.abs(frac - np.rint(frac)) > 1e-3
    want = np.bincount(frac[clear & (frac < 64)].astype(np.int64), minlength=64)
    got = SR.radial_counts(pos, rad, 0.6, 64).astype(np.int64)
    assert np.abs(got - want).sum() <= (~clear).sum() and want.sum() > 1000


def test_non_finite_bots_take_part_in_nothing():
    pos = np.array([[0.0, 0.0], [0.1, 0.0], [np.nan, 0.0], [0.05, 0.0], [0.0, np.inf]], f32)
    rad = np.array([0.1, 0.1, 0.1, np.inf, 0.1], f32)
    assert SR.radial_counts(pos, rad, 10.0, 4).tolist() == [2, 0, 0, 0]
    stats, psi, nb = SR.analyse(pos, rad, 0.05)
    assert nb.tolist() == [1, 1, 0, 0, 0] and stats["coordination"][0] == 3 and np.isfinite(psi).all()


def test_neighbours_are_the_cluster_degrees_on_the_700_bot_state():
    pos, _, rad = state_700()
    for gap in (0.0, 0.0019, 0.05):
        stats, psi, nb = SR.analyse(pos, rad, gap)
        deg = CR.analyse(pos, rad, gap)[2]
        assert np.array_equal(nb, deg), gap
        assert stats["bonds"] == int(deg.sum()) and sum(stats["coordination"]) == 700
        assert (np.abs(psi) <= 1.0 + 1e-6).all()
    assert stats["coordination"][7] > 0


# ---- 2. the entry points -----------------------------------------------------------------------------------------------

NAMES = ("pbSimRadialCounts", "pbSimStructureStats", "pbSimHexaticOf", "pbSimGetStructureTimes")


def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi, host
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NAMES:
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbStructureStats) == 56
    assert "pbStructureStats" in header and "2^32 directed bonds" in header
    for name in ("pbHostRadialCounts", "pbHostStructureStats", "pbHostHexatic"):
        assert hasattr(host.lib(), name)


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    counts = np.zeros(8, np.uint64)
    psi = np.zeros(8, np.float64)
    nb = np.zeros(4, np.uint32)
    row = _capi.pbStructureStats()

    def refused(rc, fn, word=None):
        msg = L.pbGetLastErrorString()
        assert rc == PB_ERR_ARG and fn.encode() in msg and (word is None or word.encode() in msg), (rc, msg)

    refused(L.pbSimRadialCounts(None, 1.0, 4, _capi.np_ptr(counts)), "pbSimRadialCounts")
    refused(L.pbSimRadialCounts(fake, 1.0, 4, None), "pbSimRadialCounts")
    for r_max in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
        refused(L.pbSimRadialCounts(fake, r_max, 4, _capi.np_ptr(counts)), "pbSimRadialCounts", "rMax")
    for bins in (0, 4097, 1 << 31):
        refused(L.pbSimRadialCounts(fake, 1.0, bins, _capi.np_ptr(counts)), "pbSimRadialCounts", "bins")
    refused(L.pbSimStructureStats(None, 0.0, C.byref(row)), "pbSimStructureStats")
    refused(L.pbSimStructureStats(fake, 0.0, None), "pbSimStructureStats")
    refused(L.pbSimHexaticOf(None, 0, 0.0, _capi.np_ptr(psi), _capi.np_ptr(nb)), "pbSimHexaticOf")
    refused(L.pbSimHexaticOf(fake, 0, 0.0, None, None), "pbSimHexaticOf")
    for gap in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        refused(L.pbSimStructureStats(fake, gap, C.byref(row)), "pbSimStructureStats", "linkGap")
        refused(L.pbSimHexaticOf(fake, 0, gap, _capi.np_ptr(psi), _capi.np_ptr(nb)), "pbSimHexaticOf", "linkGap")
        refused(L.pbSimHexaticOf(fake, 0, gap, None, _capi.np_ptr(nb)), "pbSimHexaticOf", "linkGap")
    refused(L.pbSimGetStructureTimes(None, None, None), "pbSimGetStructureTimes")
    assert not counts.any() and not psi.any() and not nb.any() and row.bonds == 0


def test_runner_knows_the_structure_flags(tmp_path):
    exe = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    for flag in ("--structure FILE", "--structure-gap G", "--rdf FILE", "--rdf-rmax R", "--rdf-bins B"):
        assert flag in r.stdout + r.stderr, flag
    for flag in ("--structure", "--rdf"):
        r = subprocess.run([exe, cfg_path("example.cfg"), "--engine", "legacy", flag, "c.csv"], capture_output=True,
                           text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and flag + " needs the fused engine" in r.stderr and not os.listdir(tmp_path)
    bad = [("--structure-gap", v) for v in ("-1", "wide", "nan", "inf", "0.1x")]
    bad += [("--rdf-rmax", v) for v in ("0", "-1", "wide", "nan", "inf", "2x")]
    bad += [("--rdf-bins", v) for v in ("0", "4097", "-3", "many", "10.5")]
    for flag, value in bad:
        r = subprocess.run([exe, cfg_path("example.cfg"), "--structure", "s.csv", "--rdf", "r.csv", flag, value],
                           capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "usage" in r.stderr, (flag, value)
        assert not os.listdir(tmp_path)


def test_host_engine_has_no_structure_analysis():
    from particlerobotsimulations_amd import host
    h = host.HostSim(cfg_path("example.cfg"), engine="host")
    with pytest.raises(RuntimeError):
        h.radial_counts(1.0, 10)
    with pytest.raises(RuntimeError):
        h.structure()
    with pytest.raises(RuntimeError):
        h.hexatic(0.0019)


def test_radial_distribution_of_an_ideal_gas_is_one():
    import particlerobotsimulations_amd as pb
    n, box, r_max, bins = 4000, 40.0, 2.0, 10
    pos = np.random.default_rng(5).uniform(0.0, box, (n, 2))
    inner = ((pos > r_max) & (pos < box - r_max)).all(axis=1)  # centres whose whole disc lies inside the box
    counts = np.zeros(bins, np.int64)
    for i in np.flatnonzero(inner):
        d = np.sqrt(((pos - pos[i]) ** 2).sum(axis=1))
        d[i] = np.inf
        counts += np.bincount((d[d < r_max] * (bins / r_max)).astype(np.int64), minlength=bins)
    r, g = pb.radial_distribution(counts, r_max, n / box ** 2, int(inner.sum()))
    assert r.tolist() == pytest.approx([0.1 + 0.2 * b for b in range(bins)])
    # a bin holds ~ N rho pi (r_hi^2 - r_lo^2) >= 900 pairs: Poisson noise below 4 %; five sigma
    assert np.abs(g - 1.0).max() < 0.2
    two = pb.radial_distribution(np.stack([counts, 2 * counts]), r_max, n / box ** 2, int(inner.sum()))[1]
    assert two.shape == (2, bins) and np.array_equal(two[1], 2 * two[0])
