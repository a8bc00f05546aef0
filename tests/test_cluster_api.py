"""CPU side of the cluster analysis (pbSimClusterStats, csrc/pb_cluster.hip).

1. tests/cluster_ref.py, the numpy reference the GPU tests compare against, equals an O(n^2) brute force (the same
   predicate over every pair plus a plain union-find) on jittered blobs, on the five examples' placed states and on
   hand-made cases for the rule itself.
2. The C-ABI entries are declared, exported and reject bad arguments before they touch the device; the runner knows
   --clusters and --cluster-gap; the placement-only host engine has no analysis.
3. The code objects of pb_cluster.hip use no scratch, and the other kernels' registers are what profiles/ records."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_ref as CR
from helpers import jittered_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = ["example.cfg", "example_dead_cells.cfg", "example_gap.cfg", "example_object_transport.cfg",
            "example_obstacle.cfg"]
GAPS = [0.0, 0.0019, 0.05]
f32 = np.float32


def cfg_path(name):
    return os.path.join(ROOT, "examples", name)


def brute(pos, rad, gap):
    """Every pair through the predicate, a plain union-find with the smaller index as the root."""
    pos = np.asarray(pos, f32).reshape(-1, 2)
    rad = np.asarray(rad, f32)
    n = rad.size
    ok = np.isfinite(pos).all(axis=1) & np.isfinite(rad)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    degree = np.zeros(n, np.int64)
    for i in range(n):
        if not ok[i]:
            continue
        hit = CR.linked(pos[i, 0], pos[i, 1], rad[i], pos[:, 0], pos[:, 1], rad, gap) & ok
        hit[i] = False
        degree[i] = int(hit.sum())
        for j in np.flatnonzero(hit[:i]):
            a, b = find(i), find(int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    labels = np.array([find(i) for i in range(n)], np.int64)
    return CR.stats_of(labels, degree), labels.astype(np.uint32), degree.astype(np.uint32)


def assert_same(got, want, what):
    assert got[0] == want[0], (what, got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, "labels")
    assert np.array_equal(got[2], want[2]), (what, "degree")


@pytest.mark.parametrize("n,spacing,seed", [(2, 0.19, 1), (37, 0.2, 2), (500, 0.2, 3), (2000, 0.21, 4),
                                            (1500, 0.24, 5)])
def test_reference_equals_brute_force_on_blobs(n, spacing, seed):
    pos, _, rad = jittered_blob(n, spacing, np.random.default_rng(seed), jitter=0.3)
    some = False
    for gap in GAPS:
        want = brute(pos, rad, gap)
        assert_same(CR.analyse(pos, rad, gap), want, (n, gap))
        some |= CR.nontrivial(want[0], n)
    assert some or n < 10, "every gap gave a trivial answer"


@pytest.mark.parametrize("example", EXAMPLES)
def test_reference_equals_brute_force_on_examples(example):
    from particlerobotsimulations_amd import host
    h = host.HostSim(cfg_path(example), engine="host")
    pos, rad = h.get("pos"), h.get("rad")
    for gap in GAPS:
        assert_same(CR.analyse(pos, rad, gap), brute(pos, rad, gap), (example, gap))


def both(pos, rad, gap):
    got = CR.analyse(pos, rad, gap)
    assert_same(got, brute(pos, rad, gap), gap)
    return got


def test_tangent_pair_is_linked_by_the_smallest_gap_only():
    pos = np.array([[0.0, 0.0], [0.1875, 0.0]], f32)
    rad = np.array([0.09375, 0.09375], f32)
    s, lab, deg = both(pos, rad, 0.0)
    assert s["clusters"] == 2 and s["links"] == 0 and list(lab) == [0, 1]
    s, lab, deg = both(pos, rad, np.nextafter(f32(0), f32(1)))
    assert s["clusters"] == 1 and s["links"] == 1 and list(lab) == [0, 0] and list(deg) == [1, 1]


def test_coincident_bots_are_linked():
    pos = np.array([[3.0, -2.0]] * 3 + [[50.0, 50.0]], f32)
    rad = np.full(4, 0.1, f32)
    s, lab, deg = both(pos, rad, 0.0)
    assert list(lab) == [0, 0, 0, 3] and list(deg) == [2, 2, 2, 0]
    assert s == {"clusters": 2, "largest": 3, "largest_label": 0, "isolated": 1, "links": 3, "max_degree": 2}


def test_non_finite_bot_has_no_links():
    pos = np.array([[0.0, 0.0], [0.1, 0.0], [np.nan, 0.0], [0.05, 0.0], [0.0, np.inf]], f32)
    rad = np.array([0.1, 0.1, 0.1, np.inf, 0.1], f32)
    s, lab, deg = both(pos, rad, 0.05)
    assert list(lab) == [0, 0, 2, 3, 4] and list(deg) == [1, 1, 0, 0, 0]
    assert s["clusters"] == 4 and s["isolated"] == 3


def two_blobs(n0, n1):
    rng = np.random.default_rng(7)
    a, _, ra = jittered_blob(n0, 0.17, rng, center=(-20.0, 0.0), jitter=0.05)
    b, _, rb = jittered_blob(n1, 0.17, rng, center=(20.0, 3.0), jitter=0.05)
    return np.concatenate([a, b]), np.full(n0 + n1, 0.1, f32)  # spacing 0.17 < 0.2: each blob hangs together


def test_two_separated_blobs():
    pos, rad = two_blobs(300, 200)
    s, lab, _ = both(pos, rad, 0.0019)
    assert s["clusters"] == 2 and s["largest"] == 300 and s["largest_label"] == 0
    assert set(lab[:300]) == {0} and set(lab[300:]) == {300}


def test_tie_reports_the_smaller_label():
    pos, rad = two_blobs(150, 150)
    # original indices interleaved, and bot 0 on its own far away: the tie is between labels 1 and 2
    order = np.empty(300, np.int64)
    order[0::2], order[1::2] = np.arange(150), 150 + np.arange(150)
    pos, rad = pos[order], rad[order]
    pos = np.concatenate([np.array([[0.0, 500.0]], f32), pos])
    rad = np.concatenate([np.array([0.1], f32), rad])
    s, lab, _ = both(pos, rad, 0.0019)
    assert s["clusters"] == 3 and s["largest"] == 150 and s["largest_label"] == 1 and s["isolated"] == 1
    assert set(lab[1::2]) == {1} and set(lab[2::2]) == {2}


# ---- 2. the entry points -------------------------------------------------------------------------------------------

def test_symbols_are_declared_and_exported():
    from particlerobotsimulations_amd import _capi
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in ("pbSimClusterStats", "pbSimClusterLabelsOf", "pbSimGetClusterTimes"):
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbClusterStats) == 32
    assert "pbClusterStats" in header and "2^28" in header
    from particlerobotsimulations_amd import host
    for name in ("pbHostClusterStats", "pbHostClusterLabels"):
        assert hasattr(host.lib(), name)
    assert "Cluster" not in open(os.path.join(ROOT, "include", "particlebot_ensemble.h")).read()


def test_bad_arguments_are_rejected_before_the_device_is_touched():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    PB_ERR_ARG = 2
    fake = C.c_void_p(1)  # never dereferenced: these checks come first
    row = _capi.pbClusterStats()
    lab = np.zeros(4, np.uint32)
    assert L.pbSimClusterStats(None, 0.0, C.byref(row)) == PB_ERR_ARG
    assert b"pbSimClusterStats" in L.pbGetLastErrorString()
    assert L.pbSimClusterStats(fake, 0.0, None) == PB_ERR_ARG
    assert b"pbSimClusterStats" in L.pbGetLastErrorString()
    assert L.pbSimClusterLabelsOf(None, 0, 0.0, _capi.np_ptr(lab), None) == PB_ERR_ARG
    assert b"pbSimClusterLabelsOf" in L.pbGetLastErrorString()
    assert L.pbSimClusterLabelsOf(fake, 0, 0.0, None, None) == PB_ERR_ARG
    assert b"pbSimClusterLabelsOf" in L.pbGetLastErrorString()
    for gap in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert L.pbSimClusterStats(fake, gap, C.byref(row)) == PB_ERR_ARG, gap
        assert b"pbSimClusterStats" in L.pbGetLastErrorString() and b"linkGap" in L.pbGetLastErrorString()
        assert L.pbSimClusterLabelsOf(fake, 0, gap, _capi.np_ptr(lab), _capi.np_ptr(lab)) == PB_ERR_ARG, gap
        assert b"pbSimClusterLabelsOf" in L.pbGetLastErrorString()
    assert L.pbSimGetClusterTimes(None, None, None) == PB_ERR_ARG
    assert not lab.any() and row.clusters == 0


def test_runner_knows_the_cluster_flags(tmp_path):
    exe = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert "--clusters FILE" in r.stdout + r.stderr and "--cluster-gap G" in r.stdout + r.stderr
    r = subprocess.run([exe, cfg_path("example.cfg"), "--engine", "legacy", "--clusters", "c.csv"], capture_output=True,
                       text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2 and "--clusters needs the fused engine" in r.stderr and not os.listdir(tmp_path)
    for bad in ("-1", "wide", "nan", "inf", "0.1x"):
        r = subprocess.run([exe, cfg_path("example.cfg"), "--clusters", "c.csv", "--cluster-gap", bad],
                           capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 2 and "usage" in r.stderr, bad
        assert not (tmp_path / "c.csv").exists()


def test_host_engine_has_no_cluster_analysis():
    from particlerobotsimulations_amd import host
    h = host.HostSim(cfg_path("example.cfg"), engine="host")
    with pytest.raises(RuntimeError):
        h.clusters()
    with pytest.raises(RuntimeError):
        h.cluster_labels(0.0019)


# ---- 3. the code objects ---------------------------------------------------------------------------------------------

KERNELS = ["k_cluster_compress", "k_cluster_gather", "k_cluster_hash", "k_cluster_labels", "k_cluster_links",
           "k_cluster_reduce", "k_cluster_rmax", "k_cluster_rows", "k_cluster_sizes", "k_cluster_starts"]


@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    assert r, "no code objects under csrc/build: build the libraries from source (make -C particlerobotsimulations_amd/csrc)"
    return {k: tuple(int(x) if str(x).isdigit() else x for x in v) for k, v in r.items()}


def recorded(name):
    """kernel -> (vgpr, sgpr, lds, scratch) from the `reg` rows of a file under profiles/."""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", name)):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rows[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    return rows


def test_cluster_kernels_have_no_scratch(regs):
    mine = {k: v for k, v in regs.items() if k.startswith("k_cluster_")}
    assert sorted(mine) == KERNELS
    for k, (vgpr, sgpr, lds, scratch) in mine.items():
        assert scratch == 0, (k, vgpr, sgpr, lds, scratch)
    rec = recorded("cluster_analysis.txt")
    for k, v in mine.items():
        assert rec[k] == v, (k, rec[k], v)  # the counts the profile file records are those of this build


def test_other_kernels_registers_are_unchanged(regs):
    """No other kernel's source changed.  profiles/cluster_parent_registers.txt lists every k_force / k_resident /
    k_render kernel of the PARENT commit's code objects with its counts (no tool rewrites it): this build has the same
    keys and values.  The rows profiles/frame_render.txt recorded earlier hold too."""
    pinned = ("k_force", "k_resident", "k_render_")
    rec = recorded("cluster_parent_registers.txt")
    assert len(rec) >= 40 and all(k.startswith(pinned) for k in rec)
    assert {k: v for k, v in regs.items() if k.startswith(pinned)} == rec
    before = recorded("frame_render.txt")
    assert len([k for k in before if k.startswith(("k_force", "k_resident"))]) >= 4
    for k, v in before.items():
        assert regs[k] == v, (k, regs[k], v)
