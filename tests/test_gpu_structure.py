"""GPU: the structure analysis (pbSimRadialCounts / pbSimStructureStats / pbSimHexaticOf, csrc/pb_structure.hip) against
tests/structure_ref.py on the state read back from the device.  Every comparison is exact: counts, sums, neighbour
counts and coordination are integers, psi6 is compared as bit patterns.  tests/test_structure_api.py pins the reference
to known answers on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import cluster_ref as CR
import structure_ref as SR
from helpers import assert_bit_equal, jittered_blob, simparams_from_orc
from test_contacts_api import state_700

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
f32 = np.float32
GAP = 0.0019
RDF = [(0.6, 64), (3.0, 7)]  # (rMax, bins); 3.0 covers a whole small blob on a folding grid


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def sim_with(pb, orc, pos, rad, vel=None, wall_half=4.0e6, **over):
    pos = np.asarray(pos, f32).reshape(-1, 2)
    n = pos.shape[0]
    over.setdefault("nDead", 0)
    P = orc.default_params(nCells=n, seed=3, max_time=1e9, **over)
    sp, keep = simparams_from_orc(P)
    sim = pb.Sim(sp, wall_half=wall_half, keepalive=keep)
    sim.set_state(pos=pos, vel=np.zeros((n, 2), f32) if vel is None else vel, rad=np.asarray(rad, f32),
                  phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    return sim


def strip(row):
    return {k: row[k] for k in ("bonds", "psi6_re", "psi6_im", "coordination")}


def psi_bits(psi):
    """complex128[n] or float64 (n, 2) as uint64 (n, 2)."""
    return np.ascontiguousarray(psi).view(np.float64).reshape(-1, 2).view(np.uint64)


def check_hexatic(sim, member, gap, pos, rad, what, row=None):
    """Row, psi6 and neighbour counts of one member against the reference on (pos, rad); returns the reference."""
    want, wpsi, wnb = SR.analyse(pos, rad, gap)
    if row is None:
        row = sim.structure(gap)[member]
    print(what, "gap", gap, row)
    assert strip(row) == want, (what, gap, row, want)
    assert sum(row["coordination"]) == len(wnb)
    psi, nb = sim.hexatic(gap, member=member)
    assert psi.dtype == np.complex128 and nb.dtype == np.uint32
    assert np.array_equal(nb, wnb), (what, gap, "neighbours")
    assert np.array_equal(psi_bits(psi), psi_bits(wpsi)), (what, gap, "psi6 bit patterns")
    return want, wpsi, wnb


def check_radial(sim, member, r_max, bins, pos, rad, what, counts=None):
    want = SR.radial_counts(pos, rad, r_max, bins)
    if counts is None:
        counts = sim.radial_counts(r_max, bins)
    got = counts[member]
    print(what, "rMax", r_max, "bins", bins, "pairs", int(got.sum()))
    assert got.dtype == np.uint64 and got.shape == (bins,)
    assert np.array_equal(got, want), (what, r_max, bins, np.flatnonzero(got != want)[:8])
    assert not (got & np.uint64(1)).any()
    return want


# ---- sizes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_around_the_wave_and_the_workgroup(pb, orc, n):
    pos, vel, rad = jittered_blob(n, 0.15, np.random.default_rng(1000 + n), jitter=0.3)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    want, _, wnb = check_hexatic(sim, 0, GAP, pos, rad, f"n {n}")
    for r_max, bins in RDF:
        got = check_radial(sim, 0, r_max, bins, pos, rad, f"n {n}")
        if n >= 63:
            assert got.sum() > 0
        if r_max == 3.0 and n <= 65:  # the blob is smaller than rMax: every ordered pair is counted, once
            assert int(got.sum()) == n * (n - 1)
    if n >= 63:
        assert want["bonds"] > n and (want["psi6_re"] or want["psi6_im"]), "a trivial case"
        assert np.array_equal(wnb, CR.analyse(pos, rad, GAP)[2])


# ---- bin limits ----------------------------------------------------------------------------------------------------------

def test_bin_limits_on_one_blob(pb, orc):
    n = 300
    pos, vel, rad = jittered_blob(n, 0.15, np.random.default_rng(7), jitter=0.3)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    for bins in (1, 4096):
        for r_max in (0.05, 100.0):
            got = check_radial(sim, 0, r_max, bins, pos, rad, "limits")
            if r_max == 100.0:
                assert int(got.sum()) == n * (n - 1)
            else:
                assert int(got.sum()) < n  # almost nothing is closer than 0.05
    assert sim.radial_counts(100.0, 1).tolist() == [[n * (n - 1)]]


# ---- edges and edge cases ------------------------------------------------------------------------------------------------

def test_exact_bin_edges(pb, orc):
    rad = np.full(2, 0.1, f32)
    pos = np.array([[1.0, 2.0], [1.25, 2.0]], f32)  # distance exactly 0.25
    sim = sim_with(pb, orc, pos, rad)
    assert check_radial(sim, 0, 1.0, 4, pos, rad, "edge 0.25").tolist() == [0, 2, 0, 0]
    pos = np.array([[-3.0, 0.5], [-3.0, 1.5]], f32)  # distance exactly 1.0 = rMax: not counted
    sim = sim_with(pb, orc, pos, rad)
    assert check_radial(sim, 0, 1.0, 4, pos, rad, "edge 1.0").tolist() == [0, 0, 0, 0]


def test_coincident_non_finite_and_tangent_bots(pb, orc):
    pos, rad = np.array([[3.0, -2.0]] * 2 + [[50.0, 50.0]], f32), np.full(3, 0.1, f32)
    sim = sim_with(pb, orc, pos, rad)
    assert check_radial(sim, 0, 1.0, 8, pos, rad, "coincident").tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    want, wpsi, wnb = check_hexatic(sim, 0, 0.0, pos, rad, "coincident")
    assert wnb.tolist() == [1, 1, 0] and want["bonds"] == 2 and want["psi6_re"] == 0 and want["psi6_im"] == 0
    psi, _ = sim.hexatic(0.0)
    assert np.isfinite(psi.view(np.float64)).all() and not psi.any()

    pos = np.array([[0.0, 0.0], [np.nan, 0.0], [0.05, 0.0], [0.0, np.inf]], f32)  # one finite bot among non-finite ones
    rad = np.array([0.1, 0.1, np.inf, 0.1], f32)
    sim = sim_with(pb, orc, pos, rad)
    assert not check_radial(sim, 0, 10.0, 16, pos, rad, "non-finite").any()
    want, _, _ = check_hexatic(sim, 0, 0.05, pos, rad, "non-finite")
    assert want["bonds"] == 0 and want["coordination"] == [4, 0, 0, 0, 0, 0, 0, 0]
    # the set of test_gpu_contacts.test_coincident_non_finite_and_tangent_bots: its two finite bots are one pair
    pos = np.array([[0.0, 0.0], [0.1, 0.0], [np.nan, 0.0], [0.05, 0.0], [0.0, np.inf]], f32)
    rad = np.array([0.1, 0.1, 0.1, np.inf, 0.1], f32)
    sim = sim_with(pb, orc, pos, rad)
    assert int(check_radial(sim, 0, 10.0, 16, pos, rad, "non-finite set").sum()) == 2
    want, _, wnb = check_hexatic(sim, 0, 0.05, pos, rad, "non-finite set")
    assert wnb.tolist() == [1, 1, 0, 0, 0] and want["bonds"] == 2

    pos, rad = np.array([[0.0, 0.0], [0.1875, 0.0]], f32), np.array([0.09375, 0.09375], f32)
    sim = sim_with(pb, orc, pos, rad)
    assert check_hexatic(sim, 0, 0.0, pos, rad, "tangent")[0]["bonds"] == 0
    want, wpsi, _ = check_hexatic(sim, 0, 1e-6, pos, rad, "tangent")
    assert want["bonds"] == 2 and want["psi6_re"] == 2 << 30 and want["psi6_im"] == 0 and wpsi.tolist() == [[1, 0]] * 2


# ---- a batch -------------------------------------------------------------------------------------------------------------

def test_batch_of_five_members_stepped_out_of_original_order(pb, orc):
    members, n = 5, 300
    rng = np.random.default_rng(50)
    plist, keeps = [], []
    for k in range(members):
        P = orc.default_params(nCells=n, nDead=0, seed=50 + k, max_time=1e9, phase_update_interval=0.3,
                               light_x=-2.0 + k, light_y=4.0 - 0.5 * k, attraction=4.7652e-05 * (1.0 + 0.1 * k),
                               phase_std=0.1 * k)
        sp, keep = simparams_from_orc(P)
        plist.append(sp)
        keeps.append(keep)
    ens = pb.Ensemble(plist, keepalive=keeps)
    for k in range(members):
        pos, vel, rad = jittered_blob(n, 0.2, rng, center=(0.3 * k, -0.2 * k), jitter=0.3)
        ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=rng.uniform(0, 6.28, n).astype(f32),
                         dead=(rng.random(n) < 0.05 * k).astype(np.int32))
    assert ens.step(120, dt=0.01, sort_interval=0.5) == 120  # slots leave original order, the cell lists are stale
    assert ens.stats()["resorts"] >= 2
    st3 = ens.get_state_of(3)
    ens.set_state_of(4, pos=st3["pos"], vel=st3["vel"], rad=st3["rad"], phase=st3["phase"], dead=st3["dead"])
    rows = ens.structure(GAP)
    assert len(rows) == members
    counts = {rb: ens.radial_counts(*rb) for rb in RDF}
    for k in range(members):
        st = ens.get_state_of(k)
        want, wpsi, wnb = check_hexatic(ens, k, GAP, st["pos"], st["rad"], f"member {k}", rows[k])
        assert want["bonds"] > n and want["coordination"][0] > 0 and want["coordination"][4] > 0, "a trivial member"
        for rb in RDF:
            assert counts[rb].shape == (members, rb[1])
            check_radial(ens, k, rb[0], rb[1], st["pos"], st["rad"], f"member {k}", counts[rb])
            assert np.array_equal(ens.radial_counts(rb[0], rb[1], member=k), counts[rb][k])
        # the row against the cluster analysis' degrees and against the per-bot values
        deg = ens.cluster_labels(GAP, member=k)[1].astype(np.int64)
        assert rows[k]["bonds"] == int(deg.sum())
        assert rows[k]["coordination"] == np.bincount(np.minimum(deg, 7), minlength=8).tolist()
        psi, nb = ens.hexatic(GAP, member=k)
        assert np.array_equal(nb, deg)
        sums = np.rint(psi.view(np.float64).reshape(-1, 2) * nb[:, None].astype(np.float64) * 1073741824.0)
        assert rows[k]["psi6_re"] == int(sums[:, 0].astype(np.int64).sum())
        assert rows[k]["psi6_im"] == int(sums[:, 1].astype(np.int64).sum())
        assert rows[k]["psi6"] == complex(rows[k]["psi6_re"] / 2.0 ** 30, rows[k]["psi6_im"] / 2.0 ** 30) / rows[k]["bonds"]
    assert strip(rows[3]) == strip(rows[4])
    a, b = ens.hexatic(GAP, member=3), ens.hexatic(GAP, member=4)
    assert np.array_equal(psi_bits(a[0]), psi_bits(b[0])) and np.array_equal(a[1], b[1])
    for rb in RDF:
        assert np.array_equal(counts[rb][3], counts[rb][4])


def test_payload_bot_is_an_ordinary_node(pb, orc):
    n = 201
    pos, vel, rad = jittered_blob(n, 0.2, np.random.default_rng(21), jitter=0.3)
    pos[n - 1] = pos[100] + np.array([0.1, 0.05], f32)  # the payload in the middle of the blob, twice as large
    rad[n - 1] = 0.2
    sim = sim_with(pb, orc, pos, rad, vel=vel, wall_half=64.0, nDead=-1, radFactor=2.0, attractionFactor=0.5)
    assert sim.config()["payload"] == 1
    _, _, wnb = check_hexatic(sim, 0, GAP, pos, rad, "payload")
    assert wnb[n - 1] >= 3
    for r_max, bins in RDF:
        check_radial(sim, 0, r_max, bins, pos, rad, "payload")


# ---- nothing changes, repeatability -----------------------------------------------------------------------------------------

def test_nothing_changes_and_the_shared_scratch_stays_valid(pb, orc):
    import contacts_ref as KR
    pos, vel, rad = state_700()
    n = rad.size
    P = orc.default_params(nCells=n, nDead=0, seed=3, max_time=1e9)
    sp, keep = simparams_from_orc(P)
    sim = pb.Sim(sp, wall_half=64.0, keepalive=keep)
    sim.set_state(pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    assert sim.step(30, dt=0.01, sort_interval=0.1) == 30
    before, stats = sim.get_state(), sim.stats()
    assert sim.structure_times() == (0, 0.0)
    first = (sim.radial_counts(0.6, 64), sim.structure(GAP), sim.hexatic(GAP))
    t = sim.structure_times()
    assert t[0] == 3 and t[1] > 0.0
    check_hexatic(sim, 0, GAP, before["pos"], before["rad"], "700 bots")
    check_radial(sim, 0, 0.6, 64, before["pos"], before["rad"], "700 bots")
    assert sim.structure_times()[0] == 6
    # a cluster analysis and a contact export after the structure calls (the scratch is shared), and the other way round
    for gap in (0.0, GAP):
        sim.radial_counts(3.0, 7)
        want, wlab, wdeg = CR.analyse(before["pos"], before["rad"], gap)
        assert {k: sim.clusters(gap)[0][k] for k in CR.FIELDS} == want
        lab, deg = sim.cluster_labels(gap)
        assert np.array_equal(lab, wlab) and np.array_equal(deg, wdeg)
        sim.radial_counts(0.05, 4096)
        net = KR.network(orc, P, before["pos"], before["vel"], before["rad"], gap)
        got = sim.contacts(gap)
        assert np.array_equal(got["offsets"], net["offsets"]) and np.array_equal(got["other"], net["other"])
        assert_bit_equal(got["gap"], net["gap"], "gap")
    # repeatability: the same arrays again, after everything above
    again = (sim.radial_counts(0.6, 64), sim.structure(GAP), sim.hexatic(GAP))
    assert np.array_equal(first[0], again[0]) and first[1] == again[1]
    assert np.array_equal(psi_bits(first[2][0]), psi_bits(again[2][0])) and np.array_equal(first[2][1], again[2][1])
    after = sim.get_state()
    for name in before:
        assert_bit_equal(after[name], before[name], name)
    assert sim.stats() == stats


# ---- the runner ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [{}, {"dump_interval": "1"}])
def test_runner_writes_structure_rows_and_the_final_histogram(tmp_path, extra):
    from particlerobotsimulations_amd import host
    cfg = os.path.join(ROOT, "examples", "example.cfg")
    over = dict(max_time="3", **extra)
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    r = subprocess.run([RUN, cfg, "--quiet"] + sets + ["--structure", "s.csv", "--rdf", "r.csv"], capture_output=True,
                       text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "s.csv").read().splitlines()
    assert lines[0] == "Time, Bonds, Psi6Re, Psi6Im, C0, C1, C2, C3, C4, C5, C6, C7"
    main_times = [l.split(",")[0] for l in open(tmp_path / "example_data.csv").read().splitlines()[2:]]
    assert [l.split(",")[0] for l in lines[1:]] == main_times and len(main_times) >= (4 if extra else 1)
    flat = host.load_config(cfg, **over)
    h = host.HostSim(cfg, engine="fused", **over)
    di = f32(flat.dump_interval)
    want = []

    def due(t):  # the gate of dumpParticlebot, in its fp32 operations
        t = f32(t)
        return not (t - di * np.floor(t / di) > f32(0.01))

    while True:
        if due(h.time):
            s = h.structure(0.0)[0]
            want.append("%f, %d, %d, %d, " % (h.time, s["bonds"], s["psi6_re"], s["psi6_im"]) +
                        ", ".join(str(c) for c in s["coordination"]))
        if h.finished:
            break
        if h.advance(h.steps_until_dump()) == 0:
            break
    print(want)
    assert lines[1:] == want
    assert all(sum(int(c) for c in l.split(",")[4:]) == h.n for l in lines[1:])
    if extra:
        assert any(int(l.split(",")[1]) > 0 for l in lines[1:]), "no bonds in any row"
    rows = open(tmp_path / "r.csv").read().splitlines()
    assert rows[0] == "RLo, RHi, Count" and len(rows) == 201
    r_max = f32(10.0) * f32(flat.max_radius)
    counts = h.radial_counts(r_max, 200, member=0)
    assert counts.sum() > 0
    for b, line in enumerate(rows[1:]):
        assert line == "%.9g, %.9g, %d" % (b * float(r_max) / 200.0, (b + 1) * float(r_max) / 200.0, counts[b]), b
