"""GPU: the cluster analysis (pbSimClusterStats / pbSimClusterLabelsOf, csrc/pb_cluster.hip) against tests/cluster_ref.py
on the state read back from the device.  Every comparison is exact: stats, labels and degrees are integers.
tests/test_cluster_api.py pins the reference to a brute force on the CPU.  A case is non-trivial when the reference
reports 1 < clusters < n and largest > 1; every parametrised case asserts that for at least one of its gaps, so
neither an all-isolated nor an all-one answer passes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_ref as CR
from helpers import assert_bit_equal, jittered_blob, simparams_from_orc
from test_cluster_api import EXAMPLES, GAPS, cfg_path, two_blobs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
f32 = np.float32


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def strip(row):
    return {k: row[k] for k in CR.FIELDS}


def check_member(sim, member, gap, pos, rad, what, row=None):
    """Device stats, labels and degrees of one member against the reference on (pos, rad); returns the reference stats."""
    want, wlab, wdeg = CR.analyse(pos, rad, gap)
    if row is None:
        row = sim.clusters(gap)[member]
    print(what, gap, row)
    assert strip(row) == want, (what, gap, row, want)
    lab, deg = sim.cluster_labels(gap, member=member)
    assert np.array_equal(deg, wdeg), (what, gap, "degree")
    assert np.array_equal(lab, wlab), (what, gap, "labels")
    return want


# ---- the examples ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("example", EXAMPLES)
def test_examples_placed_and_stepped(example):
    from particlerobotsimulations_amd import host
    h = host.HostSim(cfg_path(example), engine="fused", max_time="1e9", sort_interval="1.5", phase_update_interval="2")
    some = False
    for steps in (0, 350):
        assert h.advance(steps) == steps
        pos, rad = h.get("pos"), h.get("rad")
        for gap in GAPS:
            want, wlab, wdeg = CR.analyse(pos, rad, gap)
            got = h.clusters(gap)
            print(example, steps, gap, got)
            assert strip(got) == want, (example, steps, gap, got, want)
            lab, deg = h.cluster_labels(gap)
            assert np.array_equal(lab, wlab) and np.array_equal(deg, wdeg), (example, steps, gap)
            some |= CR.nontrivial(want, h.n)
        assert_bit_equal(h.get("pos"), pos, "the analysis moved nothing")
    assert some, "every state and gap of this example is trivial"


# ---- batches, lanes and forms ------------------------------------------------------------------------------------------

def make_batch(pb, orc, members, n, spacing=0.2, seed0=100, dead_step=0.05, wall_half=0.0):
    rng = np.random.default_rng(seed0)
    plist, keeps, states = [], [], []
    for k in range(members):
        P = orc.default_params(nCells=n, nDead=0, seed=seed0 + k, max_time=1e9, phase_update_interval=0.3)
        sp, keep = simparams_from_orc(P)
        plist.append(sp)
        keeps.append(keep)
    ens = pb.Ensemble(plist, wall_half=wall_half, keepalive=keeps)
    for k in range(members):
        pos, vel, rad = jittered_blob(n, spacing, rng, center=(0.3 * k, -0.2 * k), jitter=0.3)
        dead = (rng.random(n) < dead_step * k).astype(np.int32)
        ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=rng.uniform(0, 6.28, n).astype(f32), dead=dead)
        states.append((pos, rad))
    return ens, states


def check_batch(ens, what, gaps=(0.0, 0.0019)):
    some = False
    for gap in gaps:
        rows = ens.clusters(gap)
        assert len(rows) == ens.nsims
        for k in range(ens.nsims):
            st = ens.get_state_of(k)
            some |= CR.nontrivial(check_member(ens, k, gap, st["pos"], st["rad"], f"{what} member {k}", rows[k]), ens.n)
    assert some, f"{what}: every member and gap is trivial"


def test_batch_of_16_members_each_against_its_own_reference(pb, orc):
    ens, states = make_batch(pb, orc, 16, 700)
    # members 3 and 4 on top of each other, bot for bot: a link across members would double their degrees
    ens.set_state_of(4, pos=states[3][0], rad=states[3][1])
    check_batch(ens, "as set")
    a, b = ens.cluster_labels(0.0019, member=3), ens.cluster_labels(0.0019, member=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert ens.step(120, dt=0.01, sort_interval=0.5) == 120  # re-sorts and phase updates: slots leave original order
    assert ens.stats()["resorts"] >= 2
    check_batch(ens, "after 120 steps")


@pytest.mark.parametrize("members,n,resident,lanes", [(8, 300, 2, 0), (8, 300, 1, 0), (2, 600, 1, 64), (2, 3000, 1, 16),
                                                       (1, 20000, 1, 4), (1, 20000, 1, 1)])
def test_resident_and_multi_lane_forms_give_the_same_analysis(pb, orc, members, n, resident, lanes):
    def run(res, ln):
        ens, _ = make_batch(pb, orc, members, n, seed0=7)
        ens.set_resident(res)
        ens.set_lanes_per_bot(ln)
        assert ens.step(150, dt=0.01, sort_interval=0.4) == 150
        return ens

    ens = run(resident, lanes)
    if resident == 2:
        assert ens.stats()["resident_launches"] > 0
    else:
        assert ens.stats()["resident_launches"] == 0
        assert lanes == 0 or ens.config()["lanes_per_bot"] == lanes
    check_batch(ens, f"resident {resident} lanes {lanes}")
    base = run(1, 0)  # per-step launches, automatic lanes
    for gap in (0.0, 0.0019):
        assert [strip(r) for r in ens.clusters(gap)] == [strip(r) for r in base.clusters(gap)]
        for k in range(members):
            a, b = ens.cluster_labels(gap, member=k), base.cluster_labels(gap, member=k)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- hand-made cases -------------------------------------------------------------------------------------------------

def sim_with(pb, orc, pos, rad, wall_half=4.0e6):
    pos = np.asarray(pos, f32).reshape(-1, 2)
    n = pos.shape[0]
    P = orc.default_params(nCells=n, nDead=0, seed=3, max_time=1e9)
    sp, keep = simparams_from_orc(P)
    sim = pb.Sim(sp, wall_half=wall_half, keepalive=keep)
    sim.set_state(pos=pos, vel=np.zeros((n, 2), f32), rad=np.asarray(rad, f32), phase=np.zeros(n, f32),
                  dead=np.zeros(n, np.int32))
    return sim


def test_hand_made_cases_on_the_device(pb, orc):
    tiny = float(np.nextafter(f32(0), f32(1)))
    pos, rad = np.array([[0.0, 0.0], [0.1875, 0.0]], f32), np.array([0.09375, 0.09375], f32)
    sim = sim_with(pb, orc, pos, rad)
    assert check_member(sim, 0, 0.0, pos, rad, "tangent")["links"] == 0
    assert check_member(sim, 0, tiny, pos, rad, "tangent")["links"] == 1
    pos, rad = np.array([[3.0, -2.0]] * 3 + [[50.0, 50.0]], f32), np.full(4, 0.1, f32)
    assert check_member(sim_with(pb, orc, pos, rad), 0, 0.0, pos, rad, "coincident")["links"] == 3
    pos = np.array([[0.0, 0.0], [0.1, 0.0], [np.nan, 0.0], [0.05, 0.0], [0.0, np.inf]], f32)
    rad = np.array([0.1, 0.1, 0.1, np.inf, 0.1], f32)
    assert check_member(sim_with(pb, orc, pos, rad), 0, 0.05, pos, rad, "non-finite")["clusters"] == 4
    pos, rad = two_blobs(300, 200)
    assert check_member(sim_with(pb, orc, pos, rad), 0, 0.0019, pos, rad, "two blobs")["clusters"] == 2
    pos, rad = two_blobs(150, 150)
    order = np.empty(300, np.int64)
    order[0::2], order[1::2] = np.arange(150), 150 + np.arange(150)
    pos = np.concatenate([np.array([[0.0, 500.0]], f32), pos[order]])
    rad = np.concatenate([np.array([0.1], f32), rad[order]])
    want = check_member(sim_with(pb, orc, pos, rad), 0, 0.0019, pos, rad, "tie")
    assert want["largest"] == 150 and want["largest_label"] == 1


def test_walls_corners_and_outside_the_arena(pb, orc):
    rng = np.random.default_rng(5)
    W = 64.0
    parts = []
    for c in ((W, 0.0), (-W, 0.0), (0.0, W), (0.0, -W), (W, W), (-W, -W), (W, -W), (-W, W),  # walls and corners
              (3.0e5, -7.0e5), (-1048576.0 + 3.0, 1048576.0 - 3.0), (0.0, 0.0)):        # far outside; the edge of the range
        p, _, r = jittered_blob(120, 0.2, rng, center=c, jitter=0.3)
        parts.append((np.clip(p, -1048576.0, 1048576.0) if abs(c[0]) > 1e6 else p, r))
    pos = np.concatenate([p for p, _ in parts]).astype(f32)
    rad = np.concatenate([r for _, r in parts])
    on_wall = np.clip(pos[:960], -W, W)  # the first eight blobs pressed onto the walls, as the integrator's clamp does
    pos[:960] = on_wall
    sim = sim_with(pb, orc, pos, rad)
    some = False
    for gap in GAPS:
        some |= CR.nontrivial(check_member(sim, 0, gap, pos, rad, "walls"), rad.size)
    assert some


def test_argument_errors_on_a_real_batch(pb, orc):
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    ens, _ = make_batch(pb, orc, 2, 50)
    buf = np.zeros(50, np.uint32)
    assert L.pbSimClusterLabelsOf(ens._h, 2, 0.0, _capi.np_ptr(buf), None) == 2
    assert b"pbSimClusterLabelsOf" in L.pbGetLastErrorString() and b"member" in L.pbGetLastErrorString()
    assert ens.cluster_times() == (0, 0.0)  # nothing ran, nothing was allocated
    lab, _ = ens.cluster_labels(0.0, member=1)
    only_labels = np.zeros(50, np.uint32)
    assert L.pbSimClusterLabelsOf(ens._h, 1, 0.0, _capi.np_ptr(only_labels), None) == 0
    assert np.array_equal(only_labels, lab)
    assert ens.cluster_times()[0] == 2 and ens.cluster_times()[1] > 0.0


# ---- convergence -------------------------------------------------------------------------------------------------------

def test_chain_of_100000_bots_converges_in_few_rounds(pb, orc):
    """One serpentine chain, every bot linked to its neighbours along the path only: lattice step 0.19, radius 0.1
    (0.19 < 0.2 links, the diagonal 0.2687 does not), rows three steps apart joined by two connector bots.  The cap
    of 64 rounds is a condition, not a measurement: hooking plus pointer jumping needs O(log n) ~ 17 rounds, label
    propagation ~ 10^5."""
    L, rows, s = 998, 100, 0.19
    pts = []
    for r in range(rows):
        xs = range(L) if r % 2 == 0 else range(L - 1, -1, -1)
        pts += [(x, 3 * r) for x in xs]
        end = L - 1 if r % 2 == 0 else 0
        pts += [(end, 3 * r + 1), (end, 3 * r + 2)]
    n = len(pts)
    assert n == 100000
    path = (np.array(pts, np.float64) * s).astype(f32)
    perm = np.random.default_rng(11).permutation(n)  # original indices unrelated to the position along the chain
    pos = np.empty_like(path)
    pos[perm] = path
    rad = np.full(n, 0.1, f32)
    sim = sim_with(pb, orc, pos, rad, wall_half=512.0)
    row = sim.clusters(0.0)[0]
    print("chain", row)
    assert row["clusters"] == 1 and row["largest"] == n and row["largest_label"] == 0
    assert row["links"] == n - 1 and row["max_degree"] == 2 and row["isolated"] == 0
    assert row["rounds"] <= 64
    lab, deg = sim.cluster_labels(0.0)
    assert not lab.any() and np.bincount(deg).tolist() == [0, 2, n - 2]
    assert strip(row) == CR.analyse(pos, rad, 0.0)[0]


# ---- scale -------------------------------------------------------------------------------------------------------------

@pytest.mark.slow
def test_million_bot_arena(pb):
    """The arena bench.py times, after 32 steps.  The CPU oracle gives, for this state, 55 293 clusters at gap 0 (the
    largest holds 577 178 bots, 1 998 are isolated, 1 525 356 links) and one cluster of 10^6 with 1 998 000 links at
    gap 0.0019: the first is the non-trivial case, the second the largest single component the forest can be asked
    for."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import benchkit
    n = 1000000
    sim = benchkit.make_sim(pb, n, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    st = sim.get_state()
    some = False
    for gap in (0.0, 0.0019):
        want = check_member(sim, 0, gap, st["pos"], st["rad"], "10^6 bots")
        some |= CR.nontrivial(want, n)
        print("device ms:", sim.cluster_times()[1])
    assert some, "the arena is trivial at both gaps"


# ---- nothing changes ---------------------------------------------------------------------------------------------------

def layout_of(ens, k):
    import ctypes as C
    from particlerobotsimulations_amd import _capi
    orig, keys, srt = np.empty(ens.n, np.uint32), np.empty(ens.n, np.uint32), C.c_int(0)
    _capi.check(_capi.lib().pbSimGetLayoutOf(ens._h, k, _capi.np_ptr(orig), _capi.np_ptr(keys), C.byref(srt)), "layout")
    return orig, keys, srt.value


def test_twin_simulations_one_analysed_one_not(pb, orc):
    a, _ = make_batch(pb, orc, 3, 900, seed0=40)
    b, _ = make_batch(pb, orc, 3, 900, seed0=40)
    for chunk in range(6):  # 300 steps: re-sorts every 0.7, phase updates every 0.3
        assert a.step(50, dt=0.01, sort_interval=0.7) == 50
        assert b.step(50, dt=0.01, sort_interval=0.7) == 50
        a.clusters(0.0019)
        a.cluster_labels(0.0, member=chunk % 3)
    assert a.stats() == b.stats() and a.stats()["resorts"] >= 3 and a.stats()["phase_updates"] >= 5
    assert a.time == b.time and a.phase_draws == b.phase_draws
    for k in range(3):
        sa, sb = a.get_state_of(k), b.get_state_of(k)
        for name in sa:
            assert_bit_equal(sa[name], sb[name], f"member {k} {name}")
        la, lb = layout_of(a, k), layout_of(b, k)
        assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1]) and la[2] == lb[2] == 1


def test_checkpoint_after_an_analysis_resumes_bit_identically(tmp_path):
    from particlerobotsimulations_amd import host
    over = dict(max_time="1e9", sort_interval="1.5", phase_update_interval="2")
    path = cfg_path("example_obstacle.cfg")
    a = host.HostSim(path, engine="fused", **over)
    assert a.advance(230) == 230
    a.clusters(0.0019)
    a.save_checkpoint(str(tmp_path / "ck"))
    b = host.HostSim(path, engine="fused", **over)
    b.load_checkpoint(str(tmp_path / "ck"))
    c = host.HostSim(path, engine="fused", **over)  # never analysed, never checkpointed
    assert c.advance(230) == 230
    for h in (a, b, c):
        assert h.advance(240) == 240
    for name in ("pos", "vel", "rad", "phase"):
        assert_bit_equal(b.get(name), a.get(name), name)
        assert_bit_equal(c.get(name), a.get(name), name)
    assert strip(a.clusters(0.0019)) == strip(b.clusters(0.0019)) == strip(c.clusters(0.0019))


# ---- the runner --------------------------------------------------------------------------------------------------------

def test_runner_writes_cluster_rows_at_the_dump_times(tmp_path):
    from particlerobotsimulations_amd import host
    cfg = cfg_path("example_dead_cells.cfg")
    over = ["--set", "max_time", "6", "--set", "dump_interval", "1", "--set", "time_to_dead", "2"]
    a_csv, b_csv, c_csv = str(tmp_path / "a.csv"), str(tmp_path / "b.csv"), str(tmp_path / "f.csv")
    r = subprocess.run([RUN, cfg, "--quiet", "--set", "csv_filename", a_csv] + over, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([RUN, cfg, "--quiet", "--set", "csv_filename", b_csv, "--clusters", c_csv, "--cluster-gap",
                        "0.0019"] + over, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(a_csv, "rb").read() == open(b_csv, "rb").read()
    lines = open(c_csv).read().splitlines()
    assert lines[0] == "Time, Clusters, Largest, Isolated, Links, MaxDegree"
    main_times = [l.split(",")[0] for l in open(a_csv).read().splitlines()[2:]]
    assert [l.split(",")[0] for l in lines[1:]] == main_times and len(main_times) >= 6
    h = host.HostSim(cfg, engine="fused", max_time="6", dump_interval="1", time_to_dead="2")
    want = []

    def due(t, di=f32(1.0)):  # the gate of dumpParticlebot, in its fp32 operations
        t = f32(t)
        return not (t - di * np.floor(t / di) > f32(0.01))

    while True:
        s = h.clusters(0.0019) if due(h.time) else None
        if s:
            want.append("%f, %d, %d, %d, %d, %d" % (h.time, s["clusters"], s["largest"], s["isolated"], s["links"],
                                                    s["max_degree"]))
        if h.finished:
            break
        k = h.steps_until_dump()
        if h.advance(k) == 0:
            break
    assert lines[1:] == want
    ints = np.array([[int(v) for v in l.split(",")[1:]] for l in lines[1:]])
    assert ((ints[:, 0] > 1) & (ints[:, 0] < h.n) & (ints[:, 1] > 1)).any(), "every row is trivial"
