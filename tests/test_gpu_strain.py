"""GPU: the strain analysis (pbSimStrainStats / pbSimStrainOf, csrc/pb_strain.hip) against tests/strain_ref.py on the
two states read back from the device.  Every comparison is exact: moments and rows are integers, d2min and the gradient
are compared as uint64 bit patterns, and the device's d2min must be what the host derives from the device's moments.
tests/test_strain_api.py pins the reference to a brute force and to known answers on the CPU.

Without the strain analysis every test here fails: the entry points do not exist."""
import os
import subprocess

import numpy as np
import pytest

import dynamics_ref as DR
import strain_ref as SR
from helpers import assert_bit_equal, jittered_blob, simparams_from_orc
from test_contacts_api import state_700

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
f32 = np.float32
u64 = np.uint64
GAP = 0.0019


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def sim_with(pb, orc, pos, rad, vel=None, wall_half=4.0e6):
    pos = np.asarray(pos, f32).reshape(-1, 2)
    n = pos.shape[0]
    P = orc.default_params(nCells=n, seed=3, max_time=1e9, nDead=0)
    sp, keep = simparams_from_orc(P)
    sim = pb.Sim(sp, wall_half=wall_half, keepalive=keep)
    sim.set_state(pos=pos, vel=np.zeros((n, 2), f32) if vel is None else vel, rad=np.asarray(rad, f32),
                  phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    return sim


def check(sim, member, st0, st1, gap, what, threshold=0.0, row=None):
    """Row and per-bot arrays of one member against the reference on the two read-back states; returns the reference."""
    want, wbots = SR.analyse(st0["pos"], st0["rad"], st1["pos"], gap, threshold)
    if row is None:
        row = sim.strain(threshold)[member]
    print(what, "gap", gap, {k: row[k] for k in ("fitted", "unfitted", "above", "bonds_used", "bonds_dropped", "sum_d2",
                                                  "max_d2")})
    assert tuple(row) == SR.FIELDS
    assert row == want, (what, gap, {k: (row[k], want[k]) for k in row if row[k] != want[k]})
    got = sim.strain_of(member)
    n = len(wbots["d2min"])
    assert got["moments"].dtype == np.int64 and got["moments"].shape == (n, 9)
    assert got["gradient"].dtype == np.float64 and got["gradient"].shape == (n, 2, 2)
    assert got["d2min"].dtype == np.float64 and got["d2min"].shape == (n,)
    bad = np.flatnonzero((got["moments"] != wbots["moments"]).any(axis=1))
    assert bad.size == 0, (what, gap, "moments", bad[:8])
    assert np.array_equal(got["d2min"].view(u64), wbots["d2min"].view(u64)), (what, "d2min bits")
    assert np.array_equal(got["gradient"].view(u64), wbots["gradient"].view(u64)), (what, "gradient bits")
    # the device's d2min is the value the host derives from the device's own moments
    fitted, grad, d2 = SR.fit_all(got["moments"])
    assert np.array_equal(got["d2min"].view(u64), d2.view(u64)) and np.array_equal(got["gradient"].view(u64),
                                                                                   grad.view(u64))
    # what holds whatever the state
    assert row["fitted"] + row["unfitted"] == n and row["above"] <= row["fitted"] == int(fitted.sum())
    assert row["bonds_used"] == int(got["moments"][:, 0].sum())
    assert row["bonds_used"] + row["bonds_dropped"] == int(SR.KR.topology(st0["pos"], st0["rad"], gap)[0][-1])
    assert (got["d2min"] >= 0).all() and (got["d2min"][~fitted] == 0).all() and (got["gradient"][~fitted] == 0).all()
    return want, wbots


def recipe(n):
    rng = np.random.default_rng(2000 + n)
    pos, vel, rad = jittered_blob(n, 0.15, rng, jitter=0.3)
    return pos, vel, rad, DR.perturbed(pos, rng)


# ---- sizes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_around_the_wave_and_the_workgroup(pb, orc, n):
    pos, vel, rad, pos1 = recipe(n)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st0 = sim.get_state()
    sim.mark_reference(GAP)
    # identity: the state against itself
    same, sbots = check(sim, 0, st0, st0, GAP, f"n {n} identity")
    assert same["sum_d2"] == same["max_d2"] == same["above"] == same["bonds_dropped"] == 0
    assert (sbots["gradient"][sbots["fitted"]] == np.eye(2)).all()
    sim.set_state(pos=pos1)
    st1 = sim.get_state()
    assert_bit_equal(st1["pos"], pos1, "pos1")
    want, _ = check(sim, 0, st0, st1, GAP, f"n {n}")
    assert want["fitted"] == same["fitted"]  # (nothing is dropped: the mark's moments decide who is fitted)
    if n >= 63:
        assert 0 < want["fitted"] and 0 < want["unfitted"] and want["sum_d2"] > 0
    else:
        assert want["fitted"] == 0 and want["unfitted"] == n


# ---- long lists ----------------------------------------------------------------------------------------------------------

def test_long_lists_of_a_large_gap(pb, orc):
    n, gap = 300, 0.3
    rng = np.random.default_rng(2300)
    pos, vel, rad = jittered_blob(n, 0.15, rng, jitter=0.3)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st0 = sim.get_state()
    sim.mark_reference(gap)
    sim.set_state(pos=DR.perturbed(pos, rng))
    want, wbots = check(sim, 0, st0, sim.get_state(), gap, "long lists")
    assert int(wbots["moments"][:, 0].max()) > 40 and want["fitted"] == n and want["sum_d2"] > 0


# ---- a batch -------------------------------------------------------------------------------------------------------------

def test_batch_of_three_members(pb, orc):
    members, n = 3, 257  # workgroups straddle members
    rng = np.random.default_rng(77)
    plist, keeps = [], []
    for k in range(members):
        P = orc.default_params(nCells=n, nDead=0, seed=70 + k, max_time=1e9)
        sp, keep = simparams_from_orc(P)
        plist.append(sp)
        keeps.append(keep)
    ens = pb.Ensemble(plist, wall_half=4.0e6, keepalive=keeps)
    for k in range(members):
        pos, vel, rad = jittered_blob(n, 0.15 + 0.01 * k, rng, center=(0.4 * k, -0.3 * k), jitter=0.3)
        ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    st0 = [ens.get_state_of(k) for k in range(members)]
    ens.mark_reference(GAP)
    # member 1 stays as it is, member 0 is jostled, member 2 is rotated and dilated as a whole and then jostled a little
    ens.set_state_of(0, pos=DR.perturbed(st0[0]["pos"], rng))
    turn = np.array([[0.8, -0.6], [0.6, 0.8]]) * 1.25
    moved = (st0[2]["pos"].astype(np.float64) @ turn.T).astype(f32)
    ens.set_state_of(2, pos=moved + (rng.standard_normal(moved.shape) * 0.002).astype(f32))
    rows = ens.strain(0.0001)
    assert len(rows) == members
    wants = [check(ens, k, st0[k], ens.get_state_of(k), GAP, f"member {k}", 0.0001, rows[k]) for k in range(members)]
    assert wants[1][0]["sum_d2"] == 0 and wants[1][0]["above"] == 0 and wants[1][0]["fitted"] > 200
    assert wants[0][0]["sum_d2"] > 100 * wants[2][0]["sum_d2"] > 0
    assert wants[0][0]["above"] > wants[2][0]["above"]
    F = pb.deformation_gradient(rows[2])
    assert np.abs(F - turn).max() < 0.01 and np.abs(pb.deformation_gradient(rows[1]) - np.eye(2)).max() == 0.0
    assert pb.mean_d2min(rows[0]) > pb.mean_d2min(rows[2]) > pb.mean_d2min(rows[1]) == 0.0


# ---- edge cases ----------------------------------------------------------------------------------------------------------

def test_non_finite_stretched_coincident_and_carried_away_bots(pb, orc):
    rng = np.random.default_rng(2600)
    pos0, _, rad0 = jittered_blob(180, 0.15, rng, jitter=0.3)
    n = rad0.size
    below = np.nextafter(f32(8.0), f32(0.0))
    pos0[5] = np.nan              # non-finite at the mark, finite now: no marked bonds
    pos0[11] = pos0[10]           # coincident at the mark: a bond of length 0
    sim = sim_with(pb, orc, pos0, rad0)
    st0 = sim.get_state()
    assert_bit_equal(st0["pos"], pos0, "pos0")
    sim.mark_reference(GAP)
    off, _, oth = SR.KR.topology(pos0, rad0, GAP)
    partner = lambda i: int(oth[off[i]])  # noqa: E731  (the first marked partner of a bot that has one)
    pos1 = DR.perturbed(pos0, rng, shift=0.0)
    pos1[5] = (0.0, 0.0)
    pos1[20] = np.nan             # non-finite now: its partners drop their bonds to it
    pos1[21, 0] = np.inf          # likewise, with one infinite coordinate
    pos1[13] = pos1[12]           # coincident now
    pos1[30] = pos0[30] + np.array([3000.0, 0.0], f32)   # carried far away: all its bonds are dropped at both ends
    a, b = 60, 100                # two bots well apart, each with a bond stretched along x to a chosen length
    ja, jb = partner(a), partner(b)
    pos1[a], pos1[ja] = (0.5, pos0[a, 1]), (8.5, pos0[ja, 1])        # dx = 8.0 exactly: dropped
    pos1[b], pos1[jb] = (0.0, pos0[b, 1]), (below, pos0[jb, 1])      # dx = nextafter(8, 0): used, the largest q
    sim.set_state(pos=pos1)
    st1 = sim.get_state()
    assert_bit_equal(st1["pos"], pos1, "pos1")
    want, wbots = check(sim, 0, st0, st1, GAP, "edge cases")
    k, dropped, length = wbots["moments"][:, 0], wbots["dropped"], np.diff(off.astype(np.int64))
    assert length[5] == 0 and k[5] == 0 and not wbots["fitted"][5]
    for gone in (20, 21, 30):
        assert length[gone] > 0 and k[gone] == 0 and dropped[gone] == length[gone] and not wbots["fitted"][gone]
        assert dropped[partner(gone)] >= 1
    assert dropped[a] >= 1 and dropped[ja] >= 1
    assert pos1[ja, 0] - pos1[a, 0] == f32(8.0) and pos1[jb, 0] - pos1[b, 0] == below
    q = 1 << 23
    assert int(wbots["moments"][b, 8]) >= q * q and dropped[b] < length[b]  # the bond at the largest q is used
    assert length[10] > 0 and length[11] > 0 and 11 in oth[off[10]:off[11]]
    assert want["bonds_dropped"] == int(dropped.sum()) > 6 and want["fitted"] > 100 and want["max_d2"] > 0


# ---- the threshold ---------------------------------------------------------------------------------------------------------

def test_thresholds_that_bracket_the_median(pb, orc):
    n = 1025
    pos, vel, rad, pos1 = recipe(n)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st0 = sim.get_state()
    sim.mark_reference(GAP)
    sim.set_state(pos=pos1)
    st1 = sim.get_state()
    _, wbots = SR.analyse(st0["pos"], st0["rad"], st1["pos"], GAP)
    median = float(np.median(wbots["d2min"][wbots["fitted"]])) / 2.0 ** 40
    counts = []
    for t in (0.5 * median, 2.0 * median):
        want, _ = check(sim, 0, st0, st1, GAP, f"threshold {t}", threshold=t)
        assert 0 < want["above"] < want["fitted"]
        counts.append(want["above"])
    assert counts[0] > want["fitted"] // 2 > counts[1]
    with pytest.raises(RuntimeError, match="code 2.*d2Threshold"):
        sim.strain(-1.0)


# ---- member sums beyond 64 bits ----------------------------------------------------------------------------------------------

def test_member_sums_beyond_64_bits(pb, orc):
    n, gap, scale = 20000, 0.3, f32(14.5)
    rng = np.random.default_rng(2000 + n)
    pos, vel, rad = jittered_blob(n, 0.15, rng, jitter=0.3)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st0 = sim.get_state()
    sim.mark_reference(gap)
    sim.set_state(pos=pos * scale)  # a dilation: every bond grows 14.5-fold and stays below the reach of 8
    want, wbots = check(sim, 0, st0, sim.get_state(), gap, "20000 bots dilated")
    assert want["w"] > 1 << 64 and want["bonds_dropped"] == 0 and want["fitted"] == n
    assert want["bonds_used"] > 700000 and int(wbots["moments"][:, 8].max()) < 1 << 63
    # the fp32 rounding of the dilated positions (below 2^8: half an ulp is 2^-17) moves a bond vector by 2^-16 at the
    # most, so a bot with fewer than 64 bonds keeps a residual below 64 * 2 * 2^-32; bonds are longer than 0.1
    F = pb.deformation_gradient(want)
    print(np.abs(F - 14.5 * np.eye(2)).max(), pb.mean_d2min(want), int(wbots["moments"][:, 0].max()))
    assert np.abs(st0["pos"] * scale).max() < 256 and int(wbots["moments"][:, 0].max()) < 64
    assert np.abs(F - 14.5 * np.eye(2)).max() < 2.0 ** -16 / 0.1 and pb.mean_d2min(want) < 128 * 2.0 ** -32


# ---- through re-sorts ------------------------------------------------------------------------------------------------------

def test_the_analysis_reads_through_re_sorts_and_changes_nothing(pb, orc):
    pos, vel, rad = state_700()
    n = rad.size

    def make():
        P = orc.default_params(nCells=n, nDead=0, seed=3, max_time=1e9)
        sp, keep = simparams_from_orc(P)
        s = pb.Sim(sp, wall_half=64.0, keepalive=keep)
        s.set_state(pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
        s.set_resort_every_step(1)
        return s

    sim, twin = make(), make()
    st0 = sim.get_state()
    sim.mark_reference(GAP)
    assert sim.step(150, dt=0.01) == 150 and twin.step(150, dt=0.01) == 150
    assert sim.stats()["resorts"] >= 150
    want, _ = check(sim, 0, st0, sim.get_state(), GAP, "700 bots, 150 steps")
    assert want["sum_d2"] > 0 and 0 < want["fitted"]
    assert sim.step(150, dt=0.01) == 150 and twin.step(150, dt=0.01) == 150
    st1 = sim.get_state()
    later, _ = check(sim, 0, st0, st1, GAP, "700 bots, 300 steps")
    assert later != want
    other = twin.get_state()
    for name in st1:
        assert_bit_equal(st1[name], other[name], name)
    assert sim.stats() == twin.stats() and sim.time == twin.time


# ---- sessions --------------------------------------------------------------------------------------------------------------

def others(sim):
    """What the other analyses that share the scratch say, as comparable values."""
    rows, totals = sim.pair_correlation("displacement", 1.0, 50)
    re = sim.rearrangement_of()
    return (sim.rearrangement(), {k: v.tobytes() for k, v in re.items()}, sim.clusters(GAP),
            [c.tobytes() for c in sim.cluster_labels(GAP)], sim.structure(GAP), sim.radial_counts(1.0, 64).tobytes(),
            rows.tobytes(), totals)


def test_sessions(pb, orc):
    n = 257
    pos, vel, rad, pos1 = recipe(n)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    assert sim.strain_times() == (0, 0.0)
    for call in (sim.strain, sim.strain_of):  # a fresh simulation holds no mark
        with pytest.raises(RuntimeError, match="code 2.*no reference marked"):
            call()
    with pytest.raises(RuntimeError, match="code 2.*member out of range"):
        sim.strain_of(1)
    assert sim.strain_times() == (0, 0.0)
    st0 = sim.get_state()
    sim.mark_reference(GAP)
    sim.set_state(pos=pos1)
    st1 = sim.get_state()
    before = others(sim)
    marks = sim.rearrangement_times()[0]
    want, wbots = check(sim, 0, st0, st1, GAP, "first session", threshold=0.001)
    t = sim.strain_times()
    assert t[0] == 2 and t[1] > 0.0                      # the row and the per-bot call of check
    assert sim.rearrangement_times()[0] == marks         # the strain analysis has a clock of its own
    again = sim.strain(0.001)[0]
    assert again == want
    assert others(sim) == before                         # bit for bit what they said before the strain calls
    assert sim.strain(0.001)[0] == want                  # ... and the strain answer after them
    for name, v in sim.get_state().items():
        assert_bit_equal(v, st1[name], name)
    # the same answer in a fresh session
    fresh = sim_with(pb, orc, pos, rad, vel=vel)
    fresh.mark_reference(GAP)
    fresh.set_state(pos=pos1)
    assert fresh.strain(0.001)[0] == want
    got, first = fresh.strain_of(), sim.strain_of()
    for k in got:
        assert np.array_equal(got[k].view(u64), first[k].view(u64)), k
    # a replaced mark: another gap, of the state as it is now, then back
    sim.mark_reference(0.3)
    sim.set_state(pos=pos)
    wide, _ = check(sim, 0, st1, st0, 0.3, "replaced mark")
    assert wide["bonds_used"] > 4 * want["bonds_used"]
    # cleared, refused, marked anew: the first answer again
    sim.clear_reference()
    with pytest.raises(RuntimeError, match="code 2.*no reference marked"):
        sim.strain()
    sim.mark_reference(GAP)
    sim.set_state(pos=pos1)
    assert sim.strain(0.001)[0] == want
    assert np.array_equal(sim.strain_of()["d2min"].view(u64), first["d2min"].view(u64))


# ---- the runner ----------------------------------------------------------------------------------------------------------

HEADER = ("Time, MarkTime, Fitted, Unfitted, Above, BondsUsed, BondsDropped, Yxx, Yxy, Yyy, Xxx, Xxy, Xyx, Xyy, W, SumD2, "
          "MaxD2")
THRESHOLD = 0.0001


@pytest.mark.parametrize("window, rearrange", [(False, False), (True, False), (True, True)])
def test_runner_writes_strain_rows(tmp_path, window, rearrange):
    from particlerobotsimulations_amd import host
    cfg = os.path.join(ROOT, "examples", "example.cfg")
    over = dict(max_time="3", dump_interval="1")
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    flags = ["--strain", "s.csv", "--strain-threshold", str(THRESHOLD), "--rearrange-gap", str(GAP)]
    flags += ["--rearrange-window"] if window else []
    flags += ["--rearrange", "a.csv"] if rearrange else []
    r = subprocess.run([RUN, cfg, "--quiet"] + sets + flags, capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert os.path.exists(tmp_path / "a.csv") == rearrange
    lines = open(tmp_path / "s.csv").read().splitlines()
    assert lines[0] == HEADER
    main_times = [l.split(",")[0] for l in open(tmp_path / "example_data.csv").read().splitlines()[2:]]
    cells = [[c.strip() for c in l.split(",")] for l in lines[1:]]
    assert [c[0] for c in cells] == main_times and len(main_times) >= 4
    first = cells[0]
    assert int(first[2]) > 0 and first[4] == "0" and first[6] == "0" and first[15:] == ["0", "0"]
    assert first[7] == first[10] and first[9] == first[13]  # the identity: X = Y
    if window:
        assert [c[1] for c in cells[1:]] == [c[0] for c in cells[:-1]]  # MarkTime advances with the rows
    else:
        assert all(c[1] == cells[0][0] for c in cells)
    assert any(int(c[15]) > 0 for c in cells[1:]), "nothing deformed in any row"
    # the same rows from the class driven by hand
    flat = host.load_config(cfg, **over)
    h = host.HostSim(cfg, engine="fused", **over)
    di = f32(flat.dump_interval)

    def due(t):  # the gate of dumpParticlebot, in its fp32 operations
        t = f32(t)
        return not (t - di * np.floor(t / di) > f32(0.01))

    want, rwant, mark_time = [], [], None
    while True:
        if due(h.time):
            if mark_time is None:
                h.mark_reference(GAP)
                mark_time = h.time
            if rearrange:
                rwant.append(h.rearrangement()[0])
            s = h.strain(THRESHOLD)[0]
            want.append("%f, %f, " % (h.time, mark_time) + ", ".join(str(s[k]) for k in SR.FIELDS))
            if window:
                h.mark_reference(GAP)
                mark_time = h.time
        if h.finished:
            break
        if h.advance(h.steps_until_dump()) == 0:
            break
    print(want)
    assert lines[1:] == want
    # the class's per-bot call: the same moments as its own row, and d2min the fit of those moments
    s, bots = h.strain(THRESHOLD)[0], h.strain_of()
    assert bots["moments"].shape == (h.n, 9) and bots["gradient"].shape == (h.n, 2, 2) and bots["d2min"].shape == (h.n,)
    assert [int(v) for v in bots["moments"].sum(axis=0)] == [s["bonds_used"]] + [s[k] for k in SR.SUMS]
    fitted, grad, d2 = SR.fit_all(bots["moments"])
    assert int(fitted.sum()) == s["fitted"] and np.array_equal(bots["d2min"].view(u64), d2.view(u64))
    assert np.array_equal(bots["gradient"].view(u64), grad.view(u64))
    if rearrange:  # the rearrangement rows are the ones --rearrange writes on its own, strain calls in between or not
        rl = [[c.strip() for c in l.split(",")] for l in open(tmp_path / "a.csv").read().splitlines()[1:]]
        assert [(int(c[2]), int(c[3]), int(c[4]), int(c[11])) for c in rl] == [
            (s["bonds_marked"], s["bonds_now"], s["bonds_kept"], s["sum_q2"]) for s in rwant]
        assert [c[:2] for c in rl] == [c[:2] for c in cells]
