"""GPU: the rearrangement analysis (pbSimMarkReference / pbSimRearrangementStats / pbSimRearrangementOf,
csrc/pb_dynamics.hip) against tests/dynamics_ref.py on the two states read back from the device.  Every comparison is
exact: bond counts and displacement sums are integers, displacements are compared as bit patterns.
tests/test_dynamics_api.py pins the reference to a brute force and to known answers on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import dynamics_ref as DR
from helpers import assert_bit_equal, jittered_blob, simparams_from_orc
from test_contacts_api import state_700

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
f32 = np.float32
GAP = 0.0019


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


def invariants(row, bots, n):
    for k in ("bonds_marked", "bonds_now", "bonds_kept"):
        assert row[k] % 2 == 0, (k, row)
    assert row["bonds_kept"] <= min(row["bonds_marked"], row["bonds_now"])
    assert (bots["kept"] <= np.minimum(bots["marked"], bots["now"])).all()
    for k in ("marked", "now", "kept"):
        assert int(bots[k].astype(np.int64).sum()) == row["bonds_" + k], k
    assert row["bots_unchanged"] >= n - row["bots_lost"] - row["bots_gained"]
    assert row["bots_unchanged"] + row["bots_lost"] <= n and row["measured"] <= n


def check(sim, member, st0, st1, gap, what, row=None):
    """Row and per-bot arrays of one member against the reference on the two read-back states; returns the reference."""
    want, wbots = DR.analyse(st0["pos"], st0["rad"], st1["pos"], st1["rad"], gap)
    if row is None:
        row = sim.rearrangement()[member]
    print(what, "gap", gap, row)
    assert row == want, (what, gap, row, want)
    got = sim.rearrangement_of(member)
    assert got["disp"].dtype == f32 and got["disp"].shape == wbots["disp"].shape
    for k in ("marked", "now", "kept"):
        assert got[k].dtype == np.uint32
        assert np.array_equal(got[k], wbots[k]), (what, gap, k, np.flatnonzero(got[k] != wbots[k])[:8])
    fin = np.isfinite(wbots["disp"])
    assert np.array_equal(got["disp"].view(np.uint32)[fin], wbots["disp"].view(np.uint32)[fin]), (what, "disp bits")
    assert np.array_equal(np.isnan(got["disp"])[~fin], np.isnan(wbots["disp"])[~fin]), (what, "disp NaN-ness")
    assert np.array_equal(np.isfinite(got["disp"]), fin)
    invariants(row, got, len(wbots["marked"]))
    return want, wbots


def recipe(n):
    rng = np.random.default_rng(2000 + n)
    pos, vel, rad = jittered_blob(n, 0.15, rng, jitter=0.3)
    return pos, vel, rad, DR.perturbed(pos, rng)


# ---- sizes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_around_the_wave_and_the_workgroup(pb, orc, n):
    pos, vel, rad, pos1 = recipe(n)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st0 = sim.get_state()
    sim.mark_reference(GAP)
    # identity: the state against itself
    same, _ = check(sim, 0, st0, st0, GAP, f"n {n} identity")
    assert same["bonds_kept"] == same["bonds_marked"] == same["bonds_now"] and same["bots_unchanged"] == n
    assert same["bots_lost"] == same["bots_gained"] == 0 and same["measured"] == n
    assert same["sum_qx"] == same["sum_qy"] == same["sum_q2"] == same["max_q2"] == 0
    sim.set_state(pos=pos1)
    st1 = sim.get_state()
    assert_bit_equal(st1["pos"], pos1, "pos1")
    want, wbots = check(sim, 0, st0, st1, GAP, f"n {n}")
    assert want["measured"] == n
    if n >= 63:
        broken, formed = want["bonds_marked"] - want["bonds_kept"], want["bonds_now"] - want["bonds_kept"]
        assert 0 < broken < want["bonds_marked"] and 0 < formed < want["bonds_now"]
        assert 0 < want["bonds_kept"] and 0 < want["bots_unchanged"] < n
        assert 0 < want["bots_lost"] < n and 0 < want["bots_gained"] < n
    figures = {63: (284, 276, 234, 15), 257: (1278, 1208, 1018, 32), 1025: (5354, 5188, 4306, 147)}
    if n in figures:
        assert (want["bonds_marked"], want["bonds_now"], want["bonds_kept"], want["bots_unchanged"]) == figures[n]
    if n == 1025:
        assert int(wbots["marked"].max()) == 9  # a marked list longer than the eight registers


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
    assert wbots["marked"].mean() > 25 and int(wbots["marked"].max()) > 40 and int(wbots["marked"].min()) > 8
    assert 0 < want["bonds_kept"] < min(want["bonds_marked"], want["bonds_now"])


# ---- a batch -------------------------------------------------------------------------------------------------------------

def test_batch_of_three_members(pb, orc):
    members, n = 3, 257
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
    info = ens.reference_info()
    # member 1 stays as it is, the others move differently
    ens.set_state_of(0, pos=DR.perturbed(st0[0]["pos"], rng))
    ens.set_state_of(2, pos=DR.perturbed(st0[2]["pos"], rng, shift=-0.5))
    rows = ens.rearrangement()
    assert len(rows) == members
    wants = []
    for k in range(members):
        want, wbots = check(ens, k, st0[k], ens.get_state_of(k), GAP, f"member {k}", rows[k])
        wants.append((want, wbots))
    assert info["entries"] == sum(w["bonds_marked"] for w, _ in wants)
    assert wants[1][0]["bots_unchanged"] == n and wants[1][0]["sum_q2"] == 0
    for k in (0, 2):
        assert 0 < wants[k][0]["bots_unchanged"] < n and wants[k][0]["sum_q2"] > 0
    assert wants[0][0] != wants[2][0]
    assert not np.array_equal(wants[0][1]["marked"], wants[1][1]["marked"])
    assert not np.array_equal(wants[1][1]["marked"], wants[2][1]["marked"])


# ---- through re-sorts ------------------------------------------------------------------------------------------------------

def test_the_mark_survives_re_sorts_and_changes_nothing(pb, orc):
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
    mid = sim.get_state()
    want, wbots = check(sim, 0, st0, mid, GAP, "700 bots, 150 steps")
    assert 0 < want["bonds_kept"] < want["bonds_marked"] and want["sum_q2"] > 0 and want["measured"] == n
    assert sim.step(150, dt=0.01) == 150 and twin.step(150, dt=0.01) == 150
    st1 = sim.get_state()
    check(sim, 0, st0, st1, GAP, "700 bots, 300 steps")
    other = twin.get_state()
    for name in st1:
        assert_bit_equal(st1[name], other[name], name)
    assert sim.stats() == twin.stats() and sim.time == twin.time


# ---- edge cases ----------------------------------------------------------------------------------------------------------

def test_non_finite_coincident_carried_away_and_folded_bots(pb, orc):
    rng = np.random.default_rng(2600)
    a, va, ra = jittered_blob(120, 0.15, rng, jitter=0.3)
    b, vb, rb = jittered_blob(60, 0.15, rng, center=(1.0e5, -1.0e5), jitter=0.3)  # folds onto the first on the grid
    pos0, rad0 = np.concatenate([a, b]), np.concatenate([ra, rb])
    n = rad0.size
    below = np.nextafter(f32(2048.0), f32(0.0))
    pos0[5] = np.nan              # non-finite at the mark, finite now
    rad0[7] = np.inf              # a non-finite radius at the mark: no links then, but a position that is kept
    pos0[11] = pos0[10]           # coincident at the mark
    pos0[40, 0] = 0.5
    pos0[41, 0] = 0.0
    pos0[42, 1] = 0.0
    sim = sim_with(pb, orc, pos0, rad0)
    st0 = sim.get_state()
    assert_bit_equal(st0["pos"], pos0, "pos0")
    sim.mark_reference(GAP)
    pos1, rad1 = DR.perturbed(pos0, rng, shift=0.0), rad0.copy()
    rad1[7] = ra[7]
    pos1[5] = a[5]
    pos1[20] = np.nan             # non-finite now
    pos1[21, 0] = np.inf          # likewise, with one infinite coordinate: dx is inf, dy finite
    pos1[13] = pos1[12]           # coincident now
    pos1[30] = pos0[30] + np.array([3000.0, 0.0], f32)  # carried away: not measured, its bonds broken at both ends
    pos1[40] = pos0[40] + np.array([2048.0, 0.0], f32)  # exactly 2048: not measured
    pos1[41] = pos0[41] + np.array([below, 0.0], f32)   # just below: measured
    pos1[42] = pos0[42] - np.array([0.0, below], f32)
    sim.set_state(pos=pos1, rad=rad1)
    st1 = sim.get_state()
    want, wbots = check(sim, 0, st0, st1, GAP, "edge cases")
    disp = wbots["disp"]
    assert disp[40, 0] == 2048.0 and disp[41, 0] == below and disp[42, 1] == -below and disp[30, 0] > 2048.0
    assert np.isnan(disp[5]).all() and np.isnan(disp[20]).all() and np.isinf(disp[21, 0]) and np.isfinite(disp[21, 1])
    assert np.isfinite(disp[7]).all()
    assert want["measured"] == n - 5  # bots 5, 20, 21, 30 and 40
    assert wbots["marked"][5] == 0 and wbots["marked"][7] == 0 and wbots["now"][5] > 0 and wbots["now"][7] > 0
    assert wbots["marked"][20] > 0 and wbots["now"][20] == 0 and wbots["kept"][20] == 0
    assert wbots["marked"][21] > 0 and wbots["now"][21] == 0 and wbots["kept"][21] == 0
    assert wbots["marked"][30] > 0 and wbots["now"][30] == 0 and wbots["kept"][30] == 0
    assert wbots["marked"][10] > 0 and wbots["marked"][11] > 0 and wbots["now"][12] > 0
    assert want["max_q2"] == ((1 << 31) - 128) ** 2  # the largest q there is
    second = slice(120, n)  # the far sub-blob is analysed like the near one
    assert wbots["marked"][second].sum() > 0 and wbots["kept"][second].sum() > 0
    assert (wbots["kept"][second] < wbots["marked"][second]).any()


# ---- the 128-bit sum -------------------------------------------------------------------------------------------------------

def test_sum_of_squares_beyond_64_bits(pb, orc):
    n = 20000
    rng = np.random.default_rng(2000 + n)
    pos, vel, rad = jittered_blob(n, 0.15, rng, jitter=0.3)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st0 = sim.get_state()
    sim.mark_reference(GAP)
    pos1 = pos + (rng.standard_normal(pos.shape) * 0.03).astype(f32) + np.array([1500.5, -1200.25], f32)
    sim.set_state(pos=pos1)
    want, _ = check(sim, 0, st0, sim.get_state(), GAP, "20000 bots")
    assert want["sum_q2"] > 1 << 64 and want["max_q2"] < 1 << 63 and want["measured"] == n
    assert pb.mean_squared_displacement(want) == pytest.approx(1500.5 ** 2 + 1200.25 ** 2, rel=1e-3)
    assert pb.mean_squared_displacement(want, subtract_drift=True) == pytest.approx(2 * 0.03 ** 2, rel=0.1)


# ---- lifecycle -------------------------------------------------------------------------------------------------------------

def test_lifecycle_of_the_mark(pb, orc):
    n = 257
    pos, vel, rad, pos1 = recipe(n)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    assert sim.rearrangement_times() == (0, 0.0)
    none = {"marked": False, "gap": 0.0, "time": 0.0, "entries": 0}
    assert sim.reference_info() == none
    for call in (sim.rearrangement, sim.rearrangement_of):  # a fresh simulation holds no mark
        with pytest.raises(RuntimeError, match="code 2.*no reference marked"):
            call()
    assert sim.rearrangement_times() == (0, 0.0)
    sim.time = 1.25
    st0 = sim.get_state()
    sim.mark_reference(GAP)
    t = sim.rearrangement_times()
    assert t[0] == 1 and t[1] > 0.0
    sim.set_state(pos=pos1)
    st1 = sim.get_state()
    want, _ = check(sim, 0, st0, st1, GAP, "first mark")
    assert sim.rearrangement_times()[0] == 3  # the row and the per-bot call of check
    assert sim.reference_info() == {"marked": True, "gap": float(f32(GAP)), "time": 1.25,
                                    "entries": want["bonds_marked"]}
    with pytest.raises(RuntimeError, match="linkGap"):
        sim.mark_reference(-1.0)
    # a mark at another gap, of the state as it is now, replaces the first
    sim.time = 2.5
    sim.mark_reference(0.3)
    sim.set_state(pos=pos)
    wide, wbots = check(sim, 0, st1, st0, 0.3, "second mark")
    assert wide["bonds_marked"] > 4 * want["bonds_now"] and int(wbots["marked"].max()) > 8
    assert sim.reference_info() == {"marked": True, "gap": float(f32(0.3)), "time": 2.5, "entries": wide["bonds_marked"]}
    assert sim.rearrangement_times()[0] == 6
    sim.clear_reference()
    assert sim.reference_info() == none
    for call in (sim.rearrangement, sim.rearrangement_of):
        with pytest.raises(RuntimeError, match="code 2.*no reference marked"):
            call()
    assert sim.rearrangement_times()[0] == 6
    sim.clear_reference()  # nothing to clear: fine
    sim.mark_reference(GAP)
    check(sim, 0, st0, st0, GAP, "marked again")


# ---- consistency with the cluster analysis -----------------------------------------------------------------------------------

def test_marked_and_now_are_the_cluster_analysis_degrees(pb, orc):
    n = 1025
    pos, vel, rad, pos1 = recipe(n)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    deg0 = sim.cluster_labels(GAP)[1]
    sim.mark_reference(GAP)
    sim.set_state(pos=pos1)
    got = sim.rearrangement_of()
    deg1 = sim.cluster_labels(GAP)[1]
    assert np.array_equal(got["marked"], deg0) and np.array_equal(got["now"], deg1)
    assert not np.array_equal(deg0, deg1)
    again = sim.rearrangement_of()  # the cluster analysis in between shares the scratch and leaves the mark alone
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k


# ---- the runner ----------------------------------------------------------------------------------------------------------

HEADER = ("Time, MarkTime, BondsMarked, BondsNow, BondsKept, Unchanged, Lost, Gained, Measured, SumQx, SumQy, SumQ2, "
          "MaxQ2")


@pytest.mark.parametrize("window", [False, True])
def test_runner_writes_rearrangement_rows(tmp_path, window):
    from particlerobotsimulations_amd import host
    cfg = os.path.join(ROOT, "examples", "example.cfg")
    over = dict(max_time="3", dump_interval="1")
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    flags = ["--rearrange", "a.csv", "--rearrange-gap", str(GAP)] + (["--rearrange-window"] if window else [])
    r = subprocess.run([RUN, cfg, "--quiet"] + sets + flags, capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "a.csv").read().splitlines()
    assert lines[0] == HEADER
    main_times = [l.split(",")[0] for l in open(tmp_path / "example_data.csv").read().splitlines()[2:]]
    cells = [[c.strip() for c in l.split(",")] for l in lines[1:]]
    assert [c[0] for c in cells] == main_times and len(main_times) >= 4
    first = cells[0]
    assert first[2] == first[3] == first[4] and int(first[2]) > 0 and first[5] == first[8]
    assert first[6] == first[7] == "0" and first[9:] == ["0", "0", "0", "0"]
    if window:
        assert [c[1] for c in cells[1:]] == [c[0] for c in cells[:-1]]  # MarkTime advances with the rows
    else:
        assert all(c[1] == cells[0][0] for c in cells)
    assert any(int(c[11]) > 0 for c in cells[1:]), "nothing moved in any row"
    # the same rows from the class driven by hand
    flat = host.load_config(cfg, **over)
    h = host.HostSim(cfg, engine="fused", **over)
    di = f32(flat.dump_interval)

    def due(t):  # the gate of dumpParticlebot, in its fp32 operations
        t = f32(t)
        return not (t - di * np.floor(t / di) > f32(0.01))

    want, mark_time = [], None
    while True:
        if due(h.time):
            if mark_time is None:
                h.mark_reference(GAP)
                mark_time = h.time
            s = h.rearrangement()[0]
            want.append("%f, %f, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d" % (
                h.time, mark_time, s["bonds_marked"], s["bonds_now"], s["bonds_kept"], s["bots_unchanged"],
                s["bots_lost"], s["bots_gained"], s["measured"], s["sum_qx"], s["sum_qy"], s["sum_q2"], s["max_q2"]))
            if window:
                h.mark_reference(GAP)
                mark_time = h.time
        if h.finished:
            break
        if h.advance(h.steps_until_dump()) == 0:
            break
    print(want)
    assert lines[1:] == want
