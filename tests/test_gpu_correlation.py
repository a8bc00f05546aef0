"""GPU: the pair correlations (pbSimPairCorrelation, csrc/pb_correlate.hip) against tests/correlation_ref.py on the state
read back from the device.  Every comparison is exact: the rows are compared byte for byte with the reference's
normalised 128-bit integers, the totals as Python ints.  tests/test_correlation_api.py pins the reference to known
answers on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import cluster_ref as CR
import correlation_ref as KR
from helpers import assert_bit_equal, jittered_blob, simparams_from_orc
from test_contacts_api import state_700

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
f32 = np.float32
GAP = 0.0019
RB = [(0.6, 64), (3.0, 7)]  # (rMax, bins); 3.0 covers a whole small blob on a folding grid
KINDS = ("velocity", "displacement", "radius")


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


def check(sim, member, kind, r_max, bins, st, what, pos0=None, got=None):
    """One member's rows and totals against the reference on the state `st` (and the marked positions); returns the
    reference."""
    from particlerobotsimulations_amd import _capi
    ref = KR.pair_correlation(kind, st["pos"], st["vel"], st["rad"], r_max, bins, pos0)
    rows, totals = sim.pair_correlation(kind, r_max, bins) if got is None else got
    assert rows.dtype == _capi.CORRELATION_BIN_DTYPE and rows.shape[1:] == (bins,)
    want = KR.rows_of(ref, rows.dtype)
    print(what, kind, "rMax", r_max, "bins", bins, ref["totals"])
    bad = np.flatnonzero(rows[member] != want)
    assert rows[member].tobytes() == want.tobytes(), (what, kind, r_max, bins, bad[:8], rows[member][bad[:2]], want[bad[:2]])
    assert totals[member] == ref["totals"], (what, kind, totals[member], ref["totals"])
    assert not (rows[member]["pairs"] & np.uint64(1)).any()
    return ref


def non_trivial(ref, n, negative=True):
    assert sum(ref["pairs"]) > n, "a trivial case"
    assert any(KR.normalised(v)[1] != 0 for v in ref["dot"]), "no dot beyond 32 bits"
    if negative:
        assert min(ref["dot"]) < 0, "no negative dot"


# ---- sizes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_around_the_wave_and_the_workgroup(pb, orc, n):
    pos, vel, rad = jittered_blob(n, 0.15, np.random.default_rng(1000 + n), jitter=0.3)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    with pytest.raises(RuntimeError, match="no reference marked"):
        sim.pair_correlation("displacement", 0.6, 64)
    st0 = sim.get_state()
    for kind in ("velocity", "radius"):
        for r_max, bins in RB:
            ref = check(sim, 0, kind, r_max, bins, st0, f"n {n}")
            if r_max == 3.0 and n <= 65:  # the blob is smaller than rMax: every ordered pair is counted, once
                assert sum(ref["pairs"]) == n * (n - 1)
            if n >= 63:
                non_trivial(ref, n, negative=kind == "velocity")
    sim.mark_reference(GAP)
    assert sim.step(120, dt=0.01, sort_interval=0.5) == 120
    st1 = sim.get_state()
    assert not np.array_equal(st1["pos"], st0["pos"])
    for kind in KINDS:
        for r_max, bins in RB:
            ref = check(sim, 0, kind, r_max, bins, st1, f"n {n} stepped", pos0=st0["pos"])
            if n >= 63:
                non_trivial(ref, n, negative=False)
    sim.clear_reference()
    with pytest.raises(RuntimeError, match="no reference marked"):
        sim.pair_correlation(1, 0.6, 64)
    check(sim, 0, 0, 0.6, 64, st1, f"n {n} after the clear")


# ---- bin limits ----------------------------------------------------------------------------------------------------------

def test_bin_limits_on_one_blob(pb, orc):
    n = 300
    pos, vel, rad = jittered_blob(n, 0.15, np.random.default_rng(7), jitter=0.3)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st = sim.get_state()
    for bins in (1, 1024):
        for r_max in (0.05, 100.0):
            for kind in ("velocity", "radius"):
                ref = check(sim, 0, kind, r_max, bins, st, "limits")
                if r_max == 100.0:
                    assert sum(ref["pairs"]) == n * (n - 1)
                else:
                    assert sum(ref["pairs"]) < n  # almost nothing is closer than 0.05
    ref = check(sim, 0, "velocity", 100.0, 1, st, "one bin")
    t = ref["totals"]
    assert ref["dot"] == [t["sum_ax"] ** 2 + t["sum_ay"] ** 2 - t["sum_a2"]] and ref["ax"] == [(n - 1) * t["sum_ax"]]
    non_trivial(check(sim, 0, "velocity", 3.0, 1024, st, "1024 bins"), n)
    with pytest.raises(RuntimeError, match="bins must be 1 ... 1024"):
        sim.pair_correlation("velocity", 1.0, 1025)
    with pytest.raises(RuntimeError, match="unknown kind"):
        sim.pair_correlation(3, 1.0, 8)


# ---- extremes ------------------------------------------------------------------------------------------------------------

def test_velocities_at_the_end_of_the_fixed_point(pb, orc):
    n = 64
    rng = np.random.default_rng(64)
    pos, _, rad = jittered_blob(n, 0.15, rng, jitter=0.3)
    vel = (f32(2047.9) * rng.choice([-1.0, 1.0], size=(n, 2))).astype(f32)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st = sim.get_state()
    assert_bit_equal(st["vel"], vel, "vel")
    for r_max, bins in RB + [(100.0, 1)]:
        ref = check(sim, 0, "velocity", r_max, bins, st, "extreme velocities")
        non_trivial(ref, n, negative=bins > 1)  # (the one bin holds |sum a|^2 - sum_a2, of either sign)
        assert max(abs(v) for v in ref["dot"]) > 1 << 64
    assert ref["totals"]["sum_a2"] > 1 << 68  # 128 terms of almost 2^62

    vel = (rng.standard_normal((n, 2)) * 0.02).astype(f32)
    vel[3] = (np.nan, 0.0)
    vel[4] = (0.0, np.inf)
    vel[5] = (2048.0, 0.0)
    vel[6] = (0.0, -2048.0)
    vel[7] = (-np.inf, np.nan)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st = sim.get_state()
    for r_max, bins in RB:
        ref = check(sim, 0, "velocity", r_max, bins, st, "unmeasured velocities")
        assert ref["totals"]["measured"] == n - 5
        assert check(sim, 0, "radius", r_max, bins, st, "unmeasured velocities")["totals"]["measured"] == n
    non_trivial(ref, n)
    assert ref["totals"]["pairs"] == (n - 5) * (n - 6)
    assert np.array_equal(sim.radial_counts(3.0, 7)[0], KR.pair_correlation("radius", pos, vel, rad, 3.0, 7)["pairs"])


def test_non_finite_positions_and_radii(pb, orc):
    n = 70
    rng = np.random.default_rng(70)
    pos, vel, rad = jittered_blob(n, 0.15, rng, jitter=0.3)
    pos[2] = (np.nan, 0.0)
    pos[9] = (0.0, np.inf)
    rad[20] = np.inf
    rad[21] = np.nan
    rad[22] = 2048.0  # a node, and measured by every kind but the radius
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st = sim.get_state()
    for r_max, bins in RB:
        ref = check(sim, 0, "velocity", r_max, bins, st, "non-finite")
        assert ref["totals"]["measured"] == n - 4
        assert ref["pairs"] == sim.radial_counts(r_max, bins)[0].tolist()
        assert check(sim, 0, "radius", r_max, bins, st, "non-finite")["totals"]["measured"] == n - 5
    non_trivial(ref, n)
    pos = np.array([[0.0, 0.0], [np.nan, 0.0], [0.05, 0.0], [0.0, np.inf]], f32)  # one node: no pair at all
    sim = sim_with(pb, orc, pos, np.array([0.1, 0.1, np.inf, 0.1], f32), vel=np.ones((4, 2), f32))
    rows, totals = sim.pair_correlation("velocity", 10.0, 16)
    assert not rows.view(np.uint8).any()
    assert totals == [{"measured": 1, "sum_ax": 1 << 20, "sum_ay": 1 << 20, "sum_a2": 1 << 41, "pairs": 0}]


def test_pile_of_coincident_bots(pb, orc):
    n = 2000
    rng = np.random.default_rng(2000)
    pos = np.tile(np.array([[3.0, -2.0]], f32), (n, 1))
    rad = rng.uniform(0.0775, 0.1175, n).astype(f32)
    vel = rng.uniform(-2000.0, 2000.0, (n, 2)).astype(f32)
    sim = sim_with(pb, orc, pos, rad, vel=vel)
    st = sim.get_state()
    ref = check(sim, 0, "velocity", 1.0, 8, st, "pile")
    assert ref["pairs"] == [n * (n - 1)] + [0] * 7  # every pair in bin 0: the LDS atomics of one address
    t = ref["totals"]
    assert ref["dot"][0] == t["sum_ax"] ** 2 + t["sum_ay"] ** 2 - t["sum_a2"] and abs(ref["dot"][0]) > 1 << 64
    check(sim, 0, "radius", 1.0, 8, st, "pile")


def test_payload_bot_is_an_ordinary_node(pb, orc):
    n = 201
    pos, vel, rad = jittered_blob(n, 0.2, np.random.default_rng(21), jitter=0.3)
    pos[n - 1] = pos[100] + np.array([0.1, 0.05], f32)  # the payload in the middle of the blob, twice as large
    rad[n - 1] = 0.2
    sim = sim_with(pb, orc, pos, rad, vel=vel, wall_half=64.0, nDead=-1, radFactor=2.0, attractionFactor=0.5)
    assert sim.config()["payload"] == 1
    st = sim.get_state()
    for r_max, bins in RB:
        ref = check(sim, 0, "velocity", r_max, bins, st, "payload")
        assert ref["totals"]["measured"] == n
        check(sim, 0, "radius", r_max, bins, st, "payload")
    non_trivial(ref, n)


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
    ens.mark_reference(GAP)
    marked = [ens.get_state_of(k)["pos"] for k in range(members)]
    assert ens.step(120, dt=0.01, sort_interval=0.5) == 120  # slots leave original order, the cell lists are stale
    assert ens.stats()["resorts"] >= 2
    st3 = ens.get_state_of(3)
    ens.set_state_of(4, pos=st3["pos"], vel=st3["vel"], rad=st3["rad"], phase=st3["phase"], dead=st3["dead"])
    got = {(kind, rb): ens.pair_correlation(kind, *rb) for kind in KINDS for rb in RB}
    counts = {rb: ens.radial_counts(*rb) for rb in RB}
    for k in range(members):
        st = ens.get_state_of(k)
        for kind in KINDS:
            for rb in RB:
                rows, totals = got[kind, rb]
                assert rows.shape == (members, rb[1]) and len(totals) == members
                ref = check(ens, k, kind, rb[0], rb[1], st, f"member {k}", pos0=marked[k], got=got[kind, rb])
                non_trivial(ref, n, negative=kind == "velocity")
                one = ens.pair_correlation(kind, rb[0], rb[1], member=k)
                assert one[0].tobytes() == rows[k].tobytes() and one[1] == totals[k]
                assert np.array_equal(rows[k]["pairs"], counts[rb][k])  # every bot is measured
    for kind in ("velocity", "radius"):  # (member 4's mark is its own)
        for rb in RB:
            rows, totals = got[kind, rb]
            assert rows[3].tobytes() == rows[4].tobytes() and totals[3] == totals[4]


# ---- nothing changes, repeatability -----------------------------------------------------------------------------------------

def test_nothing_changes_and_the_shared_scratch_stays_valid(pb, orc):
    pos, vel, rad = state_700()
    n = rad.size
    P = orc.default_params(nCells=n, nDead=0, seed=3, max_time=1e9)
    sp, keep = simparams_from_orc(P)
    sim = pb.Sim(sp, wall_half=64.0, keepalive=keep)
    sim.set_state(pos=pos, vel=vel, rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    sim.mark_reference(GAP)
    assert sim.step(30, dt=0.01, sort_interval=0.1) == 30

    def others():
        c = sim.contacts(GAP)
        return ({k: sim.clusters(GAP)[0][k] for k in CR.FIELDS}, c["offsets"].tobytes(), c["other"].tobytes(), c["gap"].tobytes(),
                sim.radial_counts(0.6, 64).tobytes(), sim.structure(GAP), sim.rearrangement())

    before, stats, mark = sim.get_state(), sim.stats(), sim.reference_info()
    assert mark["marked"]
    was = others()
    assert sim.correlation_times() == (0, 0.0)
    first = {kind: sim.pair_correlation(kind, 0.6, 64) for kind in KINDS}
    t = sim.correlation_times()
    assert t[0] == 3 and t[1] > 0.0
    for kind in KINDS:
        non_trivial(check(sim, 0, kind, 0.6, 64, before, "700 bots", pos0=pos, got=first[kind]), n,
                    negative=kind == "velocity")
    # the other analyses after the correlations (the scratch is shared), and the other way round
    assert others() == was
    assert {k: sim.clusters(GAP)[0][k] for k in CR.FIELDS} == CR.analyse(before["pos"], before["rad"], GAP)[0]
    for kind in KINDS:
        again = sim.pair_correlation(kind, 0.6, 64)
        assert again[0].tobytes() == first[kind][0].tobytes() and again[1] == first[kind][1]
        twice = sim.pair_correlation(kind, 0.6, 64)
        assert twice[0].tobytes() == again[0].tobytes() and twice[1] == again[1]
    assert sim.correlation_times()[0] == 9
    assert others() == was
    after = sim.get_state()
    for name in before:
        assert_bit_equal(after[name], before[name], name)
    assert sim.stats() == stats and sim.reference_info() == mark
    # C(r) from the device's integers: the mean is taken out, and C0 is the variance of a
    c, ratio = pb.connected_correlation(*sim.pair_correlation("velocity", 0.6, 64, member=0))
    assert np.isfinite(c).sum() > 32 and np.array_equal(np.isfinite(c), np.isfinite(ratio))


# ---- the runner ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["velocity", "radius"])
def test_runner_writes_the_final_correlations(tmp_path, kind):
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import host
    cfg = os.path.join(ROOT, "examples", "example.cfg")
    over = dict(max_time="3")
    sets = [a for k, v in over.items() for a in ("--set", k, v)]
    flags = ["--correlate", "k.csv"] + ([] if kind == "velocity" else ["--correlate-kind", kind])
    r = subprocess.run([RUN, cfg, "--quiet"] + sets + flags, capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = open(tmp_path / "k.csv").read().splitlines()
    flat = host.load_config(cfg, **over)
    h = host.HostSim(cfg, engine="fused", **over)
    while not h.finished:
        if h.advance(h.steps_until_dump()) == 0:
            break
    r_max = f32(10.0) * f32(flat.max_radius)
    rows, t = h.pair_correlation(kind, r_max, 200, member=0)
    v = pb.correlation_values(rows)
    assert t["measured"] == h.n and t["pairs"] > h.n and t["pairs"] == sum(v["pairs"])
    assert lines[0] == "Kind, %s, Measured, %d, SumAx, %d, SumAy, %d, SumA2, %d, Pairs, %d" % (
        kind, t["measured"], t["sum_ax"], t["sum_ay"], t["sum_a2"], t["pairs"])
    assert lines[1] == "RLo, RHi, Pairs, Dot, SumAx, SumAy" and len(lines) == 202
    for b, line in enumerate(lines[2:]):
        assert line == "%.9g, %.9g, %d, %d, %d, %d" % (b * float(r_max) / 200.0, (b + 1) * float(r_max) / 200.0,
                                                       v["pairs"][b], v["dot"][b], v["ax"][b], v["ay"][b]), b
    assert any(v["dot"]) and (kind == "velocity" or any(d >= 1 << 32 for d in v["dot"]))
