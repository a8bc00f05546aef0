"""GPU: the contact export (pbSimContactsOf / pbSimContactVirialOf, csrc/pb_contacts.hip) against tests/contacts_ref.py on
the state read back from the device.  Every comparison is exact: offsets and `other` as integers, gap, force and virial
as bit patterns; where the reference's force is non-finite (coincident bots) the device's must be non-finite too.
tests/test_contacts_api.py pins the reference on the CPU and shows that the 700-bot state holds all four regimes of the
pair law."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contacts_ref as KR
from helpers import assert_bit_equal, jittered_blob, simparams_from_orc
from test_contacts_api import cfg_path, regimes, state_700

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
f32 = np.float32


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def state_of(sim, member):
    return sim.get_state_of(member) if hasattr(sim, "nsims") else sim.get_state()


def assert_same_floats(got, want, what):
    """Bit for bit where the reference is finite; non-finite where it is not."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert not np.isfinite(got[~fin]).any(), (what, "finite where the reference is not")
    as_int = np.uint32 if got.dtype == np.float32 else np.uint64
    a, b = got[fin].view(as_int), want[fin].view(as_int)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        raise AssertionError(f"{what}: {bad.size}/{a.size} finite elements differ; first {got[fin][bad[0]]!r} vs "
                             f"{want[fin][bad[0]]!r}")


def check_member(sim, orc, P, member, gap, what):
    """contacts() and contact_virial() of one member against the reference on the state read back; returns the
    reference."""
    st = state_of(sim, member)
    want = KR.network(orc, P, st["pos"], st["vel"], st["rad"], gap)
    got = sim.contacts(gap, member=member)
    print(what, gap, "entries", got["other"].size)
    assert got["offsets"].dtype == np.uint32 and got["other"].dtype == np.uint32
    assert np.array_equal(got["offsets"], want["offsets"]), (what, gap, "offsets")
    assert np.array_equal(got["other"], want["other"]), (what, gap, "other")
    assert_bit_equal(got["gap"], want["gap"], f"{what} {gap} gap")
    assert_same_floats(got["force"], want["force"], f"{what} {gap} force")
    vir = sim.contact_virial(gap, member=member)
    assert vir.dtype == np.float64 and vir.shape == (sim.n, 4)
    assert_same_floats(vir, want["virial"], f"{what} {gap} virial")
    return want


def sim_with(pb, orc, pos, rad, vel=None, wall_half=4.0e6, **over):
    pos = np.asarray(pos, f32).reshape(-1, 2)
    n = pos.shape[0]
    over.setdefault("nDead", 0)
    P = orc.default_params(nCells=n, seed=3, max_time=1e9, **over)
    sp, keep = simparams_from_orc(P)
    sim = pb.Sim(sp, wall_half=wall_half, keepalive=keep)
    sim.set_state(pos=pos, vel=np.zeros((n, 2), f32) if vel is None else vel, rad=np.asarray(rad, f32),
                  phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    return sim, P


# ---- one member --------------------------------------------------------------------------------------------------------

def test_one_member_all_regimes_and_nothing_changes(pb, orc):
    pos, vel, rad = state_700()
    sim, P = sim_with(pb, orc, pos, rad, vel=vel, wall_half=64.0)
    before, stats = sim.get_state(), sim.stats()
    assert sim.contact_times() == (0, 0.0)
    for gap in (0.0, 0.0019, 0.05):
        want = check_member(sim, orc, P, 0, gap, "700 bots")
        deg = sim.cluster_labels(gap)[1]
        assert np.array_equal(np.diff(sim.contacts(gap)["offsets"].astype(np.int64)), deg)
    seen = regimes(want["gap"])
    assert all(v > 0 for v in seen.values()), seen
    after = sim.get_state()
    for name in before:
        assert_bit_equal(after[name], before[name], name)
    assert sim.stats() == stats
    exports, ms = sim.contact_times()
    assert exports >= 6 and ms > 0.0


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_around_a_wave_and_a_workgroup(pb, orc, n):
    pos, vel, rad = jittered_blob(n, 0.15, np.random.default_rng(n), jitter=0.3)
    sim, P = sim_with(pb, orc, pos, rad, vel=vel, wall_half=64.0)
    want = check_member(sim, orc, P, 0, 0.0019, f"n = {n}")
    if n == 1:
        got = sim.contacts(0.0019)
        assert got["other"].size == 0 and got["offsets"].tolist() == [0, 0]
    else:
        assert want["other"].size > 0


# ---- a batch -----------------------------------------------------------------------------------------------------------

def test_batch_each_member_with_its_own_parameters(pb, orc):
    members, n = 5, 300
    base = orc.default_params(nCells=n, nDead=0)
    rng = np.random.default_rng(11)
    Ps, plist, keeps = [], [], []
    for k in range(members):
        P = orc.default_params(nCells=n, nDead=0, seed=50 + k, max_time=1e9, phase_update_interval=0.3,
                               spring=base.spring * (1.0 + 0.25 * k), damping=base.damping * (1.0 + 0.1 * k),
                               shear=base.shear * (1.0 + 0.3 * k), attraction=base.attraction * (1.0 + 0.5 * k))
        sp, keep = simparams_from_orc(P)
        Ps.append(P)
        plist.append(sp)
        keeps.append(keep)
    ens = pb.Ensemble(plist, keepalive=keeps)
    for k in range(members):
        pos, vel, rad = jittered_blob(n, 0.2, rng, center=(0.3 * k, -0.2 * k), jitter=0.3)
        ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=rng.uniform(0, 6.28, n).astype(f32),
                         dead=np.zeros(n, np.int32))
    assert ens.step(120, dt=0.01, sort_interval=0.5) == 120  # slots leave original order, the cell lists go stale
    assert ens.stats()["resorts"] >= 2
    st = ens.get_state_of(1)  # members 1 and 2: the same state under different springs
    ens.set_state_of(2, pos=st["pos"], vel=st["vel"], rad=st["rad"], phase=st["phase"], dead=st["dead"])
    nets = [check_member(ens, orc, Ps[k], k, 0.0019, f"member {k}") for k in range(members)]
    a, b = ens.contacts(0.0019, member=1), ens.contacts(0.0019, member=2)
    assert np.array_equal(a["offsets"], b["offsets"]) and np.array_equal(a["other"], b["other"])
    assert_bit_equal(a["gap"], b["gap"], "gaps of the twin members")
    touching = a["gap"] < 0
    assert touching.any() and (a["force"][touching] != b["force"][touching]).any(axis=1).all()
    assert all(net["other"].size > 0 for net in nets)


# ---- payload mode ------------------------------------------------------------------------------------------------------

def test_payload_bot_carries_its_attraction_factor(pb, orc):
    n = 201
    pos, vel, rad = jittered_blob(n, 0.2, np.random.default_rng(21), jitter=0.3)
    pos[n - 1] = pos[100] + np.array([0.1, 0.05], f32)  # the payload in the middle of the blob, twice as large
    rad[n - 1] = 0.2
    sim, P = sim_with(pb, orc, pos, rad, vel=vel, wall_half=64.0, nDead=-1, radFactor=2.0, attractionFactor=0.5)
    assert sim.config()["payload"] == 1
    for gap in (0.0019, 0.15):
        want = check_member(sim, orc, P, 0, gap, "payload")
    mine = want["gap"][want["offsets"][n - 1]:want["offsets"][n]]
    assert (mine < 0).any() and (mine >= f32(0.0019)).any(), "the payload needs contacts and near-contacts"
    plain = orc.default_params(nCells=n, nDead=0, seed=3, max_time=1e9)  # the same law without the factor differs
    other = KR.network(orc, plain, pos, vel, rad, 0.15)
    assert np.array_equal(other["other"], want["other"]) and not np.array_equal(other["force"], want["force"])


# ---- long lists --------------------------------------------------------------------------------------------------------

def test_long_lists_stay_ordered(pb, orc):
    n = 300
    pos, vel, rad = jittered_blob(n, 0.2, np.random.default_rng(31), jitter=0.3)
    sim, P = sim_with(pb, orc, pos, rad, vel=vel, wall_half=64.0)
    want = check_member(sim, orc, P, 0, 0.5, "gap 0.5")
    got = sim.contacts(0.5)
    deg = np.diff(got["offsets"].astype(np.int64))
    assert deg.max() == sim.clusters(0.5)[0]["max_degree"] and deg.max() >= 30
    for i in range(n):
        mine = got["other"][got["offsets"][i]:got["offsets"][i + 1]].astype(np.int64)
        assert (np.diff(mine) > 0).all(), i


# ---- edge cases --------------------------------------------------------------------------------------------------------

def test_coincident_non_finite_and_tangent_bots(pb, orc):
    pos, rad = np.array([[3.0, -2.0]] * 2 + [[50.0, 50.0]], f32), np.full(3, 0.1, f32)
    sim, P = sim_with(pb, orc, pos, rad)
    check_member(sim, orc, P, 0, 0.0, "coincident")
    got = sim.contacts(0.0)
    assert got["offsets"].tolist() == [0, 1, 2, 2] and got["other"].tolist() == [1, 0]
    assert not np.isfinite(got["force"]).any()

    pos = np.array([[0.0, 0.0], [0.1, 0.0], [np.nan, 0.0], [0.05, 0.0], [0.0, np.inf]], f32)
    rad = np.array([0.1, 0.1, 0.1, np.inf, 0.1], f32)
    sim, P = sim_with(pb, orc, pos, rad)
    check_member(sim, orc, P, 0, 0.05, "non-finite")
    got = sim.contacts(0.05)
    assert got["offsets"].tolist() == [0, 1, 2, 2, 2, 2] and got["other"].tolist() == [1, 0]

    pos, rad = np.array([[0.0, 0.0], [0.1875, 0.0]], f32), np.array([0.09375, 0.09375], f32)
    sim, P = sim_with(pb, orc, pos, rad)
    check_member(sim, orc, P, 0, 0.0, "tangent")
    assert sim.contacts(0.0)["other"].size == 0
    check_member(sim, orc, P, 0, 1e-6, "tangent")
    got = sim.contacts(1e-6)
    assert got["other"].tolist() == [1, 0] and got["gap"].tolist() == [0.0, 0.0]
    assert got["force"].tolist() == [[2.5, 0.0], [-2.5, 0.0]]  # the first attraction regime: 2.5 along the unit vector


# ---- the cap protocol --------------------------------------------------------------------------------------------------

def test_cap_protocol_and_repeatability(pb, orc):
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    pos, vel, rad = jittered_blob(120, 0.2, np.random.default_rng(41), jitter=0.3)
    sim, P = sim_with(pb, orc, pos, rad, vel=vel, wall_half=64.0)
    count = C.c_ulonglong(0)
    assert L.pbSimContactsOf(sim._h, 0, 0.0019, None, None, 0, C.byref(count)) == 0
    E = int(count.value)
    assert E > 2
    small = np.full(E - 1, 0xA5A5A5A5, np.uint32).repeat(4).reshape(-1, 4).copy()
    count.value = 0
    assert L.pbSimContactsOf(sim._h, 0, 0.0019, None, _capi.np_ptr(small), E - 1, C.byref(count)) == 2
    assert b"pbSimContactsOf" in L.pbGetLastErrorString()
    assert count.value == E and (small == 0xA5A5A5A5).all()
    assert L.pbSimContactsOf(sim._h, 1, 0.0019, None, None, 0, C.byref(count)) == 2
    assert b"member" in L.pbGetLastErrorString()

    def fetch():
        off = np.zeros(121, np.uint32)
        links = np.full((E, 4), 0xA5A5A5A5, np.uint32)
        assert L.pbSimContactsOf(sim._h, 0, 0.0019, _capi.np_ptr(off), _capi.np_ptr(links), E, C.byref(count)) == 0
        assert count.value == E and off[-1] == E
        return off, links

    (o1, l1), (o2, l2) = fetch(), fetch()
    assert np.array_equal(o1, o2) and np.array_equal(l1, l2)
    got = sim.contacts(0.0019)
    assert np.array_equal(l1[:, 0], got["other"]) and np.array_equal(l1[:, 1], got["gap"].view(np.uint32))


# ---- the runner --------------------------------------------------------------------------------------------------------

def test_runner_writes_the_final_network(tmp_path):
    from particlerobotsimulations_amd import host
    cfg = cfg_path("example.cfg")
    out, csv = str(tmp_path / "contacts.csv"), str(tmp_path / "run.csv")
    r = subprocess.run([RUN, cfg, "--quiet", "--set", "csv_filename", csv, "--set", "max_time", "3", "--contacts", out,
                        "--contact-gap", "0.0019"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = open(out).read().splitlines()
    assert lines[0] == "I, J, Gap, Fx, Fy"
    rows = [l.split(", ") for l in lines[1:]]
    assert rows and all(len(row) == 5 for row in rows)
    h = host.HostSim(cfg, engine="fused", max_time="3")
    while not h.finished:
        if h.advance(h.steps_until_dump()) == 0:
            break
    want = h.contacts(0.0019)
    owner = np.repeat(np.arange(h.n), np.diff(want["offsets"].astype(np.int64)))
    assert [int(row[0]) for row in rows] == owner.tolist()
    assert [int(row[1]) for row in rows] == want["other"].tolist()
    for col, ref in ((2, want["gap"]), (3, want["force"][:, 0]), (4, want["force"][:, 1])):
        assert_same_floats(np.array([float(row[col]) for row in rows]).astype(f32), ref, f"column {col}")
