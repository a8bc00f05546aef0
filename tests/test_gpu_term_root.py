"""The both-sums throughput form (one bot per lane, pbSimSetForceSums mode 1) roots every pair term once, in the trip
that evaluates it: the root that used to serve the attraction magnitudes only now serves the contact lanes too, and
the LDS list of pending contact magnitudes is gone from that form (pb_device.hpp pbPairEvalXY<FAST, true, true>).  A
contact term is not bounded like an attraction term, so the cases below put a zero, a denormal-range, an overflowing
and a NaN squared magnitude into contact lanes, restore odd running sums, and crowd more contacts onto a lane than the
list ever held.  Everything is compared with the oracle bit for bit (NaN positions must match, payloads are not
compared), for the branch-free kernel with and without the fast exact forms (force variants 1 and 2)."""
import numpy as np
import pytest

from helpers import assert_bit_equal, jittered_blob, simparams_from_orc

pytestmark = pytest.mark.gpu

KEYS = ("pos", "vel", "rad", "absForce_r", "absForce_a")
STEPS = (1, 2, 5)  # one step is an un-fused launch, the longer calls fuse the next step's radius + integration


@pytest.fixture(scope="module")
def orc():
    from oracle import orclib
    return orclib


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def build(pb, orc, P, state, variant, forces=None):
    """As tests/test_gpu_dead_sum.py::build, always with both sums kept; `forces`: (absForce_a, absForce_r) restored
    into both simulations before the first step."""
    osim = orc.Sim(P, reset=True)
    sp, keep = simparams_from_orc(P)
    gsim = pb.Sim(sp, keepalive=keep)
    gsim.set_lanes_per_bot(1)
    gsim.set_force_variant(variant)
    gsim.set_force_sums(1)
    full = dict(pos=osim.get("pos"), vel=osim.get("vel"), rad=osim.get("rad"), phase=osim.get("phase"),
                dead=osim.get("dead"))
    full.update(state)
    for k, v in full.items():
        osim.set(k, v)
    gsim.set_state(**full)
    if forces is not None:
        osim.set("absForce_a", forces[0])
        osim.set("absForce_r", forces[1])
        gsim.set_forces(forces[0], forces[1])
    cfg = gsim.config()
    assert cfg["lanes_per_bot"] == 1 and cfg["attraction_sums"] == 1 and cfg["dead_sum_form"] == 0, cfg
    return osim, gsim


def check(osim, gsim, what):
    st = gsim.get_state()
    for key in KEYS:
        a, b = st[key], osim.get(key)
        assert (np.isnan(a) == np.isnan(b)).all(), f"{what}: {key}: NaN positions differ"
        both = np.isnan(a) & np.isnan(b)
        assert_bit_equal(np.where(both, 0, a).astype(a.dtype), np.where(both, 0, b).astype(b.dtype), f"{what}: {key}")


def run_and_check(osim, gsim, what, steps=STEPS, after=None):
    step = 0
    for upto in steps:
        osim.run(upto - step)
        assert gsim.step(upto - step) == upto - step
        step = upto
        check(osim, gsim, f"{what}, step {upto}")
        if after is not None:
            after(upto)


def blob_state(n, seed, **kw):
    rng = np.random.default_rng(seed)
    pos, vel, rad = jittered_blob(n, 0.158, rng, center=(0.3, -0.2), jitter=0.12, **kw)
    return dict(pos=pos, vel=vel, rad=rad)


def overlapping_pairs(pos, rad):
    d = np.linalg.norm(pos[:, None, :].astype(np.float64) - pos[None, :, :], axis=2)
    reach = rad[:, None].astype(np.float64) + rad[None, :]
    np.fill_diagonal(d, np.inf)
    return int((d < reach - 1e-3).sum()) // 2


@pytest.mark.parametrize("variant", [1, 2])
def test_zero_contact_term(pb, orc, variant):
    """Overlapping bots at rest, spring constant 0: the contact term is (0, 0) and its squared magnitude 0 -- where the
    unclamped one-step root is NaN.  absForce_r of step 1 is exactly 0 for every bot, and nothing is NaN."""
    n = 1500
    P = orc.default_params(nCells=n, nDead=0, seed=31, phase_std=0.0, max_time=1e9, light_x=-3.0, light_y=0.5,
                           spring=0.0)
    s = blob_state(n, 5)
    s["vel"][...] = 0.0
    assert overlapping_pairs(s["pos"], s["rad"]) > n // 4
    osim, gsim = build(pb, orc, P, s, variant)
    assert gsim.config()["force_kind"] == variant  # (variant 2: the fast exact forms really ran)

    def after(upto):
        for key in KEYS:
            assert not np.isnan(osim.get(key)).any(), (key, upto)
        if upto == 1:
            assert (osim.get("absForce_r") == 0.0).all() and (osim.get("absForce_a") > 0.0).any()

    run_and_check(osim, gsim, f"zero contact term, variant {variant}", after=after)


@pytest.mark.parametrize("variant", [1, 2])
def test_tiny_contact_term(pb, orc, variant):
    """Spring 1e-15, no dashpot, no shear: a contact term is ~1e-16 x overlap, its squared magnitude lies in
    (0, 2^-96), below the one-step root's domain: the wave has to take sqrtf."""
    n = 1500
    P = orc.default_params(nCells=n, nDead=0, seed=32, phase_std=0.0, max_time=1e9, light_x=-3.0, light_y=0.5,
                           spring=1e-15, damping=0.0, shear=0.0)
    s = blob_state(n, 6)
    s["vel"][...] = 0.0
    assert overlapping_pairs(s["pos"], s["rad"]) > n // 4
    osim, gsim = build(pb, orc, P, s, variant)
    assert gsim.config()["force_kind"] == variant

    def after(upto):
        r = osim.get("absForce_r")
        assert not np.isnan(r).any()
        # every contact magnitude is below 2^-48 (a bot has fewer than 64 contacts), and there are contacts
        assert (r > 0.0).sum() > n // 4 and r.max() < 64 * 2.0 ** -48, (upto, r.max())

    run_and_check(osim, gsim, f"tiny contact term, variant {variant}", after=after)


@pytest.mark.parametrize("variant", [1, 2])
def test_overflowing_contact_term(pb, orc, variant):
    """Eight bots with velocities of 1e22 ... 8e22 end the step's integration clamped into the same corner of the
    arena, in contact with each other at relative velocities whose dashpot term squares to +inf.  One un-fused step."""
    n = 1500
    P = orc.default_params(nCells=n, nDead=0, seed=33, phase_std=0.0, max_time=1e9, light_x=-3.0, light_y=0.5)
    s = blob_state(n, 7)
    for k in range(8):  # (sorted into the corner's cells already: the cell lists are those of the initial positions)
        s["pos"][100 + k] = (63.6 + 0.02 * k, 63.7)
        s["vel"][100 + k] = (1e22 * (k + 1), 1e22 * (k + 1))
    osim, gsim = build(pb, orc, P, s, variant)
    run_and_check(osim, gsim, f"overflowing contact term, variant {variant}", steps=(1,))
    r = osim.get("absForce_r")
    assert np.isposinf(r[100:108]).sum() >= 2, r[100:108]
    assert np.isfinite(np.delete(r, np.arange(100, 108))).all()


@pytest.mark.parametrize("variant", [1, 2])
def test_restored_sums(pb, orc, variant):
    """absForce_a / absForce_r restored with -1, -0.0, NaN and inf entries: Sum|F_rep| starts as 0.0f * absForce_r,
    that is -0, NaN or NaN, and a bot without contacts must keep exactly that value (the sums are accumulated by
    select, never by adding +0)."""
    n = 1500
    P = orc.default_params(nCells=n, nDead=0, seed=34, phase_std=0.0, max_time=1e9, light_x=-3.0, light_y=0.5)
    s = blob_state(n, 8)
    lone = np.arange(64)  # a sparse lattice, 1.5 apart and away from the blob: bots without contacts
    s["pos"][lone, 0] = 20.0 + 1.5 * (lone % 8)
    s["pos"][lone, 1] = 20.0 + 1.5 * (lone // 8)
    s["vel"][lone] = 0.0
    odd = np.array([-1.0, -0.0, np.nan, np.inf, 0.0, 3.5, -np.inf, 1e-40], np.float32)
    fa = odd[np.arange(n) % 8].copy()
    fr = odd[(np.arange(n) // 8 + np.arange(n)) % 8].copy()  # every pairing of the two arrays' values
    osim, gsim = build(pb, orc, P, s, variant, forces=(fa, fr))

    def after(upto):
        if upto == 1:
            r = osim.get("absForce_r")[lone]
            with np.errstate(invalid="ignore"):
                want = np.float32(0.0) * fr[lone]
            assert (np.isnan(r) == np.isnan(want)).all()
            assert (np.signbit(r) == np.signbit(want))[~np.isnan(want)].all() and np.signbit(r).any()

    run_and_check(osim, gsim, f"restored sums, variant {variant}", after=after)


def crowded_state(n):
    s = blob_state(n, 9)
    rng = np.random.default_rng(90)
    for c in range(20):
        at = int(rng.integers(0, n - 40))
        s["pos"][at:at + 30] = s["pos"][at] + rng.uniform(-0.02, 0.02, size=(30, 2)).astype(np.float32)
    return s


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("payload", [0, 1])
def test_mixed_waves_and_crowded_lanes(pb, orc, payload, variant):
    """A jittered blob (lanes in contact, in both near bands and far in the same trip) with clusters of 30 nearly
    coincident bots: 29 contacts per lane, far more than the pending list of 8 the form used to flush in mid-sweep.
    The order of the additions to Sum|F_rep| must be the list's."""
    n = 4096
    kw = dict(nDead=-1, attractionFactor=0.5, massFactor=2.0) if payload else dict(nDead=0)
    P = orc.default_params(nCells=n, seed=35, phase_std=0.0, max_time=1e9, light_x=3.0, light_y=1.0, **kw)
    osim, gsim = build(pb, orc, P, crowded_state(n), variant)
    assert gsim.config()["payload"] == payload
    run_and_check(osim, gsim, f"mixed waves, payload {payload}, variant {variant}")


@pytest.mark.parametrize("variant", [1, 2])
def test_mixed_waves_through_the_64bit_offset_form(pb, orc, variant, monkeypatch):
    monkeypatch.setenv("PB_ALLOW_ENV_OVERRIDES", "1")
    monkeypatch.setenv("PB_DEBUG_FORCE_BIG", "1")
    n = 4096
    P = orc.default_params(nCells=n, nDead=0, seed=36, phase_std=0.0, max_time=1e9, light_x=3.0, light_y=1.0)
    osim, gsim = build(pb, orc, P, crowded_state(n), variant)
    assert gsim.config()["offsets64"] == 1
    run_and_check(osim, gsim, f"mixed waves, 64-bit offsets, variant {variant}")


def test_term_root_equals_sqrtf_or_is_guarded_on_every_bit_pattern(pb):
    """pbSelfTestTermRoot: all 2^32 bit patterns; outside the guard's set the clamped one-step root is sqrtf."""
    r = pb.self_test_term_root()
    assert r["checked"] == 1 << 32 and r["mismatches"] == 0, r
