"""GPU: the reference's display kernels (updateCol, calcCOG) behind the `extern "C"` seam and in the resident engine,
bit for bit against the numpy restatements of tests/display_ref.py (fp32 compared as uint32).  The shadow bit comes
from the legacy updatePhase with light_shadow = 2 (pinned against the oracle by test_gpu_legacy.py): a shadowed bot's
phase is 9999999999.0f."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import display_ref as R
from helpers import assert_bit_equal, simparams_from_orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = ["example.cfg", "example_dead_cells.cfg", "example_gap.cfg", "example_object_transport.cfg",
            "example_obstacle.cfg"]
f32 = np.float32


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def obstacle_params(orc, n, display_shadow, payload=False, **kw):
    base = dict(nCells=n, nDead=-1 if payload else 0, seed=3, light_x=-5.0, light_y=0.3, light_shadow=2,
                display_shadow=display_shadow, n_cir_obstacles=2, x_cir_obs=[-1.0, 1.0], y_cir_obs=[0.5, -1.0],
                r_cir_obs=[0.5, 0.4], nobstacles=2, x1obs=[-2.2, 0.0], x2obs=[-2.0, 0.4], y1obs=[-3.0, 1.0],
                y2obs=[-0.5, 1.5], max_time=1e9)
    base.update(kw)
    return orc.default_params(**base)


def shadow_bits(pb, pos):
    """1 where the legacy updatePhase (light_shadow 2) marks the bot as shadowed."""
    n = pos.shape[0]
    dpos, dph = pb.DeviceArray.from_host(pos), pb.DeviceArray.from_host(np.zeros(n, np.float32))
    pb.legacy.update_phase(dpos, dph, 0.155, 0.0, 0.0, n)
    return dph.download() == np.float32(9999999999.0)


def random_state(rng, P, n):
    pos = rng.uniform(-4.0, 6.0, (n, 2)).astype(np.float32)
    rad = rng.uniform(P.min_radius, P.max_radius, n).astype(np.float32)
    rad[:3] = [P.min_radius, P.max_radius, np.float32((P.min_radius + P.max_radius) / 2)]
    dead = (rng.random(n) < 0.1).astype(np.int32)
    return pos, rad, dead


@pytest.mark.parametrize("display_shadow", [0, 1])
@pytest.mark.parametrize("payload", [False, True])
def test_update_col(pb, orc, display_shadow, payload):
    rng = np.random.default_rng(10 + display_shadow + 2 * payload)
    n, extra = 3000, 37
    P = obstacle_params(orc, n, display_shadow, payload)
    sp, keep = simparams_from_orc(P)
    pb.legacy.set_parameters(sp)
    pos, rad, dead = random_state(rng, P, n)
    if payload:
        rad[-1] = np.float32(P.min_radius * P.radFactor)
        dead[-1] = 1
    shadowed = shadow_bits(pb, pos)
    assert shadowed.any() and (~shadowed).any()
    col0 = rng.uniform(0, 1, (n + extra, 4)).astype(np.float32)
    dcol = pb.DeviceArray.from_host(col0)
    drad, dpos, ddead = map(pb.DeviceArray.from_host, (rad, pos, dead))
    pb.legacy.updateCol(drad.ptr, dcol.ptr, n, dpos.ptr, None, ddead.ptr)
    got = dcol.download()
    want = R.colours(rad, dead, shadowed, P.min_radius, P.max_radius, display_shadow, alpha=col0[:n, 3])
    assert_bit_equal(got[:n], want, "colour")
    assert_bit_equal(got[n:], col0[n:], "entries past n")
    if display_shadow:  # the tint was exercised
        live = (dead == 0) & shadowed
        plain = R.colours(rad[live][:50], dead[live][:50], np.zeros(50, bool), P.min_radius, P.max_radius, 0)
        assert not np.array_equal(want[live][:50], plain)
    del keep


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 4095, 4096, 4097, 262145, 1000000])
def test_calc_cog(pb, n):
    rng = np.random.default_rng(n)
    steps, interval = 7, f32(10.0)
    total = 2 * (n + steps + 1) + 64  # the reference's POSITION buffer plus a guard tail
    buf = rng.uniform(-50, 50, total).astype(np.float32)
    pos = buf[:2 * n].reshape(n, 2)
    pos[rng.random(n) < 0.05] = -0.0
    dpos = pb.DeviceArray.from_host(buf)
    t1, t2 = pb.DeviceArray(2 * n, fill=7.0), pb.DeviceArray(2 * n, fill=7.0)
    want = R.centroid(pos)
    for time in (0.0, 35.0, 69.99, 75.0):  # slot 0, a middle slot, steps - 1, a wrap
        ind = R.ring_slot(time, interval, steps)
        pb.legacy.calcCOG(dpos.ptr, t1.ptr, t2.ptr, n, float(time), steps, float(interval))
        got = dpos.download()
        exp = buf.copy()
        exp[2 * (ind + n):2 * (ind + n) + 2] = want
        assert_bit_equal(got, exp, f"calcCOG n={n} t={time}")
        buf = exp
    if n >= 65:  # one NaN poisons the centroid
        buf2 = buf.copy()
        buf2[2 * (n // 2)] = np.nan
        dpos.upload(buf2)
        pb.legacy.calcCOG(dpos.ptr, t1.ptr, t2.ptr, n, 10.0, steps, float(interval))
        got = dpos.download()
        assert np.isnan(got[2 * (1 + n)]) and got[2 * (1 + n) + 1] == R.centroid(buf2[:2 * n])[1]
        got[2 * (1 + n)] = buf2[2 * (1 + n)]
        got[2 * (1 + n) + 1] = buf2[2 * (1 + n) + 1]
        assert_bit_equal(got, buf2, "NaN case, elsewhere")
        buf = buf2
    dpos.upload(buf)
    for args in ((0, 5.0, steps, interval), (n, 5.0, 0, interval), (n, 5.0, steps, f32(0.0)),
                 (n, -25.0, steps, interval)):
        pb.legacy.calcCOG(dpos.ptr, t1.ptr, t2.ptr, args[0], float(args[1]), args[2], float(args[3]))
    assert_bit_equal(dpos.download(), buf, "degenerate arguments write nothing")


def test_engine_colours_member_one(pb, orc):
    rng = np.random.default_rng(4)
    n = 1500
    Ps = [obstacle_params(orc, n, 0), obstacle_params(orc, n, 1, light_x=-4.0)]
    sps = [simparams_from_orc(P) for P in Ps]
    E = pb.Ensemble([s for s, _ in sps])
    states = [random_state(rng, P, n) for P in Ps]
    for k, (pos, rad, dead) in enumerate(states):
        E.set_state_of(k, pos=pos, vel=np.zeros((n, 2), np.float32), rad=rad,
                       phase=np.zeros(n, np.float32), dead=dead)
    E.step(3)  # a re-sort: the slots are no longer in original order
    st = E.get_state_of(1)
    pb.legacy.set_parameters(sps[1][0])
    shadowed = shadow_bits(pb, st["pos"])
    want = R.colours(st["rad"], st["dead"], shadowed, Ps[1].min_radius, Ps[1].max_radius, 1)
    assert_bit_equal(E.colors(1), want, "engine colours, member 1")
    pb.legacy.set_parameters(sps[0][0])
    st0 = E.get_state_of(0)
    want0 = R.colours(st0["rad"], st0["dead"], shadow_bits(pb, st0["pos"]), Ps[0].min_radius, Ps[0].max_radius, 0)
    assert_bit_equal(E.colors(0), want0, "engine colours, member 0")


@pytest.mark.parametrize("cfg", EXAMPLES)
def test_engine_colours_equal_legacy_on_examples(cfg):
    from particlerobotsimulations_amd import host
    path = os.path.join(ROOT, "examples", cfg)
    a = host.HostSim(path, engine="fused", max_time="1e9", display_shadow="1")
    b = host.HostSim(path, engine="legacy", max_time="1e9", display_shadow="1")
    assert a.advance(300) == 300 and b.advance(300) == 300
    assert_bit_equal(a.get("pos"), b.get("pos"), cfg + " pos")
    ca, cb = a.get("col"), b.get("col")
    assert_bit_equal(ca, cb, cfg + " colours")
    assert (ca[:, 3] == 1).all() and (ca[:, 1] > 0).any()


def run_trail(engine, steps, resident=None, display=True):
    from particlerobotsimulations_amd import host
    if resident is not None:
        os.environ["PB_ALLOW_ENV_OVERRIDES"], os.environ["PB_RESIDENT"] = "1", str(resident)
    try:
        h = host.HostSim(os.path.join(ROOT, "examples", "example_obstacle.cfg"), engine=engine, reset=False,
                         max_time="1e9", centroid_int="1", centroid_steps="4", phase_update_interval="2",
                         sort_interval="1.5")
        if display:
            h.set_display(True)
        h.reset()
    finally:
        os.environ.pop("PB_RESIDENT", None)
        os.environ.pop("PB_ALLOW_ENV_OVERRIDES", None)
    assert h.advance(steps) == steps
    return h


def test_engine_trail(pb):
    steps = 470  # gates at t = 0, 1, 2, 3, 4 (a wrap of the 4-slot ring), phase updates at 0, 2, 4, re-sorts at 0, 1.5, 3
    # the legacy engine stepped one step at a time, positions captured at every gate step
    from particlerobotsimulations_amd import host
    h = host.HostSim(os.path.join(ROOT, "examples", "example_obstacle.cfg"), engine="legacy", reset=False,
                     max_time="1e9", centroid_int="1", centroid_steps="4", phase_update_interval="2",
                     sort_interval="1.5")
    h.set_display(True)
    h.reset()
    want_xy = np.tile(np.array([-5000.0, 0.0], np.float32), (4, 1))
    want_t = np.full(4, np.nan, np.float32)
    dt, ci, recs = f32(0.01), f32(1.0), 0
    for _ in range(steps):
        t = f32(h.time)
        if f32(t - f32(ci * np.floor(f32(t / ci)))) < dt:
            ind = R.ring_slot(t, ci, 4)
            want_xy[ind] = R.centroid(h.get("pos"))
            want_t[ind] = t
            recs += 1
        assert h.advance(1) == 1
    assert recs == 5
    lx, lt, lr = h.centroid_trail()
    assert_bit_equal(lx, want_xy, "legacy trail vs numpy")
    assert_bit_equal(lt, want_t, "legacy times")
    assert lr == recs
    for resident in (1, 2):  # the per-step kernels, then the resident form forced
        f = run_trail("fused", steps, resident)
        fx, ft, fr = f.centroid_trail()
        assert_bit_equal(fx, want_xy, f"fused trail (resident={resident})")
        assert_bit_equal(ft, want_t, "fused times")
        assert fr == recs
        assert_bit_equal(f.get("pos"), h.get("pos"), "fused pos with trail")
        off = run_trail("fused", steps, resident, display=False)
        for k in ("pos", "vel", "rad", "phase"):
            assert_bit_equal(off.get(k), f.get(k), f"{k}: trail on == off")


def test_reference_frame(tmp_path):
    h = run_trail("fused", 470)
    plain, ref = tmp_path / "plain.ppm", tmp_path / "ref.ppm"
    xy, _, _ = h.centroid_trail()
    c = (float(xy[0, 0]), float(xy[0, 1]) - 2000.0)  # the view centred on the blob
    h.write_frame(str(plain), size=200, center=c, half_extent=4.0)
    h.write_frame(str(ref), size=200, center=c, half_extent=4.0, style="reference")
    a, b = plain.read_bytes(), ref.read_bytes()
    assert a[:15] == b[:15] and len(a) == len(b)
    img = np.frombuffer(b[len(b) - 200 * 200 * 3:], np.uint8).reshape(200, 200, 3)
    assert ((img[..., 0] == 255) & (img[..., 1] == 0) & (img[..., 2] == 0)).any()  # the trail's red discs
    col = h.get("col")
    live = col[:, 1] > 0
    g = np.clip(np.rint(col[live, 1] * np.float32(255)), 0, 255).astype(np.uint8)
    assert np.isin(g, img[..., 1]).mean() > 0.9  # the bots' green levels appear in the frame (some discs hide others)


def test_runner_trail_and_frames(tmp_path):
    exe = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
    trail, frames = tmp_path / "trail.csv", tmp_path / "frames"
    frames.mkdir()
    r = subprocess.run([exe, os.path.join(ROOT, "examples", "example_obstacle.cfg"), "--quiet", "--set", "max_time",
                        "4.695", "--set", "centroid_int", "1", "--set", "centroid_steps", "4", "--set",
                        "phase_update_interval", "2", "--set", "sort_interval", "1.5", "--set", "csv_filename",
                        str(tmp_path / "run.csv"), "--trail", str(trail), "--frames", str(frames), "--frame-size", "64",
                        "--frame-style", "reference"], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    rows = trail.read_text().splitlines()
    assert rows[0] == "slot,time,x,y" and len(rows) == 5
    h = run_trail("fused", 470)
    xy, times, _ = h.centroid_trail()
    for row in rows[1:]:
        k, t, x, y = row.split(",")
        k = int(k)
        assert np.float32(float(t)) == times[k] and np.float32(float(x)) == xy[k, 0]
        assert float(y) == float(np.float64(xy[k, 1]) - 2000.0)
    assert any(p.suffix == ".ppm" for p in frames.iterdir())
