"""One step of the streamlined force kernel (force variant 3, csrc/pb_stream.hip) against a float64 evaluation of
the same operation (tests/stream_ref.py): every output of every one of its eight instantiations, per bot.

How one step is observed.  sim.step(1) from a set state runs k_state (exact actuation and integration, covered bit
for bit elsewhere), a re-sort and ONE unfused force launch: get_state() then returns the positions and radii the force
kernel saw and the velocities and sums it computed from them.  sim.step(2) fuses the next step's actuation
(pbActuateS) and integration into the first force launch.  A phase above 1e7 freezes the radius, the phase update
interval is far away, the clock starts at 5 s (off the gates at 0).

Tolerances are not picked.  tests/golden/stream_step/yardstick.json holds, per input and output, how far the
oracle's own fp32 builds (exact, fma, fma_powf, cuda_like) are from float64 -- maximum and 99th percentile over the
bots none of whose decisions (contact / floor / ramp / far per candidate, held, stopped, actuation branch) lies
within DELTA of its threshold; tests/test_stream_ref.py reproduces that file on the CPU.  The kernel is held to
K[output] times that yardstick, in both statistics.  K covers what the kernel legitimately adds to an FMA build:
v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 at 1 ulp where the reference's divisions and roots round to 0.5 ulp, two or three
of them per term, and another order of additions (contacts last).  K = twice the largest ratio measured on MI355X,
rounded up (profiles/stream_step_errors.txt has every figure):

    output            largest ratio to the yardstick (where)                          K
    vel               1.09  (blob of 2, maximum)                                      3
    absForce_r        1.12  (pair ladder, 99th percentile)                            3
    absForce_a        1.00  (every input)                                             2
    rad               1.00  (both actuation inputs, fused and in two calls)           2

662 figures in all, none above 1.12: nothing to explain (a ratio above 8 would point to a wrong term).  The three
inputs on small, rectangular and anisotropic grids (geom_g8, geom_r8x64, geom_aniso: 60 figures more) were measured
afterwards under the same K: vel 1.25 at most (geom_aniso, maximum; 2 x 1.25 still rounds up to 3), absForce_r 1.00,
absForce_a 1.00 -- also with the 1187 candidates per bot of the 8 x 8 grid.

Where the yardstick is 0 (an output that is exactly 0 in every build, e.g. Sum|F_attr| of a bot without candidates)
the kernel must give exactly 0 too.  Bots excluded by a decision margin still have to be finite and within one jump
of the reference (2.5 N per candidate near a gap threshold, the hold threshold, mu g dt)."""
import json

import numpy as np
import pytest

import stream_ref as sr
from helpers import assert_bit_equal, simparams_from_orc
from oracle import orclib

pytestmark = pytest.mark.gpu

K = {"vel": 3, "fa": 2, "fr": 3, "rad": 2}
Y = json.load(open(sr.YARDSTICK))


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def with_params(P, **kw):
    Q = orclib.OrcParams.from_buffer_copy(P)
    for k, v in kw.items():
        setattr(Q, k, v)
    return Q


def kernel_name(payload, asum, walk):
    b = lambda v: "true" if v else "false"  # noqa: E731
    return f"k_force_stream<{b(payload)}, {b(asum)}, {b(walk)}>("


def configure(sim, walk, sums, variant=3):
    sim.set_force_variant(variant)
    sim.set_lanes_per_bot(1)
    sim.set_resident(1)
    if variant == 3:
        sim.set_stream_walk(walk)
    sim.set_force_sums(sums)


def marker(n):
    """what set_forces leaves in absForce_a / absForce_r before the step (finite: the kernel multiplies absR by 0)"""
    k = np.arange(n, dtype=np.float32)
    return (3.25 + 0.001 * k).astype(np.float32), (1.5 + 0.002 * k).astype(np.float32)


def new_sim(pb, inp, walk, sums=0, cc=0, variant=3, P=None):
    P = with_params(inp["P"] if P is None else P, constrained_contraction=int(cc))
    sp, keep = simparams_from_orc(P)
    sim = pb.Sim(sp, wall_half=inp["wall_half"], keepalive=keep)
    n = inp["n"]
    sim.set_state(pos=inp["pos0"], vel=inp["vel0"], rad=inp["rad"], phase=np.full(n, sr.FROZEN),
                  dead=np.zeros(n, np.int32))
    sim.set_forces(*marker(n))
    sim.time = sr.T0
    configure(sim, walk, sums, variant)
    return sim


def hold_to_yardstick(label, yard, errs, keep):
    """print every figure, then hold max and p99 of each output to K times the yardstick"""
    bad = []
    for key, err in errs.items():
        for stat, got in zip(("max", "p99"), sr.stats(err, keep)):
            y = yard[key][stat]
            ratio = got / y if y > 0 else (0.0 if got == 0 else float("inf"))
            print(f"RATIO {label} {key} {stat} kernel {got:.3e} yardstick {y:.3e} ratio {ratio:.2f} "
                  f"excluded {int((~keep).sum())}")
            if not got <= K[key] * y:
                bad.append((label, key, stat, got, y))
    assert not bad, bad


def check_step(label, inp, st, asum, yard=None):
    """the state after step(1) against the float64 step of the input"""
    ref = inp["ref"]
    n = inp["n"]
    keep = ~ref["excluded"]
    assert (~keep).sum() <= 0.01 * n                       # the cap on exclusions, before looking at the device
    assert_bit_equal(st["pos"], inp["pos1"], f"{label}: positions after the exact integration")
    assert_bit_equal(st["rad"], inp["rad"], f"{label}: frozen radii")
    fa = st["absForce_a"]
    assert (fa is not None) == bool(asum)
    for key in ("vel", "absForce_r") + (("absForce_a",) if asum else ()):
        assert np.isfinite(st[key]).all(), (label, key)
    errs = sr.step_errors(ref, st["vel"], fa, st["absForce_r"])
    # decisions: at rest exactly where the reference stops the bot (a held bot is stopped: it keeps |v| < 1e-6)
    rest = (st["vel"] == 0).all(1)
    assert np.array_equal(rest[keep], ref["stopped"][keep]), (label, np.flatnonzero(rest != ref["stopped"])[:10])
    dv = np.linalg.norm(st["vel"].astype(np.float64) - ref["vel"], axis=1)
    assert (dv[~keep] <= sr.jump_bound(ref)[~keep] + 1e-5).all(), label
    hold_to_yardstick(label, Y["step"][inp["name"]] if yard is None else yard, errs, keep)


def run_step(pb, name, payload, walk, sums=0, cc=0):
    inp = sr.step_input(name)
    assert (int(inp["P"].nDead) == -1) == bool(payload)
    sim = new_sim(pb, inp, walk, sums, cc)
    asum = bool(sums or cc)
    assert sim.force_kernel_name().startswith(kernel_name(payload, asum, walk)), sim.force_kernel_name()
    assert sim.step(1, dt=sr.DT) == 1
    cfg = sim.config()
    assert cfg["force_variant"] == 3 and cfg["force_kind"] == 3 and cfg["stream_walk"] == walk
    st = sim.get_state()
    check_step(f"{name}/{'payload' if payload else 'plain'}/{('off', 'sums', 'cc')[2 if cc else sums]}/walk{walk}",
               inp, st, asum)
    if not asum:   # sums off: absForce_a is left as set_forces put it
        sim.set_force_sums(1)
        assert_bit_equal(sim.get_state()["absForce_a"], marker(inp["n"])[0], f"{name}: absForce_a untouched")
    sim.close()
    return st


# ---- a. the pair ladder: every output is a single term ----------------------------------------------------------
@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("sums", ["off", "sums", "cc"])
@pytest.mark.parametrize("payload", [False, True])
def test_pair_ladder_all_eight_instantiations(pb, payload, sums, walk):
    """2000 isolated pairs (gap -0.02 .. 0.006, dense around 0 / 0.0009 / 0.0019, every orientation, normal and
    tangential approach of both signs, one bot of every other pair at rest) through each instantiation; with the
    payload, its pair in contact / on the floor / on the ramp / far, the payload bot on either side (att1, att2)."""
    names = [f"ladder_payload{k}" for k in range(4)] if payload else ["ladder"]
    for name in names:
        assert not sr.step_input(name)["ref"]["excluded"].any()      # the ladder excludes nobody by construction
        st = run_step(pb, name, payload, walk, sums=int(sums == "sums"), cc=int(sums == "cc"))
        if payload:   # the payload pair itself, on top of the statistics: both bots within K of the yardstick's maximum
            inp = sr.step_input(name)
            n = inp["n"]
            errs = sr.step_errors(inp["ref"], st["vel"], st["absForce_a"], st["absForce_r"])
            for key, e in errs.items():
                assert (e[n - 2:] <= K[key] * Y["step"][name][key]["max"]).all(), (name, key, e[n - 2:])


@pytest.mark.parametrize("name", ["ladder_alt", "ladder_noattr"])
def test_pair_ladder_other_constants(pb, name):
    """spring 700, damping 7, shear 25, attraction 1e-4; and attraction 0 (the ramp then falls to 0 at 0.0019)"""
    for walk in (0, 1):
        run_step(pb, name, False, walk, sums=1)


def test_two_bots_at_the_same_point(pb):
    """two distinct bots at one point, at rest: NaN in the reference, a zero pair force here (k_force_stream's
    comment on the clamped d2), and finite everywhere"""
    inp = sr.step_input("ladder_coincide")
    for walk in (0, 1):
        sim = new_sim(pb, inp, walk, sums=1)
        assert sim.step(1, dt=sr.DT) == 1
        st = sim.get_state()
        for key in ("pos", "vel", "rad", "absForce_a", "absForce_r"):
            assert np.isfinite(st[key]).all(), key
        assert (st["vel"][:2] == 0).all() and (st["absForce_a"][:2] == 0).all() and (st["absForce_r"][:2] == 0).all()
        sim.close()


# ---- b. moving blobs: nobody held, nobody stopped, vel shows every net force ----------------------------------------
@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("sums", [0, 1])
@pytest.mark.parametrize("name", sr.BLOBS)
def test_moving_blob(pb, name, sums, walk):
    """sizes 1, 2, 63, 65, TILE -+ 1, 4 TILE + 1 and 64 TILE - 7 (the per-XCD tile mapping, empty trailing tiles, the
    flattened walk's shadow lanes behind the last bot), spacing 0.16 and 0.17"""
    ref = sr.step_input(name)["ref"]
    assert not ref["held"].any() and ref["stopped"].sum() <= 2
    run_step(pb, name, False, walk, sums=sums)


@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("sums", [0, 1])
def test_moving_blob_with_payload(pb, sums, walk):
    """massFactor 1.7, frictionFactor 0.6, attractionFactor 0.3: the payload branch of pbFrictionAndKickS"""
    run_step(pb, "blob_payload", True, walk, sums=sums)


# ---- c. resting blobs: the decisions ------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("name", sr.RESTS)
def test_resting_blob(pb, name, walk):
    """zero, sub-threshold and slow velocities: held / stopped as the float64 reference decides for every bot whose
    margin exceeds DELTA (check_step), a held bot exactly at rest, the sums compared for every kept bot"""
    inp = sr.step_input(name)
    st = run_step(pb, name, False, walk, sums=1)
    ref = inp["ref"]
    sure = ref["held"] & (ref["hold_margin"] > sr.DELTA_REL)
    assert sure.sum() >= 3 and (st["vel"][sure] == 0).all()


# ---- d / e. pile-up, wrap, aliasing -------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("name", ["pile", "wrap", "alias"])
def test_pile_wrap_alias(pb, name, walk):
    """pile: 60 bots in one cell, more contacts than PB_STREAM_CAP lists; wrap: a blob across the grid's x-wrap next
    to the wall (waves with a wrapped stencil row fall back to the row-by-row loop inside the WALK kernel); alias:
    walls at +-2000 over the 512^2 grid, three blobs in aliased cells"""
    inp = sr.step_input(name)
    if name == "pile":
        p = inp["ref"]["pairs"]
        contacts = np.bincount(p["I"][p["regime"] == 0], minlength=inp["n"])
        assert contacts[:60].max() > 10       # PB_STREAM_CAP
    if name == "wrap":
        h = sr.cell_hashes(orclib, inp["P"], inp["pos1"]) % inp["P"].gridSizeX
        assert (h < 3).any() and (h > inp["P"].gridSizeX - 4).any()
    run_step(pb, name, False, walk, sums=1)


@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("sums", [0, 1])
@pytest.mark.parametrize("name", sr.GEOMS)
def test_small_rectangular_and_anisotropic_grids(pb, name, sums, walk):
    """the wrap blob on an 8 x 8 grid (every cell aliased 545-fold under the +-64 walls: 1187 candidates per bot,
    half of the bots wrap in x), on 8 x 64 and on 64 x 8 with cells 0.235 x 0.31 and origin (-3, -64)"""
    inp = sr.step_input(name)
    P = inp["P"]
    gx = int(P.gridSizeX)
    h = sr.cell_hashes(orclib, P, inp["pos1"]).astype(np.int64)
    cx = np.sort(h, kind="stable") % gx
    wraps = (cx < 2) | (cx >= gx - 2)           # the bot's stencil rows split in two at the x-wrap (nseg == 2)
    assert wraps.any() and not wraps.all()
    if name == "geom_g8":
        assert wraps.mean() >= 0.25
        if walk == 1:
            # a wave is 64 consecutive slots of the sorted order (lanes behind the last bot shadow it): it takes the
            # flattened walk only when none of its bots wraps
            pad = np.concatenate([wraps, np.full(-len(wraps) % 64, wraps[-1])]).reshape(-1, 64)
            falls_back = pad.any(1)
            assert falls_back.any() and not falls_back.all(), falls_back.mean()
    run_step(pb, name, False, walk, sums=sums)


# ---- f. a batch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", [0, 1])
def test_batch_of_three(pb, walk):
    """three members with different constants, payload on: the blockIdx.y parameter block and cell-table offsets"""
    inps = [sr.step_input(name) for name in sr.BATCH]
    sps = [simparams_from_orc(i["P"]) for i in inps]
    ens = pb.Ensemble([s[0] for s in sps], keepalive=[s[1] for s in sps])
    n = inps[0]["n"]
    from particlerobotsimulations_amd import _capi
    for m, inp in enumerate(inps):
        ens.set_state_of(m, pos=inp["pos0"], vel=inp["vel0"], rad=inp["rad"], phase=np.full(n, sr.FROZEN),
                         dead=np.zeros(n, np.int32))
        a, r = marker(n)
        _capi.check(_capi.lib().pbSimSetForcesOf(ens._h, m, _capi.np_ptr(a), _capi.np_ptr(r)), "pbSimSetForcesOf")
    ens.time = sr.T0
    configure(ens, walk, 1)
    assert ens.force_kernel_name().startswith(kernel_name(True, True, walk))
    assert ens.step(1, dt=sr.DT) == 1
    for m, inp in enumerate(inps):
        check_step(f"batch{m}/walk{walk}", inp, ens.get_state_of(m), True)
    ens.close()


# ---- g. fused actuation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("walk", [0, 1])
@pytest.mark.parametrize("mode", ["cc0", "cc0_sums", "cc1"])
def test_second_step_actuation(pb, mode, walk, fused):
    """step(2): the second actuation runs inside k_force_stream (pbActuateS) on the sums that launch has just
    computed; step(1); step(1): the same actuation in exact arithmetic (k_state) on the stored sums, held to the same
    bound, which shows the comparison is sound.  Phases reach every branch (dead, frozen, negative time wrapped, idle,
    rising free / stalled, falling free / constrained / stalled)."""
    cc = int(mode == "cc1")
    inp = sr.actuation_input(cc)
    n = inp["n"]
    keep = inp["margin"] > sr.DELTA_REL
    assert (~keep).sum() <= 0.01 * n and inp["ref1"]["excluded"].sum() <= 0.01 * n
    sp, keepalive = simparams_from_orc(inp["P"])
    sim = pb.Sim(sp, keepalive=keepalive)
    sim.set_state(pos=inp["pos0"], vel=inp["vel0"], rad=inp["rad0"], phase=inp["phase"], dead=inp["dead"])
    sim.set_forces(inp["absA0"], inp["absR0"])
    sim.time = sr.T0
    configure(sim, walk, int(mode == "cc0_sums"))
    assert sim.force_kernel_name().startswith(kernel_name(False, mode != "cc0", walk))
    if fused:
        assert sim.step(2, dt=sr.DT) == 2
        assert sim.stats()["fused_launches"] == 1
    else:
        assert sim.step(1, dt=sr.DT) == 1 and sim.step(1, dt=sr.DT) == 1
        assert sim.stats()["fused_launches"] == 0
    rad = sim.get_state()["rad"]
    sim.close()
    assert np.isfinite(rad).all()
    still = np.isin(inp["branch"], (0, 1, 2)) & keep          # dead, frozen, idle: untouched
    assert np.array_equal(rad[still], inp["rad1"][still])
    err = np.abs(rad.astype(np.float64) - inp["rad2"]) / float(inp["P"].max_radius)
    # an excluded bot may take the other branch: still inside [min_radius, max_radius]
    assert (rad >= inp["P"].min_radius).all() and (rad <= inp["P"].max_radius).all()
    hold_to_yardstick(f"actuation/{mode}/walk{walk}/{'fused' if fused else 'two_calls'}", Y["actuation"][f"cc{cc}"],
                      {"rad": err}, keep)


# ---- h. obstacles ---------------------------------------------------------------------------------------------------
def test_obstacles_against_the_exact_kernel(pb):
    """A circular and a rectangular obstacle inside a moving blob: variant 3 against variant 2 on the device after
    one step from the same state, to the bounds of the same blob without obstacles (the obstacle terms are the same
    code, pbObstacles, in both kernels)."""
    name = f"blob_{4 * sr.TILE + 1}_16"
    inp = sr.step_input(name)
    P = with_params(inp["P"], n_cir_obstacles=1, nobstacles=1)
    P.x_cir_obs[0], P.y_cir_obs[0], P.r_cir_obs[0] = 0.3, 0.2, 0.5
    P.x1obs[0], P.x2obs[0], P.y1obs[0], P.y2obs[0] = -1.6, -1.2, -0.8, 0.9
    out = {}
    for variant in (2, 3):
        sim = new_sim(pb, inp, 1, sums=1, variant=variant, P=P)
        assert sim.step(1, dt=sr.DT) == 1
        out[variant] = sim.get_state()
        sim.close()
    a, b = out[2], out[3]
    assert_bit_equal(a["pos"], b["pos"], "same state")
    hit = a["absForce_r"] > 2 * (inp["ref"]["fr"] + 1.0)      # an obstacle's spring is stiff: bots inside one stand out
    assert hit.sum() >= 20
    fa, fr = a["absForce_a"].astype(np.float64), a["absForce_r"].astype(np.float64)
    ref = {"vel": a["vel"].astype(np.float64), "fa": fa, "fr": fr, "mass": inp["ref"]["mass"], "scale": fa + fr}
    errs = sr.step_errors(ref, b["vel"], b["absForce_a"], b["absForce_r"])
    hold_to_yardstick("obstacles/variant3_vs_2", Y["step"][name], errs, ~inp["ref"]["excluded"])
