"""float64 reference of ONE collide step and of the radius actuation, in plain numpy (no GPU), and the inputs
the per-step tests of the streamlined force kernel run it on (tests/test_stream_ref.py on the CPU,
tests/test_gpu_stream_step.py on the device; force variant 3, csrc/pb_stream.hip).

The operation is the reference's (oracle/pb_oracle.c: orc_collide / pair_force / orc_updateRad_light_wave), evaluated
on the fp32 inputs promoted to float64:

  candidates   every bot of the 25 cells around the bot's own cell, grid wrap and aliased cells included (the
               cells are the oracle's orc_calcHash, which the device does not touch); far candidates do contribute
               A / gap^2, so brute force over all pairs would be another operation
  pair law     spring / dashpot / shear in contact; the 2.5 N floor below a gap of 0.0009, the ramp with slope
               (A / 0.0019^2 - 2.5) / 0.001 up to 0.0019, A / gap^2 beyond; A carries the payload factor of either side
  tail         static hold, kick, kinetic friction (payload mass and friction factors)

Obstacles are left out: the streamlined kernel calls the exact kernels' own pbObstacles.

Next to every value the reference keeps the DECISIONS it took and how far each was from going the other way (the
margin): a kernel that rounds differently may legitimately decide a pair or a bot within DELTA of a threshold the
other way, so those bots are excluded from value comparisons (never from finiteness, never from the one-jump bound)."""
import ctypes as C
import functools
import os

import numpy as np

INT1 = float(np.float32(0.0009))   # the fp32 constants of the pair law, promoted
INT2 = float(np.float32(0.0019))
FMIN = 2.5
HOLD_V = float(np.float32(0.000001))
DT = float(np.float32(0.01))
T0 = 5.0                           # time of the step: away from the phase-update and re-sort gates at 0
FROZEN = np.float32(2e7)           # a phase above 1e7 freezes the radius

DELTA_GAP = 1e-6    # absolute, on gaps: 2 * PB_STREAM_NEAR = 2e-7 is where the kernel re-decides exactly
DELTA_REL = 1e-5    # relative, on the hold / stop / actuation decisions
REGIMES = ("contact", "floor", "ramp", "far")
ACT_BRANCHES = ("dead", "frozen", "idle", "rise_stall", "rise", "fall_free", "fall_stall", "fall_constrained")

TILE = 256          # the force kernels' workgroup (csrc/pb_engine.hpp PB_TILE)
FAR_PUI = 1.0e9     # phase_update_interval that keeps the phase update out
YARDSTICK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_step", "yardstick.json")


def _f(x):
    return float(x)


# ------------------------------------------------------------------------------------------------------------
# candidates
# ------------------------------------------------------------------------------------------------------------
def cell_hashes(orc, P, pos):
    n = len(pos)
    h, idx = np.empty(n, np.uint32), np.empty(n, np.uint32)
    orc.lib().orc_calcHash(C.byref(P), h, idx, np.ascontiguousarray(pos, np.float32).reshape(-1), n)
    return h


def candidate_pairs(orc, P, pos):
    """(I, J): for every bot I its candidates J != I, the reference's set (orc_collide's stencil loop)."""
    n = len(pos)
    h = cell_hashes(orc, P, pos).astype(np.int64)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    GX, GY = int(P.gridSizeX), int(P.gridSizeY)
    mx, my = h % GX, h // GX
    allI, allJ = [], []
    me = np.arange(n)
    for y in range(-2, 3):
        for x in range(-2, 3):
            nh = ((my + y) & (GY - 1)) * GX + ((mx + x) & (GX - 1))
            lo, hi = np.searchsorted(hs, nh, "left"), np.searchsorted(hs, nh, "right")
            cnt = hi - lo
            tot = int(cnt.sum())
            if tot == 0:
                continue
            i = np.repeat(me, cnt)
            off = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            j = order[np.repeat(lo, cnt) + off]
            keep = i != j
            allI.append(i[keep])
            allJ.append(j[keep])
    if not allI:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(allI), np.concatenate(allJ)


# ------------------------------------------------------------------------------------------------------------
# the pair law
# ------------------------------------------------------------------------------------------------------------
def pair_terms(P, pa, pb, va, vb, ra, rb, attraction):
    """float64 pair force ON bot a from bot b, arrays of pairs.  Returns dict: tx, ty, mag, regime (index into
    REGIMES, -1 for two bots at the same point: zero force), margin (distance of the gap from the nearest of the
    thresholds 0 / 0.0009 / 0.0019)."""
    pa, pb, va, vb = (np.asarray(a, np.float64) for a in (pa, pb, va, vb))
    ra, rb = np.asarray(ra, np.float64), np.asarray(rb, np.float64)
    A = np.broadcast_to(np.asarray(attraction, np.float64), ra.shape)
    r = pb - pa
    dist = np.hypot(r[:, 0], r[:, 1])
    same = dist == 0.0
    reach = ra + rb
    gap = dist - reach
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.where(same[:, None], 0.0, r / np.where(same, 1.0, dist)[:, None])
        regime = np.where(gap < 0.0, 0, np.where(gap < INT1, 1, np.where(gap < INT2, 2, 3)))
        # contact
        rv = vb - va
        vn = (rv * nrm).sum(1)
        tv = rv - vn[:, None] * nrm
        ks = -_f(P.spring) * (reach - dist)
        tc = ks[:, None] * nrm + _f(P.damping) * rv + _f(P.shear) * tv
        # attraction
        slope = (A / (INT2 * INT2) - FMIN) / (INT2 - INT1)
        coef = np.where(regime == 1, FMIN, np.where(regime == 2, FMIN + slope * (gap - INT1),
                                                     A / np.where(gap == 0.0, 1.0, gap * gap)))
    contact = regime == 0
    t = np.where(contact[:, None], tc, coef[:, None] * nrm)
    mag = np.where(contact, np.hypot(tc[:, 0], tc[:, 1]), coef)
    t[same] = 0.0
    mag = np.where(same, 0.0, mag)
    regime = np.where(same, -1, regime)
    margin = np.minimum(np.abs(gap), np.minimum(np.abs(gap - INT1), np.abs(gap - INT2)))
    margin = np.where(same, np.inf, margin)
    return {"tx": t[:, 0], "ty": t[:, 1], "mag": mag, "regime": regime, "margin": margin, "gap": gap}


def _conj_margin(a_true, a_margin, b_true, b_margin):
    """margin of the decision (a and b): how far the nearest input that could change it is from its threshold"""
    both = a_true & b_true
    neither = ~a_true & ~b_true
    return np.where(both, np.minimum(a_margin, b_margin),
                    np.where(neither, np.maximum(a_margin, b_margin), np.where(a_true, b_margin, a_margin)))


def collide_step(orc, P, pos, vel, rad, dt=DT):
    """One collide step in float64 on fp32 inputs (original bot order).  Returns a dict of per-bot arrays
    Fx, Fy, fa, fr, vel (n, 2), scale, and the decision record: held, stopped, hold_margin, stop_margin,
    pair_margin (smallest gap margin over the bot's candidates), near_pairs (candidates within DELTA_GAP of a
    threshold), excluded (some decision of the bot within DELTA), coincident, and the pair arrays under "pairs"."""
    pos32, vel32, rad32 = (np.ascontiguousarray(a, np.float32) for a in (pos, vel, rad))
    pos, vel, rad = pos32.astype(np.float64), vel32.astype(np.float64), rad32.astype(np.float64)
    n = len(pos)
    I, J = candidate_pairs(orc, P, pos32)
    payload = int(P.nDead) == -1
    pidx = int(P.nCells) - 1
    A = np.full(I.shape, _f(P.attraction))
    if payload:
        af = _f(P.attractionFactor)
        A = A * np.where(J == pidx, af, 1.0) * np.where(I == pidx, af, 1.0)
    pt = pair_terms(P, pos[I], pos[J], vel[I], vel[J], rad[I], rad[J], A)
    contact = pt["regime"] == 0
    Fx = np.bincount(I, pt["tx"], minlength=n)
    Fy = np.bincount(I, pt["ty"], minlength=n)
    fr = np.bincount(I, np.where(contact, pt["mag"], 0.0), minlength=n)
    fa = np.bincount(I, np.where(contact, 0.0, pt["mag"]), minlength=n)
    pair_margin = np.full(n, np.inf)
    np.minimum.at(pair_margin, I, pt["margin"])
    near_pairs = np.bincount(I, pt["margin"] <= DELTA_GAP, minlength=n).astype(np.int64)
    coincident = np.bincount(I, pt["regime"] == -1, minlength=n) > 0

    isp = np.zeros(n, bool)
    if payload:
        isp[pidx] = True
    friction = np.where(isp, _f(P.friction) * _f(P.frictionFactor), _f(P.friction))
    gravity = np.where(isp, _f(P.gravity) * _f(P.massFactor), _f(P.gravity))
    mass = np.where(isp, _f(P.massFactor), 1.0)
    speed0 = np.hypot(vel[:, 0], vel[:, 1])
    Fmag = np.hypot(Fx, Fy)
    holdF = 2.0 * friction * gravity
    v_small, f_small = speed0 < HOLD_V, Fmag < holdF
    with np.errstate(divide="ignore", invalid="ignore"):
        mv = np.abs(speed0 / HOLD_V - 1.0)
        mf = np.where(holdF > 0, np.abs(Fmag / np.where(holdF > 0, holdF, 1.0) - 1.0), np.inf)
    held = v_small & f_small
    hold_margin = _conj_margin(v_small, mv, f_small, mf)
    kx = np.where(held, 0.0, Fx) / mass * dt
    ky = np.where(held, 0.0, Fy) / mass * dt
    v1 = vel + np.stack([kx, ky], 1)
    fric = friction * gravity * dt
    s1 = np.hypot(v1[:, 0], v1[:, 1])
    stopped = s1 < fric
    with np.errstate(divide="ignore", invalid="ignore"):
        stop_margin = np.where(fric > 0, np.abs(s1 / np.where(fric > 0, fric, 1.0) - 1.0), np.inf)
        vout = np.where(stopped[:, None], 0.0, v1 * (1.0 - fric / np.where(s1 > 0, s1, 1.0))[:, None])
    excluded = (pair_margin <= DELTA_GAP) | (hold_margin <= DELTA_REL) | (stop_margin <= DELTA_REL) | coincident
    return {"Fx": Fx, "Fy": Fy, "fa": fa, "fr": fr, "vel": vout, "scale": np.maximum(Fmag, fa + fr),
            "mass": mass, "fric": fric, "holdF": holdF, "held": held, "stopped": stopped,
            "hold_margin": hold_margin, "stop_margin": stop_margin, "pair_margin": pair_margin,
            "near_pairs": near_pairs, "coincident": coincident, "excluded": excluded,
            "pairs": {"I": I, "J": J, **pt}}


# ------------------------------------------------------------------------------------------------------------
# radius actuation
# ------------------------------------------------------------------------------------------------------------
def actuate(P, rad, phase, dead, absA, absR, time, dt=DT):
    """orc_updateRad_light_wave in float64.  Returns (new radius, branch index into ACT_BRANCHES, margin): the
    margin is the relative distance of the nearest comparison the bot's branch rests on from its threshold."""
    rad = np.asarray(rad, np.float64)
    phase32 = np.asarray(phase, np.float32)
    phase = phase32.astype(np.float64)
    absA, absR = np.asarray(absA, np.float64), np.asarray(absR, np.float64)
    dead = np.asarray(dead) != 0
    rp, rmin, rmax = _f(P.rise_period), _f(P.min_radius), _f(P.max_radius)
    con, conc = _f(P.constraint), _f(P.constraint_contraction)
    period = (int(P.Nx) + 1) * rp
    max_speed = float(np.float32(0.1))
    frozen = phase32 > np.float32(10000000.0)
    t1 = _f(time) + np.where(frozen, 0.0, phase)
    neg = t1 < 0
    t1 = np.where(neg, t1 + 100 * period, t1)
    t1w = np.where(t1 >= period, t1 - period * np.floor(t1 / period), t1)
    # margins of the time comparisons, relative to the period: t1 against 0, a multiple of the period, 2 rp, rp
    m_time = np.minimum.reduce([np.abs(_f(time) + phase), np.abs(t1w), np.abs(period - t1w), np.abs(t1w - 2 * rp),
                                np.abs(t1w - rp)]) / period
    idle = t1w >= 2 * rp
    rising = t1w <= rp
    target = np.where(rising, rmin + (rmax - rmin) / rp * t1w, rmax + (rmin - rmax) / rp * (t1w - rp))
    want = target - rad
    torque = np.minimum(want * con * rad / max_speed / rmax / dt, con)
    tr = torque / rad
    up = want > 0
    drive = tr > absR
    dr_up = np.where(drive, max_speed * rmax / con * (tr - absR) * dt, 0.0)
    if int(P.constrained_contraction):
        pull = -conc * want > absA * rad
        dr_dn = np.maximum(np.where(pull, (conc * want + absA * rad) / conc, 0.0), -rmax * dt)
    else:
        pull = np.ones_like(up)
        dr_dn = want
    out = np.clip(rad + np.where(up, dr_up, dr_dn), rmin, rmax)
    live = ~(dead | frozen | idle)
    out = np.where(live, out, rad)
    cc = bool(int(P.constrained_contraction))
    branch = np.where(dead, 0, np.where(frozen, 1, np.where(idle, 2, np.where(
        up, np.where(drive, 4, 3), np.where(pull, 7 if cc else 5, 6)))))
    with np.errstate(divide="ignore", invalid="ignore"):
        m_want = np.abs(want) / rmax
        m_drive = np.abs(tr - absR) / np.maximum(np.maximum(np.abs(tr), absR), 1e-300)
        lhs, rhs = -conc * want, absA * rad
        m_pull = np.abs(lhs - rhs) / np.maximum(np.maximum(np.abs(lhs), np.abs(rhs)), 1e-300) if cc else np.inf
    margin = np.minimum(m_time, np.minimum(m_want, np.where(up, m_drive, m_pull)))
    margin = np.where(dead | frozen, np.inf, np.where(idle, m_time, margin))
    return out, branch, margin


# ------------------------------------------------------------------------------------------------------------
# the oracle's fp32 builds on the same inputs (for the yardstick; CPU only)
# ------------------------------------------------------------------------------------------------------------
BUILDS = (None, "fma", "fma_powf", "cuda_like")   # None: the oracle itself


def integrate_fp32(orc, P, pos, vel, rad, dt=DT):
    """the oracle's exact integration (wall clamp included): what k_state leaves for the force kernel"""
    pos, vel = (np.ascontiguousarray(a, np.float32).copy() for a in (pos, vel))
    rad = np.ascontiguousarray(rad, np.float32)
    orc.lib().orc_integrateSystem(C.byref(P), pos.reshape(-1), vel.reshape(-1), rad, np.float32(dt), len(rad))
    return pos, vel


def collide_fp32(orc, P, pos, vel, rad, build=None, dt=DT):
    """orc_collide of one of the oracle's builds on the given (post-integration) state: vel, absForce_a, absForce_r
    in original bot order."""
    L = orc.variant_lib(build)
    n = len(rad)
    pos, vel, rad = (np.ascontiguousarray(a, np.float32) for a in (pos, vel, rad))
    h, idx = np.empty(n, np.uint32), np.empty(n, np.uint32)
    L.orc_calcHash(C.byref(P), h, idx, pos.reshape(-1), n)
    L.orc_sortParticlebots(h, idx, n)
    cs, ce = np.empty(P.numCells, np.uint32), np.zeros(P.numCells, np.uint32)
    sp, sv, sr = np.empty(2 * n, np.float32), np.empty(2 * n, np.float32), np.empty(n, np.float32)
    L.orc_reorderDataAndFindCellStart(C.byref(P), cs, ce, sp, sv, sr, h, idx, pos.reshape(-1), vel.reshape(-1), rad,
                                      n, P.numCells)
    nv, fa, fr = np.zeros(2 * n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    L.orc_collide(C.byref(P), nv, fa, fr, sp, sv, sr, idx, cs, ce, n, np.float32(dt))
    return nv.reshape(n, 2), fa, fr


def actuate_fp32(orc, P, rad, phase, dead, absA, absR, time, build=None, dt=DT):
    L = orc.variant_lib(build)
    rad = np.ascontiguousarray(rad, np.float32).copy()
    L.orc_updateRad_light_wave(C.byref(P), np.ascontiguousarray(absA, np.float32), np.ascontiguousarray(absR, np.float32),
                               rad, np.ascontiguousarray(phase, np.float32), np.float32(time), np.float32(dt),
                               np.ascontiguousarray(dead, np.int32), len(rad))
    return rad


# ------------------------------------------------------------------------------------------------------------
# errors in the issue's scales
# ------------------------------------------------------------------------------------------------------------
def step_errors(ref, vel, fa, fr, dt=DT):
    """per-bot relative errors of a candidate's outputs against the float64 step `ref`:
    vel: |dv| / (dt / m) over max(|F|, Sum|F_attr| + Sum|F_rep|); fa, fr: over their own value (where the reference's
    value is 0 the candidate's must be 0 too: error inf otherwise).  fa may be None (sums not kept)."""
    out = {}
    dv = np.asarray(vel, np.float64) - ref["vel"]
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(ref["scale"] > 0, ref["scale"], 1.0)
        out["vel"] = np.hypot(dv[:, 0], dv[:, 1]) / (dt / ref["mass"]) / scale
        for key, val in (("fa", fa), ("fr", fr)):
            if val is None:
                continue
            val = np.asarray(val, np.float64)
            r = ref[key]
            out[key] = np.where(r > 0, np.abs(val - r) / np.where(r > 0, r, 1.0), np.where(val == 0, 0.0, np.inf))
    return out


def jump_bound(ref, dt=DT):
    """how far a bot's velocity may be from the reference's when one of its decisions goes the other way: 2.5 N per
    candidate near a gap threshold, the hold threshold when the hold is near, mu g dt when the stop is near"""
    near_hold = ref["hold_margin"] <= DELTA_REL
    near_stop = ref["stop_margin"] <= DELTA_REL
    return ((FMIN * ref["near_pairs"] + np.where(near_hold, ref["holdF"], 0.0)) * dt / ref["mass"]
            + np.where(near_stop, ref["fric"], 0.0))


def stats(err, keep):
    """(max, 99th percentile) over the kept bots"""
    e = err[keep]
    if e.size == 0:
        return 0.0, 0.0
    return float(e.max()), float(np.quantile(e, 0.99))


# ------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------
PAYLOAD_KW = dict(nDead=-1, attractionFactor=0.3, massFactor=1.7, frictionFactor=0.6)
ALT_KW = dict(spring=700.0, damping=7.0, shear=25.0, attraction=1.0e-4)
BLOB_SIZES = (1, 2, 63, 65, TILE - 1, TILE + 1, 4 * TILE + 1, 64 * TILE - 7)
DRIFT = np.float32([0.9, 0.5])   # |drift| = 1.03: far above the hold speed 1e-6 and above mu g dt = 0.022


def make_params(orc, n, geometry=None, **kw):
    """geometry: a name of helpers.GEOMETRIES, applied after the derive step (which only makes square grids)"""
    base = dict(nCells=n, nDead=0, seed=7, phase_std=0.0, max_time=1e9, light_x=-3.0, light_y=2.0,
                phase_update_interval=FAR_PUI)
    base.update(kw)
    P = orc.default_params(**base)
    if geometry is not None:
        import helpers
        P = helpers.geometry(P, geometry)
    return P


def ladder_gaps(npairs):
    """gaps over [-0.02, 0.006], dense around 0 / 0.0009 / 0.0019, none closer to them than 2 * DELTA_GAP"""
    rng = np.random.default_rng(101)
    parts = [np.linspace(-0.02, 0.006, npairs // 4)]
    per = (npairs - npairs // 4) // 3
    for k, thr in enumerate((0.0, INT1, INT2)):
        cnt = per if k < 2 else npairs - npairs // 4 - 2 * per
        mag = 10.0 ** rng.uniform(np.log10(2e-6), np.log10(4e-4), cnt)
        parts.append(thr + mag * np.where(rng.random(cnt) < 0.5, -1.0, 1.0))
    g = np.concatenate(parts)
    for thr in (0.0, INT1, INT2):
        close = np.abs(g - thr) < 2e-6
        g[close] = thr + 2e-6 * np.where(g[close] < thr, -1.0, 1.0)
    return g


def ladder_state(orc, P, last_gap=None, swap=False, npairs=2000, coincide=False):
    """isolated pairs on a 1.5-unit lattice (more than six cells: a bot's only candidate is its partner).  Bot 2k is
    at rest in every other pair, bot 2k + 1 moves; the LAST pair holds the payload bot (index n - 1): `last_gap`
    puts that pair into a regime, `swap` puts the payload bot on the other side of it."""
    rng = np.random.default_rng(202)
    lo, hi = _f(P.min_radius), _f(P.max_radius)
    side = int(np.ceil(np.sqrt(npairs)))
    k = np.arange(npairs)
    site = np.stack([(k % side) - (side - 1) / 2.0, (k // side) - (side - 1) / 2.0], 1) * 1.5
    site += rng.uniform(-0.05, 0.05, site.shape)
    ra, rb = rng.uniform(lo, hi, npairs), rng.uniform(lo, hi, npairs)
    theta = rng.uniform(0, 2 * np.pi, npairs)
    theta[:8] = np.arange(8) * (np.pi / 4)          # axis-aligned and diagonal pairs
    theta[8:16] = np.arange(8) * (np.pi / 4)
    gaps = ladder_gaps(npairs)
    if last_gap is not None:
        gaps[-1] = last_gap
    dist = ra + rb + gaps
    u = np.stack([np.cos(theta), np.sin(theta)], 1)
    u[np.abs(u) < 1e-12] = 0.0
    pa = site - 0.5 * dist[:, None] * u
    pb_ = site + 0.5 * dist[:, None] * u
    tang = np.stack([-u[:, 1], u[:, 0]], 1)
    # relative velocity: normal and tangential parts of both signs
    vn = rng.uniform(0.3, 1.2, npairs) * np.where(rng.random(npairs) < 0.5, -1, 1)
    vt = rng.uniform(0.3, 1.2, npairs) * np.where(rng.random(npairs) < 0.5, -1, 1)
    vb = vn[:, None] * u + vt[:, None] * tang
    va = rng.uniform(-0.8, 0.8, (npairs, 2))
    va[::2] = 0.0
    n = 2 * npairs
    pos, vel, rad = np.empty((n, 2), np.float32), np.empty((n, 2), np.float32), np.empty(n, np.float32)
    vel[0::2], vel[1::2] = va, vb
    rad[0::2], rad[1::2] = ra, rb
    # the force kernel sees the state AFTER the step's integration: start one integration back, then trim the
    # mover's radius (its ulp is 7e-9; a coordinate's is 4e-6 out here) so that the gap the kernel sees is the wanted one
    pos[0::2], pos[1::2] = pa - va * DT, pb_ - vb * DT
    p1, _ = integrate_fp32(orc, P, pos, vel, rad)
    p1 = p1.astype(np.float64)
    seen = np.hypot(*(p1[1::2] - p1[0::2]).T)
    rad[1::2] = seen - rad[0::2].astype(np.float64) - gaps
    if swap:   # the payload bot on the other side of its pair: the at-rest bot carries att1, the mover att2
        for a in (pos, vel, rad):
            a[[n - 2, n - 1]] = a[[n - 1, n - 2]]
    if coincide:   # two distinct bots at the same point, at rest (they stay there through the integration)
        pos[1] = pos[0]
        vel[0] = vel[1] = 0.0
    return pos, vel, rad


def blob_state(n, spacing, seed, center=(0.0, 0.0), motion="moving"):
    from helpers import jittered_blob
    rng = np.random.default_rng(seed)
    pos, vel, rad = jittered_blob(n, spacing, rng, center=center)
    if motion == "moving":
        vel = (DRIFT + rng.standard_normal((n, 2)) * 0.03).astype(np.float32)
    else:  # thirds: at rest, below the hold speed, slow (most of those are stopped by kinetic friction)
        kind = rng.integers(0, 3, n)
        ang = rng.uniform(0, 2 * np.pi, n)
        mag = np.where(kind == 0, 0.0, np.where(kind == 1, rng.uniform(1e-7, 8e-7, n),
                                                10.0 ** rng.uniform(-5.5, -1.0, n)))
        vel = (mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
    return pos, vel, rad


def pile_state():
    """60 bots in one cell inside a 700-bot blob: more contacts per bot than the kernel's list holds"""
    pos, vel, rad = blob_state(700, 0.17, 23, center=(5.0, 0.0))
    rng = np.random.default_rng(24)
    pos[:60] = np.float32([5.0, 0.0]) + rng.uniform(-0.09, 0.09, (60, 2)).astype(np.float32)
    return pos, vel, rad


def alias_state():
    """three 1200-bot blobs whose cells alias under walls at +-2000 (the 512^2 grid spans 120 units)"""
    span = 512 * 0.235
    parts = [blob_state(1200, 0.16, 41 + k, center=c) for k, c in
             enumerate(((-3.0, 2.0), (-3.0 + 3 * span, 2.0), (-3.0 + 0.4, 2.0 - 5 * span)))]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _spec(name):
    """name -> (parameter overrides, state builder taking (orc, P), wall_half)"""
    if name.startswith("ladder"):
        kw = {}
        last, swap = None, False
        if name == "ladder_alt":
            kw = dict(ALT_KW)
        elif name == "ladder_noattr":
            kw = dict(attraction=0.0)
        elif name.startswith("ladder_payload"):
            k = int(name[-1])   # the payload pair in contact / on the floor / on the ramp / far
            last, swap = (-0.01, 0.0004, 0.0014, 0.004)[k], bool(k % 2)
            kw = dict(PAYLOAD_KW)
        co = name == "ladder_coincide"
        return kw, 4000, (lambda orc, P: ladder_state(orc, P, last_gap=last, swap=swap, coincide=co)), 0.0
    if name.startswith("blob_payload"):
        return dict(PAYLOAD_KW), 4 * TILE + 1, (lambda orc, P: blob_state(4 * TILE + 1, 0.16, 77)), 0.0
    if name.startswith("blob_") or name.startswith("rest_"):
        _, n, sp = name.split("_")
        n, sp = int(n), int(sp) / 100.0
        motion = "moving" if name.startswith("blob_") else "rest"
        return {}, n, (lambda orc, P: blob_state(n, sp, 1000 + n + int(sp * 100), motion=motion)), 0.0
    if name == "pile":
        return {}, 700, (lambda orc, P: pile_state()), 0.0
    if name == "wrap":
        return {}, 3000, (lambda orc, P: blob_state(3000, 0.16, 5, center=(57.0, 61.0))), 0.0
    if name.startswith("geom_"):   # the wrap blob on a small, a rectangular and an anisotropic grid
        return dict(geometry=name[5:]), 3000, (lambda orc, P: blob_state(3000, 0.16, 5, center=(57.0, 61.0))), 0.0
    if name == "alias":
        return dict(arena_half=2000.0, grid=512), 3600, (lambda orc, P: alias_state()), 2000.0
    if name.startswith("batch"):
        m = int(name[-1])
        kw = dict(PAYLOAD_KW)
        kw.update([dict(), dict(ALT_KW, massFactor=0.6, attractionFactor=2.0),
                   dict(friction=0.25, attractionFactor=0.0, frictionFactor=1.5, spring=1300.0)][m])
        return kw, 4 * TILE + 1, (lambda orc, P: blob_state(4 * TILE + 1, (0.16, 0.17, 0.165)[m], 300 + m)), 0.0
    raise KeyError(name)


LADDERS = ("ladder", "ladder_alt", "ladder_noattr") + tuple(f"ladder_payload{k}" for k in range(4))
BLOBS = tuple(f"blob_{n}_{s}" for n in BLOB_SIZES for s in (16, 17))
RESTS = tuple(f"rest_{n}_{s}" for n, s in ((4 * TILE + 1, 16), (4 * TILE + 1, 17), (64 * TILE - 7, 16)))
BATCH = tuple(f"batch{m}" for m in range(3))
GEOMS = ("geom_g8", "geom_r8x64", "geom_aniso")
STEP_INPUTS = LADDERS + BLOBS + ("blob_payload",) + RESTS + ("pile", "wrap", "alias") + BATCH + GEOMS


@functools.lru_cache(maxsize=None)
def step_input(name):
    """The named input, its parameters, the state the force kernel sees after the exact integration of the step
    and the float64 step on it.  Computed once per process and shared: treat as read-only."""
    from oracle import orclib as orc
    kw, n, build, wall = _spec(name)
    P = make_params(orc, n, **kw)
    pos0, vel0, rad = build(orc, P)
    assert len(rad) == n
    pos1, vel1 = integrate_fp32(orc, P, pos0, vel0, rad)
    ref = collide_step(orc, P, pos1, vel1, rad)
    return {"name": name, "P": P, "n": n, "wall_half": wall, "pos0": pos0, "vel0": vel0, "rad": rad,
            "pos1": pos1, "vel1": vel1, "ref": ref}


# fused actuation -----------------------------------------------------------------------------------------
ACT_N = 4 * TILE + 1


@functools.lru_cache(maxsize=None)
def actuation_input(cc):
    """A moving blob whose phases reach every branch of the actuation (cc: constrained_contraction), with the
    sums of the step before given (set_forces).  Two steps: the first actuation is exact (k_state) on the given
    sums, the second (fused into the force kernel, pbActuateS) on the sums of the first force launch."""
    from oracle import orclib as orc
    n = ACT_N
    P = make_params(orc, n, constrained_contraction=int(cc))
    rng = np.random.default_rng(900 + cc)
    pos0, vel0, rad0 = blob_state(n, 0.17, 901)
    # the last TILE bots stand alone on a 1.5-unit lattice beside the blob: no contact, Sum|F_rep| = 0, so they can
    # rise against nothing (a bot inside the moving blob is always stalled by its contacts)
    k = np.arange(TILE)
    pos0[n - TILE:] = np.stack([10.0 + 1.5 * (k % 16), -12.0 + 1.5 * (k // 16)], 1)
    rp = _f(P.rise_period)
    period = (int(P.Nx) + 1) * rp
    # t1 = T0 + phase spread over [-2, 1.5) periods: negative (wrapped by + 100 periods), rising, falling, idle
    phase = (rng.uniform(-2.0, 1.5, n) * period - T0).astype(np.float32)
    phase[rng.random(n) < 0.06] = FROZEN
    dead = (rng.random(n) < 0.06).astype(np.int32)
    # sums of the step before: from nothing (a free bot) to more than the torque cap can push against
    absR0 = (rng.uniform(0.0, 9.0, n) * (rng.random(n) < 0.7)).astype(np.float32)
    absA0 = (rng.uniform(0.0, 12.0, n) * (rng.random(n) < 0.8)).astype(np.float32)
    t0 = np.float32(T0)
    t1 = np.float32(t0 + np.float32(DT))
    # step 1: exact actuation and integration (k_state is bit-identical to the oracle), then the force launch
    rad1 = actuate_fp32(orc, P, rad0, phase, dead, absA0, absR0, t0)
    pos1, vel1 = integrate_fp32(orc, P, pos0, vel0, rad1)
    ref1 = collide_step(orc, P, pos1, vel1, rad1)
    rad2, branch, margin = actuate(P, rad1, phase, dead, ref1["fa"], ref1["fr"], t1)
    return {"P": P, "n": n, "pos0": pos0, "vel0": vel0, "rad0": rad0, "phase": phase, "dead": dead, "absA0": absA0,
            "absR0": absR0, "rad1": rad1, "pos1": pos1, "vel1": vel1, "ref1": ref1, "t1": t1, "rad2": rad2,
            "branch": branch, "margin": margin}


# ------------------------------------------------------------------------------------------------------------
# the yardstick: the reference's own fp32 builds against float64 (tests/golden/stream_step/yardstick.json)
# ------------------------------------------------------------------------------------------------------------
OUTPUTS = ("vel", "fa", "fr")


def measure_step_yardstick(orc, name):
    """per output: the largest (max, p99) relative error over the oracle's fp32 builds on the named input"""
    inp = step_input(name)
    ref = inp["ref"]
    keep = ~ref["excluded"]
    out = {k: {"max": 0.0, "p99": 0.0} for k in OUTPUTS}
    for b in BUILDS:
        v, fa, fr = collide_fp32(orc, inp["P"], inp["pos1"], inp["vel1"], inp["rad"], b)
        err = step_errors(ref, v, fa, fr)
        for k in OUTPUTS:
            mx, p99 = stats(err[k], keep)
            out[k]["max"], out[k]["p99"] = max(out[k]["max"], mx), max(out[k]["p99"], p99)
    out["n"], out["excluded"] = int(inp["n"]), int(ref["excluded"].sum())
    return out


def measure_actuation_yardstick(orc, cc):
    inp = actuation_input(cc)
    keep = inp["margin"] > DELTA_REL
    rmax = _f(inp["P"].max_radius)
    out = {"rad": {"max": 0.0, "p99": 0.0}}
    for b in BUILDS:
        _, fa, fr = collide_fp32(orc, inp["P"], inp["pos1"], inp["vel1"], inp["rad1"], b)
        rad2 = actuate_fp32(orc, inp["P"], inp["rad1"], inp["phase"], inp["dead"], fa, fr, inp["t1"], b)
        mx, p99 = stats(np.abs(rad2.astype(np.float64) - inp["rad2"]) / rmax, keep)
        out["rad"]["max"], out["rad"]["p99"] = max(out["rad"]["max"], mx), max(out["rad"]["p99"], p99)
    out["n"], out["excluded"] = int(inp["n"]), int((~keep).sum())
    return out


def measure_yardstick(orc):
    return {"step": {name: measure_step_yardstick(orc, name) for name in STEP_INPUTS},
            "actuation": {f"cc{cc}": measure_actuation_yardstick(orc, cc) for cc in (0, 1)}}
