"""Reference for the time series (pbSimMoments / pbSimSetSeries, csrc/pb_moments.hip): numpy fp32 for the scaling and
the measured test, Python ints for every sum, so that each figure is exact and can be compared with the device's with
==.  include/particlebot_hip.h has the definitions."""
import numpy as np

f32 = np.float32
SCALE = f32(1048576.0)  # 2^20
BOUND = f32(2048.0)
SUMS = ("sum_qx", "sum_qy", "sum_qr", "sum_wx", "sum_wy")
BOX = ("min_qx", "max_qx", "min_qy", "max_qy")
SQUARES = ("xx", "yy", "xy", "rr", "vv")
FIELDS = ("measured",) + SUMS + BOX + SQUARES  # what moments() returns; a device row also carries time and step


def quantise(a):
    """(q as a list of Python ints, ok): q = rint(a * 2^20) in fp32 (exact scaling, ties to even) where fabsf(a) < 2048
    and a is finite; ok says where."""
    a = np.asarray(a, f32)
    with np.errstate(invalid="ignore"):
        ok = np.abs(a) < BOUND  # NaN and the infinities fail the comparison
    q = np.rint(np.where(ok, a, f32(0.0)) * SCALE)  # fp32 throughout
    return [int(v) for v in q.reshape(-1)], ok.reshape(-1)


def moments(pos, vel, rad):
    """The row of one member from its positions (n, 2), velocities (n, 2) and radii (n): a dict of Python ints."""
    pos, vel = np.asarray(pos, f32).reshape(-1, 2), np.asarray(vel, f32).reshape(-1, 2)
    rad = np.asarray(rad, f32).reshape(-1)
    qx, okx = quantise(pos[:, 0])
    qy, oky = quantise(pos[:, 1])
    wx, okwx = quantise(vel[:, 0])
    wy, okwy = quantise(vel[:, 1])
    qr, okr = quantise(rad)
    ok = okx & oky & okwx & okwy & okr
    who = [int(i) for i in np.flatnonzero(ok)]
    row = {"measured": len(who)}
    row["sum_qx"], row["sum_qy"], row["sum_qr"] = (sum(q[i] for i in who) for q in (qx, qy, qr))
    row["sum_wx"], row["sum_wy"] = (sum(q[i] for i in who) for q in (wx, wy))
    row["min_qx"] = min((qx[i] for i in who), default=0)
    row["max_qx"] = max((qx[i] for i in who), default=0)
    row["min_qy"] = min((qy[i] for i in who), default=0)
    row["max_qy"] = max((qy[i] for i in who), default=0)
    row["xx"] = sum(qx[i] * qx[i] for i in who)
    row["yy"] = sum(qy[i] * qy[i] for i in who)
    row["xy"] = sum(qx[i] * qy[i] for i in who)
    row["rr"] = sum(qr[i] * qr[i] for i in who)
    row["vv"] = sum(wx[i] * wx[i] + wy[i] * wy[i] for i in who)
    return row


def gate(t, interval, dt):
    """The schedule's fp32 test t - interval floorf(t / interval) < dt."""
    t, interval, dt = f32(t), f32(interval), f32(dt)
    return bool(f32(t - f32(interval * np.floor(f32(t / interval)))) < dt)


def gate_steps(t0, dt, interval, nsteps, max_time):
    """Replays the fp32 clock of nsteps steps from time t0: the list of (k, t) of the steps that run and in front of
    which a record is taken, k counted from 0 and t the step's fp32 start time.  interval 0: every step that runs.  A
    step whose start time exceeds max_time does not run, nor does any after it."""
    t, dt, out = f32(t0), f32(dt), []
    for k in range(int(nsteps)):
        if t > f32(max_time):
            break
        if float(interval) == 0.0 or gate(t, interval, dt):
            out.append((k, float(t)))
        t = f32(t + dt)
    return out
