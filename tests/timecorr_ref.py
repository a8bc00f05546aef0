"""Reference for the time correlations (pbSimSetTimeCorrelation / pbSimGetTimeCorrelation, csrc/pb_timecorr.hip): numpy
fp32 for the differences, the scaling and the measured test, Python ints for every sum, so that each figure is exact and
can be compared with the device's with ==.  include/particlebot_hip.h has the definitions."""
import numpy as np

f32 = np.float32
SCALE = f32(1048576.0)  # 2^20
BOUND = f32(2048.0)
FIELDS = ("lag", "origins", "sum_steps", "samples", "sum_qx", "sum_qy", "msd", "vacf", "overlap", "max_q2")


def _below(a):
    with np.errstate(invalid="ignore"):
        return np.abs(a) < BOUND  # NaN and the infinities fail the comparison


def _quantise(a, ok):
    """rint(a * 2^20) in fp32 (exact scaling, ties to even) as int64 where ok, 0 elsewhere."""
    return np.rint(np.where(ok, a, f32(0.0)) * SCALE).astype(np.int64)


def a2_of(overlap_radius):
    """qa * qa with qa = rint(overlapRadius * 2^20) in fp32, as the host forms it once."""
    qa = int(np.rint(f32(overlap_radius) * SCALE))
    return qa * qa


def pair(now, then, a2):
    """The sums one pair of snapshots (pos (n, 2), vel (n, 2)) each adds to a cell: a dict of Python ints."""
    (pn, vn), (pt, vt) = ((np.asarray(p, f32).reshape(-1, 2), np.asarray(v, f32).reshape(-1, 2)) for p, v in (now, then))
    with np.errstate(invalid="ignore"):
        d = pn - pt  # fp32; inf - inf and NaN - x are NaN, inf - x is inf: all fail the bound
    ok = _below(d).all(1) & _below(vn).all(1) & _below(vt).all(1)
    keep = ok[:, None]
    q, wn, wt = _quantise(d, keep), _quantise(vn, keep), _quantise(vt, keep)
    s = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1])[ok]            # below 2^63: int64 holds it
    p = (wn[:, 0] * wt[:, 0] + wn[:, 1] * wt[:, 1])[ok]        # |p| below 2^63
    s, p = [int(v) for v in s], [int(v) for v in p]
    return {"samples": len(s), "sum_qx": sum(int(v) for v in q[ok, 0]), "sum_qy": sum(int(v) for v in q[ok, 1]),
            "msd": sum(s), "vacf": sum(p), "overlap": sum(1 for v in s if v < a2), "max_q2": max(s, default=0)}


def table(snapshots, steps, lags, overlap_radius):
    """The rows of one member after the records `snapshots` (a list of (pos, vel), in the order taken) with
    pbSimStats.steps `steps` per record: a list of `lags` dicts of Python ints, lag 0 first.  Record r is paired with
    the records r - l for l = 0 ... min(r, lags - 1)."""
    a2 = a2_of(overlap_radius)
    rows = [dict.fromkeys(FIELDS, 0) for _ in range(lags)]
    for l, row in enumerate(rows):
        row["lag"] = l
    for r in range(len(snapshots)):
        for l in range(min(r, lags - 1) + 1):
            row, add = rows[l], pair(snapshots[r], snapshots[r - l], a2)
            row["origins"] += 1
            row["sum_steps"] += int(steps[r]) - int(steps[r - l])
            for k in ("samples", "sum_qx", "sum_qy", "msd", "vacf", "overlap"):
                row[k] += add[k]
            row["max_q2"] = max(row["max_q2"], add["max_q2"])
    return rows
