"""Reference for the self van Hove function (pbSimSetVanHove / pbSimGetVanHove, csrc/pb_vanhove.hip): numpy fp32 for the
differences, the scaling and the measured test, Python ints for everything else, so that each figure is exact and can be
compared with the device's with ==.  It follows include/particlebot_hip.h's definitions literally: the edges are
(k * qw) ** 2 capped at 2^63, the radial bin is a bisect in them, the axis bin is a floor division."""
from bisect import bisect_right

import numpy as np

f32 = np.float32
SCALE = f32(1048576.0)  # 2^20
BOUND = f32(2048.0)
CAP = 1 << 63
MOMENTS = ("samples", "beyond_r", "beyond_x", "beyond_y", "msd", "q4")
FIELDS = ("lag", "origins", "sum_steps") + MOMENTS


def qw_of(width):
    """rint(width * 2^20) in fp32, as the host forms it once."""
    return int(np.rint(f32(width) * SCALE))


def edges_of(qw, bins):
    """E_k = min((k qw)^2, 2^63) for k = 0 ... bins."""
    return [min((k * qw) ** 2, CAP) for k in range(bins + 1)]


def quantised_pairs(now, then):
    """(qx, qy) as Python ints of the measured bots of one pair of snapshots (pos (n, 2) each)."""
    pn, pt = (np.asarray(p, f32).reshape(-1, 2) for p in (now, then))
    with np.errstate(invalid="ignore"):
        d = pn - pt                        # fp32; inf - inf and NaN - x are NaN, inf - x is inf: all fail the bound
        ok = (np.abs(d) < BOUND).all(1)    # NaN and the infinities fail the comparison
    q = np.rint(np.where(ok[:, None], d, f32(0.0)) * SCALE).astype(np.int64)
    return [(int(x), int(y)) for x, y in q[ok]]


def empty_row(lag, bins):
    row = dict.fromkeys(FIELDS, 0)
    row["lag"] = lag
    row["radial"], row["x"], row["y"] = [0] * bins, [0] * (2 * bins), [0] * (2 * bins)
    return row


def add_pair(row, qx, qy, qw, bins, edges):
    """One measured pair into a lag's row."""
    s = qx * qx + qy * qy
    row["samples"] += 1
    row["msd"] += s
    row["q4"] += s * s
    if s < edges[bins]:
        row["radial"][bisect_right(edges, s) - 1] += 1  # max{k : E_k <= s}; an edge belongs to the upper bin
    else:
        row["beyond_r"] += 1
    for name, q in (("x", qx), ("y", qy)):
        b = q // qw  # floor towards minus infinity
        if -bins <= b < bins:
            row[name][b + bins] += 1
        else:
            row["beyond_" + name] += 1


def table(records_pos, steps, lags, width, bins):
    """The rows of one member after the records `records_pos` (a list of pos arrays (n, 2), in the order taken) with
    pbSimStats.steps `steps` per record: a list of `lags` dicts, lag 0 first, as Sim.van_hove() gives them.  Record r is
    paired with the records r - l for l = 0 ... min(r, lags - 1)."""
    qw = qw_of(width)
    edges = edges_of(qw, bins)
    rows = [empty_row(l, bins) for l in range(lags)]
    for r in range(len(records_pos)):
        for l in range(min(r, lags - 1) + 1):
            row = rows[l]
            row["origins"] += 1
            row["sum_steps"] += int(steps[r]) - int(steps[r - l])
            for qx, qy in quantised_pairs(records_pos[r], records_pos[r - l]):
                add_pair(row, qx, qy, qw, bins, edges)
    return rows


def identities_hold(row):
    return (sum(row["radial"]) + row["beyond_r"] == row["samples"] and sum(row["x"]) + row["beyond_x"] == row["samples"]
            and sum(row["y"]) + row["beyond_y"] == row["samples"])
