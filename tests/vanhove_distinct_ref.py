"""Reference for the distinct van Hove function (pbSimSetVanHoveDistinct / pbSimGetVanHoveDistinct,
csrc/pb_vanhove_distinct.hip): every ordered pair (i at the earlier record, j at the later record) of a member, numpy
fp32 for the differences, the scaling and the range test, int64 for s = qx^2 + qy^2 (below 2^63) and an exact integer
square root for the bin, so that each figure can be compared with the device's with ==.  It follows
include/particlebot_hip.h's definitions literally and knows nothing of cells: all pairs, in blocks of rows.
tests/test_vanhove_distinct_ref.py pins it to a plain Python-int loop that bisects in vanhove_ref.edges_of."""
import numpy as np

import vanhove_ref as VR

f32 = np.float32
FIELDS = ("lag", "origins", "sum_steps", "centres", "partners", "pairs")
ROWS_PER_BLOCK = 256


def present(pos, rad):
    """The filing's rule: x, y and rad all finite."""
    pos, rad = np.asarray(pos, f32).reshape(-1, 2), np.asarray(rad, f32).reshape(-1)
    return np.isfinite(pos).all(1) & np.isfinite(rad)


def isqrt64(s):
    """floor(sqrt(s)) of an int64 array with 0 <= s < 2^63, exact: the fp64 root corrected by comparing squares."""
    r = np.sqrt(s.astype(np.float64)).astype(np.int64)
    r -= (r * r > s)
    r += ((r + 1) * (r + 1) <= s)
    assert ((r * r <= s) & ((r + 1) * (r + 1) > s)).all()
    return r


def counted_pairs(now, then, qw, bins):
    """Of two records (pos, rad): the arrays i, j and bin of every counted ordered pair, i the original index at the
    earlier record `then`, j at the later record `now`."""
    (pn, rn), (pt, rt) = now, then
    pn, pt = (np.asarray(p, f32).reshape(-1, 2) for p in (pn, pt))
    on_now, on_then = present(pn, rn), present(pt, rt)
    n = len(pn)
    limit = (bins * qw) ** 2
    out = ([], [], [])
    for lo in range(0, n, ROWS_PER_BLOCK):
        rows = np.arange(lo, min(lo + ROWS_PER_BLOCK, n))
        with np.errstate(invalid="ignore"):
            dx = pn[None, :, 0] - pt[rows, None, 0]  # fp32: x_j(now) - x_i(then)
            dy = pn[None, :, 1] - pt[rows, None, 1]
            ok = (np.abs(dx) < VR.BOUND) & (np.abs(dy) < VR.BOUND)
        ok &= on_then[rows, None] & on_now[None, :] & (rows[:, None] != np.arange(n)[None, :])
        i, j = np.nonzero(ok)
        qx = np.rint(dx[i, j] * VR.SCALE).astype(np.int64)
        qy = np.rint(dy[i, j] * VR.SCALE).astype(np.int64)
        s = qx * qx + qy * qy
        keep = s < limit
        out[0].append(rows[i[keep]]), out[1].append(j[keep]), out[2].append(isqrt64(s[keep]) // qw)
    return tuple(np.concatenate(a) if a else np.zeros(0, np.int64) for a in out)


def empty_row(lag, bins):
    row = dict.fromkeys(FIELDS, 0)
    row["lag"] = lag
    row["counts"] = [0] * bins
    return row


def table(records, steps, lags, width, bins):
    """The rows of one member after `records` (a list of (pos (n, 2), rad (n,)), in the order taken) with pbSimStats.steps
    `steps` per record: a list of `lags` dicts, lag 0 first, as Sim.van_hove_distinct() gives them."""
    qw = VR.qw_of(width)
    assert qw >= 1 and qw * bins < 1 << 31
    rows = [empty_row(l, bins) for l in range(lags)]
    for r in range(len(records)):
        for l in range(min(r, lags - 1) + 1):
            row = rows[l]
            row["origins"] += 1
            row["sum_steps"] += int(steps[r]) - int(steps[r - l])
            row["centres"] += int(present(*records[r - l]).sum())
            row["partners"] += int(present(*records[r]).sum())
            _, _, b = counted_pairs(records[r], records[r - l], qw, bins)
            hist = np.bincount(b, minlength=bins)
            row["counts"] = [c + int(h) for c, h in zip(row["counts"], hist)]
            row["pairs"] += int(hist.sum())
    return rows


# ---- what a walk around the bot's CURRENT position would have missed ---------------------------------------------------

def grid_of(n, width, bins):
    """The filing's grid for a member of n bots at rMax = bins * quantised width: (edge, columns, rows)."""
    bits = 4
    while (1 << bits) < n:
        bits += 1
    edge = max(VR.qw_of(width) * bins / 2.0 ** 20 * (1.0 + 1.0 / 1024.0), 1.0 / 256.0)
    return edge, 1 << ((bits + 1) // 2), 1 << (bits // 2)


def missed_around_the_current_position(now, then, width, bins):
    """How many counted pairs (i then, j now) have j outside the nine cells around where i is NOW: the pairs a sweep
    centred on the bot's current position would not meet (an i that is absent now has no current cell: all of its pairs
    count)."""
    qw = VR.qw_of(width)
    i, j, _ = counted_pairs(now, then, qw, bins)
    pn = np.asarray(now[0], f32).reshape(-1, 2)
    edge, gx, gy = grid_of(len(pn), width, bins)
    here = present(*now)
    with np.errstate(invalid="ignore"):
        cell = np.floor(np.where(here[:, None], pn, f32(0.0)).astype(np.float64) / edge).astype(np.int64)
    ddx = (cell[j, 0] - cell[i, 0]) % gx
    ddy = (cell[j, 1] - cell[i, 1]) % gy
    near = ((ddx <= 1) | (ddx == gx - 1)) & ((ddy <= 1) | (ddy == gy - 1)) & here[i]
    return int((~near).sum())
