"""numpy-only reference of the pair correlations (pbSimPairCorrelation, csrc/pb_correlate.hip): a brute force over all
O(n^2) pairs, one row of partners at a time, every float32 operation in the order include/particlebot_hip.h states it.

    node:      position and radius finite (as in pbSimRadialCounts)
    velocity:  a = (rint(vx * 2^20), rint(vy * 2^20)),  measured iff node, |vx| < 2048 and |vy| < 2048
    displacement: dx = x_now - x_mark, dy likewise;  a = (rint(dx * 2^20), rint(dy * 2^20)),  measured iff node,
               |dx| < 2048 and |dy| < 2048
    radius:    a = (rint(rad * 2^20), 0),  measured iff node and |rad| < 2048
    rx = xj - xi;  ry = yj - yi;  dist = sqrt(rx*rx + ry*ry);  scale = float32(bins) / float32(rMax)
    the ordered pair (i, j), i != j, both measured, is in bin trunc(dist * scale) iff fl(dist * scale) < bins
    per bin:   pairs,  dot = sum (ax_i ax_j + ay_i ay_j),  ax = sum ax_i,  ay = sum ay_i
The products are int64 (|a| < 2^31, so |ax_i ax_j + ay_i ay_j| < 2^63); the bin sums are accumulated as low and high
32-bit parts with np.add.at and composed into Python ints.  For verification only: O(n^2) time."""
import numpy as np

f32 = np.float32
TWO20 = f32(1048576.0)
LIMIT = f32(2048.0)
KINDS = {"velocity": 0, "displacement": 1, "radius": 2}


def q20(v):
    """rint(float32(v * 2^20)) as int64, 0 where v is not below 2048 in magnitude."""
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        ok = np.abs(v) < LIMIT
        return np.where(ok, np.rint((np.where(ok, v, f32(0)) * TWO20).astype(f32)), 0).astype(np.int64)


def nodes(pos, rad):
    pos = np.asarray(pos, f32).reshape(-1, 2)
    return np.isfinite(pos).all(axis=1) & np.isfinite(np.asarray(rad, f32))


def vector_of(kind, pos, vel, rad, pos0=None):
    """(a int64 (n, 2), measured bool[n]) of one member's state; pos0: the marked positions, for displacements."""
    kind = KINDS.get(kind, kind)
    pos = np.asarray(pos, f32).reshape(-1, 2)
    rad = np.asarray(rad, f32)
    if kind == 0:
        f = np.asarray(vel, f32).reshape(-1, 2)
    elif kind == 1:
        with np.errstate(all="ignore"):
            f = pos - np.asarray(pos0, f32).reshape(-1, 2)
        assert f.dtype == f32
    elif kind == 2:
        f = np.stack([rad, np.zeros_like(rad)], axis=1)
    else:
        raise ValueError(kind)
    with np.errstate(all="ignore"):
        measured = nodes(pos, rad) & (np.abs(f[:, 0]) < LIMIT) & (np.abs(f[:, 1]) < LIMIT)
    a = np.stack([q20(f[:, 0]), q20(f[:, 1])], axis=1)
    a[~measured] = 0
    return a, measured


def normalised(v):
    """(lo, hi) with v = hi * 2^32 + lo, 0 <= lo < 2^32, hi the floor quotient."""
    v = int(v)
    return v & 0xFFFFFFFF, v >> 32


def correlate(pos, a, measured, r_max, bins):
    """A dict of lists of Python ints, one entry per bin (pairs, dot, ax, ay), and `totals`: measured, sum_ax, sum_ay,
    sum_a2 and pairs.  Only measured bots take part; they are nodes by construction (vector_of)."""
    pos = np.asarray(pos, f32).reshape(-1, 2)
    a = np.asarray(a, np.int64).reshape(-1, 2)
    measured = np.asarray(measured, bool)
    bins = int(bins)
    with np.errstate(all="ignore"):
        scale = f32(bins) / f32(r_max)
    pairs = np.zeros(bins, np.int64)
    dlo, dhi = np.zeros(bins, np.int64), np.zeros(bins, np.int64)
    sax, say = np.zeros(bins, np.int64), np.zeros(bins, np.int64)
    for i in np.flatnonzero(measured):
        with np.errstate(all="ignore"):
            rx = pos[:, 0] - pos[i, 0]
            ry = pos[:, 1] - pos[i, 1]
            dist = np.sqrt(rx * rx + ry * ry)
            fb = (dist * scale).astype(f32)
            hit = measured & (fb < f32(bins))  # NaN: not counted
        hit[i] = False
        b = fb[hit].astype(np.int64)
        d = a[i, 0] * a[hit, 0] + a[i, 1] * a[hit, 1]
        assert d.dtype == np.int64
        np.add.at(pairs, b, 1)
        np.add.at(dlo, b, d & 0xFFFFFFFF)
        np.add.at(dhi, b, d >> 32)
        np.add.at(sax, b, a[i, 0])
        np.add.at(say, b, a[i, 1])
    am = a[measured]
    totals = {"measured": int(measured.sum()), "sum_ax": int(am[:, 0].sum()), "sum_ay": int(am[:, 1].sum()),
              "sum_a2": sum(int(x) * int(x) + int(y) * int(y) for x, y in am), "pairs": int(pairs.sum())}
    return {"pairs": [int(v) for v in pairs], "dot": [(int(h) << 32) + int(l) for h, l in zip(dhi, dlo)],
            "ax": [int(v) for v in sax], "ay": [int(v) for v in say], "totals": totals}


def pair_correlation(kind, pos, vel, rad, r_max, bins, pos0=None):
    a, measured = vector_of(kind, pos, vel, rad, pos0)
    return correlate(pos, a, measured, r_max, bins)


def rows_of(ref, dtype):
    """The reference's bins as the structured array the library returns (normalised 128-bit fields)."""
    out = np.zeros(len(ref["pairs"]), dtype)
    out["pairs"] = ref["pairs"]
    for name in ("dot", "ax", "ay"):
        for b, v in enumerate(ref[name]):
            lo, hi = normalised(v)
            out[name + "_lo"][b], out[name + "_hi"][b] = lo, hi
    return out
