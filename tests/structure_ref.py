"""numpy-only reference of the structure analysis (pbSimRadialCounts / pbSimStructureStats / pbSimHexaticOf,
csrc/pb_structure.hip): a brute force over all O(n^2) pairs, every operation in float32 in the order
include/particlebot_hip.h states it.

    rx = xj - xi;  ry = yj - yi;  dist = sqrt(rx*rx + ry*ry)
    radial:  scale = float32(bins) / float32(rMax);  b = trunc(dist * scale), counted iff b < bins  (ordered pairs)
    bond:    (dist - (ri + rj)) < gap;  for dist > 0
             ux = rx / dist;  uy = ry / dist
             c2 = ux*ux - uy*uy;  s2 = (ux*uy) + (ux*uy);  c4 = c2*c2 - s2*s2;  s4 = (c2*s2) + (c2*s2)
             c6 = c4*c2 - s4*s2;  s6 = s4*c2 + c4*s2;      q = int64(rint(float32(c * 2^30)))
A bot with a non-finite position or radius takes part in nothing.  numpy rounds every float32 operation on its own (it
never contracts a*b - c*d), sums are int64, the histogram is built with np.add.at."""
import numpy as np

f32 = np.float32
TWO30 = f32(1073741824.0)


def _state(pos, rad):
    pos = np.asarray(pos, f32).reshape(-1, 2)
    rad = np.asarray(rad, f32)
    ok = np.isfinite(pos).all(axis=1) & np.isfinite(rad)
    return pos, rad, ok


def _row(pos, ok, i):
    """rx, ry, dist from bot i to every bot (float32) and the mask of partners."""
    with np.errstate(all="ignore"):
        rx = pos[:, 0] - pos[i, 0]
        ry = pos[:, 1] - pos[i, 1]
        dist = np.sqrt(rx * rx + ry * ry)
    partner = ok.copy()
    partner[i] = False
    return rx, ry, dist, partner


def radial_counts(pos, rad, r_max, bins):
    """uint64[bins]: ordered pairs per bin."""
    pos, rad, ok = _state(pos, rad)
    bins = int(bins)
    with np.errstate(all="ignore"):
        scale = f32(bins) / f32(r_max)
    counts = np.zeros(bins, np.int64)
    for i in np.flatnonzero(ok):
        _, _, dist, partner = _row(pos, ok, i)
        with np.errstate(all="ignore"):
            fb = (dist * scale).astype(f32)
            hit = partner & (fb < f32(bins))  # trunc(fb) < bins, the same decision for every finite fb; NaN: not counted
        np.add.at(counts, fb[hit].astype(np.int64), 1)
    return counts.astype(np.uint64)


def q30(v):
    return np.rint((np.asarray(v, f32) * TWO30).astype(f32)).astype(np.int64)


def bond_terms(rx, ry, dist):
    """(qre, qim) int64 of bonds with dist > 0, from float32 arrays."""
    with np.errstate(all="ignore"):
        ux = rx / dist
        uy = ry / dist
        c2 = ux * ux - uy * uy
        s2 = (ux * uy) + (ux * uy)
        c4 = c2 * c2 - s2 * s2
        s4 = (c2 * s2) + (c2 * s2)
        c6 = c4 * c2 - s4 * s2
        s6 = s4 * c2 + c4 * s2
    for a in (ux, uy, c2, s2, c4, s4, c6, s6):
        assert a.dtype == f32
    return q30(c6), q30(s6)


def hexatic_sums(pos, rad, gap):
    """(Sre int64[n], Sim int64[n], neighbours uint32[n])."""
    pos, rad, ok = _state(pos, rad)
    n = rad.size
    sre, sim, nb = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.uint32)
    for i in np.flatnonzero(ok):
        rx, ry, dist, partner = _row(pos, ok, i)
        with np.errstate(all="ignore"):
            bonded = partner & ((dist - (rad[i] + rad)) < f32(gap))
        nb[i] = int(bonded.sum())
        turn = bonded & (dist > 0)
        if turn.any():
            qre, qim = bond_terms(rx[turn], ry[turn], dist[turn])
            sre[i], sim[i] = int(qre.sum()), int(qim.sum())
    return sre, sim, nb


def psi6_of(sre, sim, nb):
    """The public per-bot value, float64 (n, 2): ((double)S / 2^30) / (double)neighbours, (0, 0) without neighbours."""
    out = np.zeros((len(nb), 2), np.float64)
    has = np.asarray(nb) > 0
    d = np.asarray(nb, np.float64)[has]
    out[has, 0] = (np.asarray(sre, np.int64)[has].astype(np.float64) / 1073741824.0) / d
    out[has, 1] = (np.asarray(sim, np.int64)[has].astype(np.float64) / 1073741824.0) / d
    return out


def stats_of(sre, sim, nb):
    """The member's pbStructureStats row as a dict of Python integers."""
    nb = np.asarray(nb, np.int64)
    return {"bonds": int(nb.sum()), "psi6_re": int(np.asarray(sre, np.int64).sum()),
            "psi6_im": int(np.asarray(sim, np.int64).sum()),
            "coordination": np.bincount(np.minimum(nb, 7), minlength=8).tolist()}


def analyse(pos, rad, gap):
    """(stats dict, psi6 float64 (n, 2), neighbours uint32[n]) of one member's state."""
    sre, sim, nb = hexatic_sums(pos, rad, gap)
    return stats_of(sre, sim, nb), psi6_of(sre, sim, nb), nb
