"""Reference for the bond recorder (pbSimSetBondDynamics / pbSimGetBondDynamics, csrc/pb_bonds.hip): the link network of
the present bots from tests/contacts_ref.py's topology (CSR in original order, a bot's entries ascending), the quantised
positions from tests/scatter_ref.py's snapshot, NumPy int64 for what fits and Python ints for every square and every sum
over origins, so that each figure is exact and can be compared with the device's with ==.  include/particlebot_hip.h has
the definitions."""
import numpy as np

import contacts_ref as KR
import scatter_ref as XR

f32 = np.float32
WIDTH = 8
SCALARS = ("origins", "sum_steps", "samples", "crowded", "bonds_then", "bonds_now", "bonds_kept", "bots_unchanged",
           "bots_lost", "bots_gained", "plain_q2")
LISTS = ("cage_samples", "cage_overlap", "cage_q2")
FIELDS = ("lag",) + SCALARS + LISTS


def qa_of(overlap_radius):
    """qa = rint(overlapRadius * 2^20) in fp32, as the host forms it once."""
    return int(np.rint(f32(overlap_radius) * f32(1048576.0)))


def present(pos, rad, max_radius):
    """The presence rule: |x|, |y| < 2048 (a NaN or an infinity fails) and the radius finite and <= maxRadius."""
    rad = np.asarray(rad, f32).reshape(-1)
    qx, qy, ok = XR.snapshot(pos)
    with np.errstate(invalid="ignore"):
        return ok & np.isfinite(rad) & (rad <= f32(max_radius))


def snapshot(pos, rad, gap, max_radius):
    """What a record stores of one member: (qx, qy int64, here bool, degree int64, neighbours: a list per bot of the
    ascending original indices of ALL its neighbours; an absent bot has none and is nobody's neighbour)."""
    pos = np.array(pos, f32).reshape(-1, 2)
    rad = np.array(rad, f32).reshape(-1)
    qx, qy, _ = XR.snapshot(pos)
    here = present(pos, rad, max_radius)
    pos[~here] = np.nan  # no link reaches a bot without a position; its radius must not shape the search either
    rad[~here] = 0.0
    offsets, owner, other = KR.topology(pos, rad, f32(gap))
    offsets = offsets.astype(np.int64)
    neighbours = [[int(j) for j in other[offsets[i]:offsets[i + 1]]] for i in range(rad.size)]
    assert all(here[i] and all(here[j] for j in nb) for i, nb in enumerate(neighbours) if nb)
    return qx, qy, here, np.diff(offsets), neighbours


def empty_row(lag):
    row = dict.fromkeys(SCALARS, 0)
    row.update(lag=lag, cage_samples=[0] * WIDTH, cage_overlap=[0] * WIDTH, cage_q2=[0] * WIDTH)
    return row


def pair(row, now, then, qa):
    """Adds what one pair of snapshots (then = the earlier one) adds to a lag's row."""
    (xn, yn, hn, dn, nn), (xt, yt, ht, dt, nt) = now, then
    both = hn & ht
    crowded = both & ((dn > WIDTH) | (dt > WIDTH))
    row["crowded"] += int(crowded.sum())
    dx, dy = xn - xt, yn - yt  # int64, below 2^32 in magnitude
    for i in np.flatnonzero(both & ~crowded).tolist():
        a, b = nt[i], nn[i]
        t, w, kept = len(a), len(b), len(set(a) & set(b))
        row["samples"] += 1
        row["bonds_then"] += t
        row["bonds_now"] += w
        row["bonds_kept"] += kept
        row["bots_unchanged"] += int(kept == t and kept == w)
        row["bots_lost"] += int(kept < t)
        row["bots_gained"] += int(kept < w)
        if t == 0 or not all(hn[j] for j in a):
            continue
        cx = t * int(dx[i]) - sum(int(dx[j]) for j in a)
        cy = t * int(dy[i]) - sum(int(dy[j]) for j in a)
        if abs(cx) >= 1 << 31 or abs(cy) >= 1 << 31:
            continue
        s = cx * cx + cy * cy
        row["cage_samples"][t - 1] += 1
        row["cage_overlap"][t - 1] += int(s < (t * qa) ** 2)
        row["cage_q2"][t - 1] += s
        row["plain_q2"] += int(dx[i]) ** 2 + int(dy[i]) ** 2


def table(records, radii, steps, lags, gap, max_radius, overlap_radius):
    """The rows of one member after the records `records` (positions (n, 2), in the order taken) with radii `radii` (one
    array for all records, or one per record) and pbSimStats.steps `steps` per record: per lag a dict of Python ints, as
    Sim.bond_dynamics() returns one member.  Record r is paired with the records r - l for l = 0 ... min(r, lags - 1)."""
    qa = qa_of(overlap_radius)
    per_record = isinstance(radii, (list, tuple))
    snaps = [snapshot(p, radii[r] if per_record else radii, gap, max_radius) for r, p in enumerate(records)]
    rows = [empty_row(l) for l in range(lags)]
    for r in range(len(snaps)):
        for l in range(min(r, lags - 1) + 1):
            rows[l]["origins"] += 1
            rows[l]["sum_steps"] += int(steps[r]) - int(steps[r - l])
            pair(rows[l], snaps[r], snaps[r - l], qa)
    return rows
