"""Reference for the coherent intermediate scattering function (pbSimSetCoherent / pbSimGetCoherent,
csrc/pb_coherent.hip): the series' quantisation (tests/series_ref.py) for the positions, the structure factor's index
(tests/sfactor_ref.py), the table from pb.phasor_table(), Python ints for every mode, product and sum, so that each
figure is exact and can be compared with the device's with ==.  include/particlebot_hip.h has the definitions."""
import numpy as np

import series_ref as SR
import sfactor_ref as KR

f32 = np.float32
FIELDS = ("lag", "nx", "ny", "origins", "sum_steps", "bots_now", "bots_then", "re", "im")
UNIT = 1 << 60  # a product of two modes in units of 2^-30


def modes(pos, vectors, box_log2):
    """What a record stores of one member's positions (n, 2): (measured, [(C, S) per vector]) as Python ints; a bot
    whose x or y is out of range is unmeasured and adds nothing."""
    pos = np.asarray(pos, f32).reshape(-1, 2)
    qx, okx = SR.quantise(pos[:, 0])
    qy, oky = SR.quantise(pos[:, 1])
    ok = okx & oky
    qx, qy = np.array(qx, np.int64)[ok], np.array(qy, np.int64)[ok]
    tab = KR.table().astype(np.int64)
    out = []
    for nx, ny in np.asarray(vectors).reshape(-1, 2).tolist():
        idx = KR.index(nx, ny, qx, qy, box_log2)
        out.append((int(tab[idx, 0].sum()), int(tab[idx, 1].sum())))  # fewer than 2^28 entries of at most 2^30
    return int(ok.sum()), out


def pair(now, then):
    """What one pair of records adds to a lag: (bots_now, bots_then, [(re, im) per vector]): rho_now conj(rho_then)."""
    (mn, vn), (mt, vt) = now, then
    return mn, mt, [(cn * ct + sn * st, sn * ct - cn * st) for (cn, sn), (ct, st) in zip(vn, vt)]


def table_of_modes(recs, steps, lags, vectors):
    """The rows of one member from its records' modes `recs` (each what modes() returns), with pbSimStats.steps `steps`
    per record: per lag a list over the vectors of dicts of Python ints, as Sim.coherent_scattering() returns one member.
    Record r is paired with the records r - l for l = 0 ... min(r, lags - 1)."""
    vectors = np.asarray(vectors).reshape(-1, 2).tolist()
    rows = [[dict(dict.fromkeys(FIELDS, 0), lag=l, nx=int(nx), ny=int(ny)) for nx, ny in vectors] for l in range(lags)]
    for r in range(len(recs)):
        for l in range(min(r, lags - 1) + 1):
            bots_now, bots_then, sums = pair(recs[r], recs[r - l])
            for row, (re, im) in zip(rows[l], sums):
                row["origins"] += 1
                row["sum_steps"] += int(steps[r]) - int(steps[r - l])
                row["bots_now"] += bots_now
                row["bots_then"] += bots_then
                row["re"] += re
                row["im"] += im
    return rows


def table(records, steps, lags, vectors, box_log2):
    """table_of_modes() of the records `records` (positions (n, 2), or tuples that start with them, in the order taken)."""
    recs = [modes(r[0] if isinstance(r, (tuple, list)) else r, vectors, box_log2) for r in records]
    return table_of_modes(recs, steps, lags, vectors)


def limbs(value):
    """The three little-endian 64-bit limbs of a signed value as a 192-bit two's-complement word."""
    assert -(1 << 191) <= value < 1 << 191
    v = value & ((1 << 192) - 1)
    return [v & 0xFFFFFFFFFFFFFFFF, (v >> 64) & 0xFFFFFFFFFFFFFFFF, v >> 128]
