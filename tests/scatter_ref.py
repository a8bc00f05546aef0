"""Reference for the self-intermediate scattering function (pbSimSetScattering / pbSimGetScattering,
csrc/pb_scatter.hip): the series' quantisation (tests/series_ref.py) for the positions, the structure factor's index
(tests/sfactor_ref.py) applied to the uint32 difference of the quantised positions, the table from pb.phasor_table(),
Python ints for every sum, so that each figure is exact and can be compared with the device's with ==.
include/particlebot_hip.h has the definitions."""
import numpy as np

import series_ref as SR
import sfactor_ref as KR

f32 = np.float32
FIELDS = ("lag", "nx", "ny", "origins", "sum_steps", "samples", "re", "im")
UNIT = KR.UNIT


def snapshot(pos):
    """What a record stores of one member's positions (n, 2): (qx, qy, measured) as int64, int64 and bool arrays; a bot
    whose x or y is out of range is unmeasured."""
    pos = np.asarray(pos, f32).reshape(-1, 2)
    qx, okx = SR.quantise(pos[:, 0])
    qy, oky = SR.quantise(pos[:, 1])
    return np.array(qx, np.int64), np.array(qy, np.int64), okx & oky


def pair(now, then, vectors, box_log2):
    """What one pair of snapshots adds to a lag: (samples, [(re, im) per vector]) as Python ints."""
    (xn, yn, okn), (xt, yt, okt) = now, then
    ok = okn & okt
    dx, dy = (xn - xt)[ok], (yn - yt)[ok]  # |.| < 2^32: sfactor_ref.index takes them mod 2^32
    tab = KR.table().astype(np.int64)
    sums = []
    for nx, ny in np.asarray(vectors).reshape(-1, 2).tolist():
        idx = KR.index(nx, ny, dx, dy, box_log2)
        sums.append((int(tab[idx, 0].sum()), int(tab[idx, 1].sum())))  # fewer than 2^28 entries of at most 2^30
    return int(ok.sum()), sums


def table(records, steps, lags, vectors, box_log2):
    """The rows of one member after the records `records` (positions (n, 2), or tuples that start with them, in the
    order taken) with pbSimStats.steps `steps` per record: per lag a list over the vectors of dicts of Python ints, as
    Sim.scattering() returns one member.  Record r is paired with the records r - l for l = 0 ... min(r, lags - 1)."""
    vectors = np.asarray(vectors).reshape(-1, 2).tolist()
    snaps = [snapshot(r[0] if isinstance(r, (tuple, list)) else r) for r in records]
    rows = [[dict(dict.fromkeys(FIELDS, 0), lag=l, nx=int(nx), ny=int(ny)) for nx, ny in vectors] for l in range(lags)]
    for r in range(len(snaps)):
        for l in range(min(r, lags - 1) + 1):
            samples, sums = pair(snaps[r], snaps[r - l], vectors, box_log2)
            for row, (re, im) in zip(rows[l], sums):
                row["origins"] += 1
                row["sum_steps"] += int(steps[r]) - int(steps[r - l])
                row["samples"] += samples
                row["re"] += re
                row["im"] += im
    return rows
