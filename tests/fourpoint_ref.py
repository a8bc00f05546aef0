"""Reference for the four-point recorder (pbSimSetFourPoint / pbSimGetFourPoint, csrc/pb_fourpoint.hip): the scattering's
snapshot (tests/scatter_ref.py) for the quantised positions, the overlap of a pair from the difference of the quantised
positions, the structure factor's index (tests/sfactor_ref.py) at the EARLIER position, the table from pb.phasor_table(),
NumPy int64 for the table sums and Python ints for every product and sum over origins, so that each figure is exact and
can be compared with the device's with ==.  include/particlebot_hip.h has the definitions."""
import numpy as np

import scatter_ref as XR
import sfactor_ref as KR

f32 = np.float32
FIELDS = ("lag", "nx", "ny", "origins", "sum_steps", "samples", "overlap", "overlap2", "re", "im", "power")
UNIT = 1 << 30  # a mode in units of 2^-30; power in units of 2^-60


def qa_of(overlap_radius):
    """qa = rint(overlapRadius * 2^20) in fp32, as the host forms it once."""
    return int(np.rint(f32(overlap_radius) * f32(1048576.0)))


def weights(now, then, qa):
    """(measured, overlapping) of one pair of snapshots (each what scatter_ref.snapshot returns): two bool arrays."""
    (xn, yn, okn), (xt, yt, okt) = now, then
    ok = okn & okt
    dx, dy = np.abs(xn - xt), np.abs(yn - yt)  # below 2^32: the squares would not fit int64, so the near test comes first
    near = ok & (dx < qa) & (dy < qa)
    s = np.where(near, dx, 0) ** 2 + np.where(near, dy, 0) ** 2  # each below 2^62
    return ok, near & (s < qa * qa)


def pair(now, then, vectors, box_log2, qa):
    """What one origin pair is: (m, Q, [(A, B) per vector]) as Python ints."""
    ok, w = weights(now, then, qa)
    xt, yt = then[0][w], then[1][w]
    tab = KR.table().astype(np.int64)
    modes = []
    for nx, ny in np.asarray(vectors).reshape(-1, 2).tolist():
        idx = KR.index(nx, ny, xt, yt, box_log2)
        modes.append((int(tab[idx, 0].sum()), int(tab[idx, 1].sum())))  # fewer than 2^28 entries of at most 2^30
    return int(ok.sum()), int(w.sum()), modes


def table(records, steps, lags, overlap_radius, vectors, box_log2):
    """The rows of one member after the records `records` (positions (n, 2), or tuples that start with them, in the order
    taken) with pbSimStats.steps `steps` per record: per lag a list over the vectors of dicts of Python ints, as
    Sim.four_point() returns one member.  Record r is paired with the records r - l for l = 0 ... min(r, lags - 1)."""
    vectors = np.asarray(vectors).reshape(-1, 2).tolist()
    qa = qa_of(overlap_radius)
    snaps = [XR.snapshot(r[0] if isinstance(r, (tuple, list)) else r) for r in records]
    rows = [[dict(dict.fromkeys(FIELDS, 0), lag=l, nx=int(nx), ny=int(ny)) for nx, ny in vectors] for l in range(lags)]
    for r in range(len(snaps)):
        for l in range(min(r, lags - 1) + 1):
            m, q, modes = pair(snaps[r], snaps[r - l], vectors, box_log2, qa)
            for row, (a, b) in zip(rows[l], modes):
                row["origins"] += 1
                row["sum_steps"] += int(steps[r]) - int(steps[r - l])
                row["samples"] += m
                row["overlap"] += q
                row["overlap2"] += q * q
                row["re"] += a
                row["im"] += b
                row["power"] += a * a + b * b
    return rows


def overlaps(records, lags, overlap_radius):
    """Q of every origin: [lag] -> list over the origins r = lag ... of (m, Q, the overlap mask in original order)."""
    qa = qa_of(overlap_radius)
    snaps = [XR.snapshot(r[0] if isinstance(r, (tuple, list)) else r) for r in records]
    out = [[] for _ in range(lags)]
    for r in range(len(snaps)):
        for l in range(min(r, lags - 1) + 1):
            ok, w = weights(snaps[r], snaps[r - l], qa)
            out[l].append((int(ok.sum()), int(w.sum()), w))
    return out


def limbs(value, count):
    """The `count` little-endian 64-bit limbs of a signed value as a two's-complement word."""
    bits = 64 * count
    assert -(1 << (bits - 1)) <= value < 1 << (bits - 1)
    v = value & ((1 << bits) - 1)
    return [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(count)]
