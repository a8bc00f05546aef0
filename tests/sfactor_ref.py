"""Reference for the structure factor (pbSimStructureFactor / pbSimStructureFactorOf, csrc/pb_sfactor.hip): the series'
quantisation (tests/series_ref.py) for the values, uint32 arithmetic for the turn of a bot, the table from pbPhasorTable,
Python ints for every sum, so that each figure is exact and can be compared with the device's with ==.
include/particlebot_hip.h has the definitions."""
import numpy as np

import series_ref as SR

f32 = np.float32
KINDS = ("density", "radius", "velocity")
SUMS = ("re", "im", "re2", "im2")
ROW_FIELDS = ("nx", "ny", "measured") + SUMS
STEPS = 4096
UNIT = 1 << 30
M32 = 0xFFFFFFFF

_table = None


def table():
    """The (4096, 2) int32 table the library exports: row j = (C[j], S[j])."""
    global _table
    if _table is None:
        import particlerobotsimulations_amd as pb
        _table = pb.phasor_table()
    return _table


def index(nx, ny, qx, qy, box_log2):
    """The table index of bots at (qx, qy) for the vector (nx, ny): every step on 32-bit unsigned words, mod 2^32."""
    assert -8 <= box_log2 <= 12
    with np.errstate(over="ignore"):
        qx, qy = np.asarray(qx, np.int64).astype(np.uint32), np.asarray(qy, np.int64).astype(np.uint32)
        u = np.uint32(int(nx) & M32) * qx + np.uint32(int(ny) & M32) * qy
        t = u << np.uint32(12 - box_log2)
        return ((t + np.uint32(0x80000)) >> np.uint32(20)) & np.uint32(STEPS - 1)


def weights(pos, vel, rad, kind):
    """(measured mask, qx, qy, a, a2) of one member's bots for a kind: int64 arrays, zeros where a bot is not measured."""
    assert kind in KINDS, kind
    pos, vel = np.asarray(pos, f32).reshape(-1, 2), np.asarray(vel, f32).reshape(-1, 2)
    rad = np.asarray(rad, f32).reshape(-1)
    qx, okx = SR.quantise(pos[:, 0])
    qy, oky = SR.quantise(pos[:, 1])
    ok = okx & oky
    n = len(rad)
    a, a2 = np.ones(n, np.int64), np.zeros(n, np.int64)
    if kind == "radius":
        qr, okr = SR.quantise(rad)
        ok, a = ok & okr, np.array(qr, np.int64)
    elif kind == "velocity":
        wx, okwx = SR.quantise(vel[:, 0])
        wy, okwy = SR.quantise(vel[:, 1])
        ok, a, a2 = ok & okwx & okwy, np.array(wx, np.int64), np.array(wy, np.int64)
    return ok, np.array(qx, np.int64), np.array(qy, np.int64), a, a2


def _exact_sum(a, c):
    """sum a[i] * c[i] as a Python int: |a c| <= 2^61 fits an int64, and the sum is taken over the two halves of every
    product, each of which stays far inside an int64."""
    p = a * c
    return (int((p >> 32).sum()) << 32) + int((p & M32).sum())


def structure_factor(pos, vel, rad, vectors, box_log2, kind="density"):
    """One member's rows: a list of dicts of Python ints (ROW_FIELDS), one per vector of `vectors`, in its order."""
    ok, qx, qy, a, a2 = weights(pos, vel, rad, kind)
    qx, qy, a, a2 = qx[ok], qy[ok], a[ok], a2[ok]
    tab = table().astype(np.int64)
    rows = []
    for nx, ny in np.asarray(vectors).reshape(-1, 2).tolist():
        idx = index(nx, ny, qx, qy, box_log2)
        c, s = tab[idx, 0], tab[idx, 1]
        rows.append({"nx": int(nx), "ny": int(ny), "measured": int(ok.sum()), "re": _exact_sum(a, c), "im": _exact_sum(a, s),
                     "re2": _exact_sum(a2, c), "im2": _exact_sum(a2, s)})
    return rows


def from_device(rows):
    """A structured (nvec,) array of Sim.structure_factor() as the list of dicts structure_factor() above returns."""
    out = []
    for r in rows:
        d = {"nx": int(r["nx"]), "ny": int(r["ny"]), "measured": int(r["measured"])}
        for k in SUMS:
            d[k] = (int(r[k + "_hi"]) << 32) + int(r[k + "_lo"])
        out.append(d)
    return out
