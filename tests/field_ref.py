"""Reference for the field maps (pbSimFieldMap / pbSimFieldMapOf, csrc/pb_field.hip): numpy fp32 with separate operations
for the choice of the cell, the series' quantisation (tests/series_ref.py) for the values, Python ints for every sum, so
that each figure is exact and can be compared with the device's with ==.  include/particlebot_hip.h has the
definitions."""
import numpy as np

import series_ref as SR

f32 = np.float32
CELL_FIELDS = ("count", "dead", "sum_qr", "sum_wx", "sum_wy", "rr", "vv")
TOTALS = ("measured", "inside", "outside", "unmeasured")


def axis(coord, center, half, cells):
    """(index, inside) of fp32 coordinates along one axis: x0 = center - half and s = (float)cells / (half + half) once,
    then t = (x - x0) * s with two roundings; inside iff t >= 0 && t < (float)cells; index (int)t.  -0.0 is inside, in 0."""
    center, half = f32(center), f32(half)
    x0 = f32(center - half)
    s = f32(f32(cells) / f32(half + half))
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(coord, f32) - x0).astype(f32)  # one rounding
        t = (d * s).astype(f32)                        # and another
        inside = (t >= f32(0.0)) & (t < f32(cells))
    index = np.where(inside, t, f32(0.0)).astype(np.int64)  # truncation of a value in [0, cells)
    return index, inside


def field_map(pos, vel, rad, dead, nx, ny, center, half):
    """One member's map: (cells, totals).  cells[iy][ix] is a dict of Python ints (CELL_FIELDS), row 0 the lowest y;
    totals a dict (TOTALS).  `half` is one half extent or (halfX, halfY)."""
    pos, vel = np.asarray(pos, f32).reshape(-1, 2), np.asarray(vel, f32).reshape(-1, 2)
    rad, dead = np.asarray(rad, f32).reshape(-1), np.asarray(dead).reshape(-1)
    hx, hy = (half, half) if np.isscalar(half) else half
    _, okx = SR.quantise(pos[:, 0])
    _, oky = SR.quantise(pos[:, 1])
    wx, okwx = SR.quantise(vel[:, 0])
    wy, okwy = SR.quantise(vel[:, 1])
    qr, okr = SR.quantise(rad)
    measured = okx & oky & okwx & okwy & okr
    ix, inx = axis(pos[:, 0], center[0], hx, nx)
    iy, iny = axis(pos[:, 1], center[1], hy, ny)
    inside = measured & inx & iny
    cells = [[dict.fromkeys(CELL_FIELDS, 0) for _ in range(nx)] for _ in range(ny)]
    for i in (int(k) for k in np.flatnonzero(inside)):
        c = cells[int(iy[i])][int(ix[i])]
        c["count"] += 1
        c["dead"] += int(dead[i] != 0)
        c["sum_qr"] += qr[i]
        c["sum_wx"] += wx[i]
        c["sum_wy"] += wy[i]
        c["rr"] += qr[i] * qr[i]
        c["vv"] += wx[i] * wx[i] + wy[i] * wy[i]
    m, k = int(measured.sum()), int(inside.sum())
    return cells, {"measured": m, "inside": k, "outside": m - k, "unmeasured": len(rad) - m}


def from_device(cells):
    """A structured (ny, nx) array of Sim.field_map() as the nested list of dicts field_map() above returns."""
    out = []
    for row in cells:
        out.append([{"count": int(c["count"]), "dead": int(c["dead"]), "sum_qr": int(c["sum_qr"]),
                     "sum_wx": int(c["sum_wx"]), "sum_wy": int(c["sum_wy"]),
                     "rr": (int(c["rr_hi"]) << 32) + int(c["rr_lo"]), "vv": (int(c["vv_hi"]) << 32) + int(c["vv_lo"])}
                    for c in row])
    return out
