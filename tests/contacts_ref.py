"""Reference of the contact export (pbSimContactsOf / pbSimContactVirialOf, csrc/pb_contacts.hip): numpy and the CPU
oracle only.

Topology: tests/cluster_ref.py's links (pinned to a brute force by tests/test_cluster_api.py and, for this file's own
ordering, by tests/test_contacts_api.py).  Layout: CSR in original bot order, every undirected link under both ends, a
bot's entries ascending in `other`.  gap = dist - (ri + rj) by the predicate's fp32 formula.  Force: one
orc_collideSpheres call per directed entry (A = the owning bot, B = other) into zeroed outputs, the attraction argument
formed in fp32 as collideCell does, P.attraction * att2 * att1 with the payload's attractionFactor for whichever end is
the payload bot.  Virial: a sequential float64 loop over each bot's entries in CSR order."""
import numpy as np

import cluster_ref as CR

f32 = np.float32


def topology(pos, rad, gap):
    """(offsets uint32 n + 1, owner int64 E, other int64 E) in CSR order."""
    rad = np.asarray(rad, f32)
    n = rad.size
    i, j = CR.links(pos, rad, gap)
    owner = np.concatenate([i, j]).astype(np.int64)
    other = np.concatenate([j, i]).astype(np.int64)
    order = np.lexsort((other, owner))
    owner, other = owner[order], other[order]
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(owner, minlength=n), out=offsets[1:])
    return offsets.astype(np.uint32), owner, other


def gaps_of(pos, rad, owner, other):
    """dist - (ri + rj) of every directed entry, and (rx, ry), every operation rounded to fp32."""
    pos = np.asarray(pos, f32).reshape(-1, 2)
    rad = np.asarray(rad, f32)
    with np.errstate(all="ignore"):
        rx = pos[other, 0] - pos[owner, 0]
        ry = pos[other, 1] - pos[owner, 1]
        dist = np.sqrt(rx * rx + ry * ry)
        gap = dist - (rad[owner] + rad[other])
    assert gap.dtype == f32 and rx.dtype == f32
    return gap, rx, ry


def attraction_of(P, owner, other):
    """collideCell's attraction argument per directed entry, in fp32: P.attraction * att2 * att1."""
    one = f32(1.0)
    payload = int(P.nDead) == -1
    last = int(P.nCells) - 1
    att1 = np.where(payload & (owner == last), f32(P.attractionFactor), one).astype(f32)
    att2 = np.where(payload & (other == last), f32(P.attractionFactor), one).astype(f32)
    out = f32(P.attraction) * att2 * att1
    assert out.dtype == f32
    return out


def network(orc, P, pos, vel, rad, gap):
    """The whole export of one member's state: dict of offsets (uint32, n + 1), other (uint32, E), gap (float32, E),
    force (float32, E x 2) and virial (float64, n x 4)."""
    import ctypes as C
    pos = np.ascontiguousarray(np.asarray(pos, f32).reshape(-1, 2))
    vel = np.ascontiguousarray(np.asarray(vel, f32).reshape(-1, 2))
    rad = np.ascontiguousarray(np.asarray(rad, f32))
    n = rad.size
    offsets, owner, other = topology(pos, rad, gap)
    g, rx, ry = gaps_of(pos, rad, owner, other)
    att = attraction_of(P, owner, other)
    L = orc.lib()
    E = owner.size
    force = np.zeros((E, 2), f32)
    fa, fr = np.zeros(1, f32), np.zeros(1, f32)
    with np.errstate(all="ignore"):
        for e in range(E):
            a, b = int(owner[e]), int(other[e])
            out = np.zeros(2, f32)
            fa[0] = fr[0] = 0.0
            L.orc_collideSpheres(C.byref(P), pos[a].copy(), pos[b].copy(), vel[a].copy(), vel[b].copy(), float(rad[a]),
                                 float(rad[b]), float(att[e]), out, fa, fr)
            force[e] = out
        virial = np.zeros((n, 4), np.float64)
        for i in range(n):
            sxx = sxy = syx = syy = np.float64(0.0)
            for e in range(int(offsets[i]), int(offsets[i + 1])):
                x, y = np.float64(rx[e]), np.float64(ry[e])
                fx, fy = np.float64(force[e, 0]), np.float64(force[e, 1])
                sxx = sxx + x * fx
                sxy = sxy + x * fy
                syx = syx + y * fx
                syy = syy + y * fy
            virial[i] = (sxx, sxy, syx, syy)
    return {"offsets": offsets, "other": other.astype(np.uint32), "gap": g, "force": force, "virial": virial}
