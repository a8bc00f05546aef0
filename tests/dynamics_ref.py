"""numpy-only reference of the rearrangement analysis (pbSimMarkReference / pbSimRearrangementStats /
pbSimRearrangementOf, csrc/pb_dynamics.hip).

Two states of one member: the marked one (pos0, rad0) and the present one (pos1, rad1).  The two link networks come from
tests/contacts_ref.py's topology (CSR in original order, a bot's entries ascending), `kept` from intersecting the two
ascending lists.  Displacements are taken in float32 in the order the header states: dx = x_now - x_mark, measured iff
all four coordinates are finite and |dx|, |dy| < 2048; q = rint(d * 2^20) (nearest even), s = qx^2 + qy^2.  Every sum is
a Python int.  tests/test_dynamics_api.py pins all of it to an O(n^2) brute force and to hand-built answers."""
import numpy as np

import contacts_ref as KR

f32 = np.float32
FIELDS = ("bonds_marked", "bonds_now", "bonds_kept", "bots_unchanged", "bots_lost", "bots_gained", "measured", "sum_qx",
          "sum_qy", "sum_q2", "max_q2")


def bond_counts(pos0, rad0, pos1, rad1, gap):
    """(marked, now, kept): int64 arrays per bot."""
    n = np.asarray(rad0).size
    off0, own0, oth0 = KR.topology(pos0, rad0, gap)
    off1, own1, oth1 = KR.topology(pos1, rad1, gap)
    marked = np.diff(off0.astype(np.int64))
    now = np.diff(off1.astype(np.int64))
    # CSR order is ascending in (owner, other): the two key lists are ascending and without repeats
    k0, k1 = own0 * n + oth0, own1 * n + oth1
    assert (np.diff(k0) > 0).all() and (np.diff(k1) > 0).all()
    both = np.intersect1d(k0, k1, assume_unique=True)
    kept = np.bincount(both // n, minlength=n).astype(np.int64)
    return marked, now, kept


def displacements(pos0, pos1):
    """(disp float32 (n, 2), measured bool n, qx, qy: lists of Python ints, 0 where not measured)."""
    pos0 = np.asarray(pos0, f32).reshape(-1, 2)
    pos1 = np.asarray(pos1, f32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        disp = pos1 - pos0
        assert disp.dtype == f32
        measured = (np.isfinite(pos0).all(axis=1) & np.isfinite(pos1).all(axis=1) &
                    (np.abs(disp[:, 0]) < f32(2048.0)) & (np.abs(disp[:, 1]) < f32(2048.0)))
        scaled = disp * f32(1048576.0)
        assert scaled.dtype == f32
        q = np.rint(np.where(measured[:, None], scaled, f32(0.0))).astype(np.int64)
    return disp, measured, [int(v) for v in q[:, 0]], [int(v) for v in q[:, 1]]


def analyse(pos0, rad0, pos1, rad1, gap):
    """(row dict over FIELDS, per-bot dict of disp, marked, now, kept) of one member."""
    marked, now, kept = bond_counts(pos0, rad0, pos1, rad1, gap)
    disp, measured, qx, qy = displacements(pos0, pos1)
    s = [x * x + y * y for x, y in zip(qx, qy)]
    row = {"bonds_marked": int(marked.sum()), "bonds_now": int(now.sum()), "bonds_kept": int(kept.sum()),
           "bots_unchanged": int(((kept == marked) & (kept == now)).sum()), "bots_lost": int((kept < marked).sum()),
           "bots_gained": int((kept < now).sum()), "measured": int(measured.sum()), "sum_qx": sum(qx), "sum_qy": sum(qy),
           "sum_q2": sum(s), "max_q2": max(s) if s else 0}
    return row, {"disp": disp, "marked": marked.astype(np.uint32), "now": now.astype(np.uint32),
                 "kept": kept.astype(np.uint32)}


def perturbed(pos, rng, shift=0.25):
    """The present state of the tests' recipe: the marked positions plus fp32 noise of 0.03 plus `shift`."""
    pos = np.asarray(pos, f32)
    out = pos + (rng.standard_normal(pos.shape) * 0.03).astype(f32) + f32(shift)
    assert out.dtype == f32
    return out
