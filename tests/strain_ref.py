"""numpy-only reference of the strain analysis (pbSimStrainStats / pbSimStrainOf, csrc/pb_strain.hip; the definitions
are in include/particlebot_hip.h).

Two states of one member: the marked one (pos0, rad0, the link network at `gap`) and the present positions pos1.  The
marked network comes from tests/contacts_ref.py's topology.  Bond vectors are taken in float32 in the order the header
states, a bond is used iff all four components are below 8 in magnitude (a NaN or an infinity is not), q = rint(v * 2^20)
to nearest even.  The moments are exact integers (int64 per bot, Python ints per member); the fit is np.float64, one
operation at a time in the stated order (numpy rounds each once and contracts nothing).  tests/test_strain_api.py pins all of it to an O(n^2) brute force
and to hand-built answers."""
import numpy as np

import contacts_ref as KR

f32 = np.float32
f64 = np.float64
REACH = f32(8.0)
MAX_LIST = 1 << 16
MOMENTS = ("k", "yxx", "yxy", "yyy", "xxx", "xxy", "xyx", "xyy", "w")
SUMS = MOMENTS[1:]
FIELDS = ("fitted", "unfitted", "above", "bonds_used", "bonds_dropped") + SUMS + ("sum_d2", "max_d2")


def fit(m):
    """(fitted, J as four np.float64: Jxx Jxy Jyx Jyy, d2 np.float64) of nine integer moments, in binary64, every
    operation rounded once in the header's order; the integers are converted with round-to-nearest (Python's float())."""
    k = int(m[0])
    a, b, c, xxx, xxy, xyx, xyy, w = (f64(float(int(v))) for v in m[1:])
    zero = f64(0.0)
    det = a * c - b * b
    if not (k >= 3 and det > 0):
        return False, (zero, zero, zero, zero), zero
    jxx = (xxx * c - xxy * b) / det
    jxy = (xxy * a - xxx * b) / det
    jyx = (xyx * c - xyy * b) / det
    jyy = (xyy * a - xyx * b) / det
    d2 = w - ((jxx * xxx + jxy * xxy) + (jyx * xyx + jyy * xyy))
    d2 = d2 if d2 > 0 else zero
    return True, (jxx, jxy, jyx, jyy), d2


def units(d2):
    """e = rint(d2) as a Python int; 2^63 for a d2 of 2^63 or more."""
    return int(np.rint(d2)) if d2 < f64(2.0 ** 63) else 1 << 63


def fit_all(mom):
    """fit() of every row of an int64 (n, 9) array at once: the same operations in the same order, elementwise in
    np.float64 (astype rounds to nearest).  (fitted bool n, J float64 (n, 2, 2), d2 float64 n)."""
    mom = np.asarray(mom, np.int64).reshape(-1, 9)
    a, b, c, xxx, xxy, xyx, xyy, w = (mom[:, k].astype(f64) for k in range(1, 9))
    det = a * c - b * b
    fitted = (mom[:, 0] >= 3) & (det > 0)
    safe = np.where(fitted, det, f64(1.0))
    jxx = (xxx * c - xxy * b) / safe
    jxy = (xxy * a - xxx * b) / safe
    jyx = (xyx * c - xyy * b) / safe
    jyy = (xyy * a - xyx * b) / safe
    d2 = w - ((jxx * xxx + jxy * xxy) + (jyx * xyx + jyy * xyy))
    d2 = np.where(d2 > 0, d2, f64(0.0))
    J = np.stack([jxx, jxy, jyx, jyy], axis=1)
    J[~fitted] = 0.0
    d2[~fitted] = 0.0
    return fitted, J.reshape(-1, 2, 2), d2


def analyse_csr(off, oth, pos0, pos1, threshold=0.0):
    """(row dict over FIELDS, per-bot dict of moments int64 (n, 9), gradient float64 (n, 2, 2), d2min float64 n, fitted
    bool n, dropped int64 n) from the marked network as a CSR (offsets n + 1, other E)."""
    pos0 = np.asarray(pos0, f32).reshape(-1, 2)
    pos1 = np.asarray(pos1, f32).reshape(-1, 2)
    n = pos0.shape[0]
    off = np.asarray(off).astype(np.int64)
    oth = np.asarray(oth).astype(np.int64)
    length = np.diff(off)
    own = np.repeat(np.arange(n, dtype=np.int64), length)
    with np.errstate(all="ignore"):
        d = np.concatenate([pos0[oth] - pos0[own], pos1[oth] - pos1[own]], axis=1)  # d0x d0y dx dy
        assert d.dtype == f32
        used = (np.abs(d) < REACH).all(axis=1) & (length < MAX_LIST)[own]
        scaled = np.where(used[:, None], d, f32(0.0)) * f32(1048576.0)
        assert scaled.dtype == f32
    q = np.rint(scaled).astype(np.int64)
    q0x, q0y, qx, qy = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    terms = [used.astype(np.int64), q0x * q0x, q0x * q0y, q0y * q0y, qx * q0x, qx * q0y, qy * q0x, qy * q0y,
             qx * qx + qy * qy]
    mom = np.zeros((n, 9), np.int64)
    for k, v in enumerate(terms):
        # a running sum that may wrap: a bot's own sum is below 2^63, so the difference of two wrapped values is exact
        run = np.concatenate([np.zeros(1, np.int64), np.cumsum(v, dtype=np.int64)])
        mom[:, k] = run[off[1:]] - run[off[:-1]]
    dropped = length - mom[:, 0]
    fitted, grad, d2min = fit_all(mom)
    thr = f64(float(f32(threshold))) * f64(2.0 ** 40)
    e = [units(v) for v in d2min[fitted]]
    row = {"fitted": int(fitted.sum()), "unfitted": int(n - fitted.sum()), "above": int((fitted & (d2min > thr)).sum()),
           "bonds_used": int(mom[:, 0].sum()), "bonds_dropped": int(dropped.sum()), "sum_d2": sum(e),
           "max_d2": max(e) if e else 0}
    for k, name in enumerate(MOMENTS):
        if k:
            row[name] = sum(int(v) for v in mom[:, k])
    row = {name: row[name] for name in FIELDS}
    return row, {"moments": mom, "gradient": grad, "d2min": d2min, "fitted": fitted, "dropped": dropped}


def analyse(pos0, rad0, pos1, gap, threshold=0.0):
    """The analysis of one member: the mark of (pos0, rad0) at `gap` against the present positions pos1."""
    off, _, oth = KR.topology(pos0, rad0, gap)
    return analyse_csr(off, oth, pos0, pos1, threshold)
