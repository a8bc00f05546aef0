"""particlerobotsimulations_amd -- MI355X-native particle-robot update loop.

Python is only the scripting shell over the C-ABI of libparticlebot_hip.so (hand-written HIP for
gfx950): device memory, the reference's `extern "C"` device boundary (`legacy`) and the resident
fused engine (`Sim`).  The C++ host side (class Particlebot, .cfg loader, headless runner) lives in
csrc/ and libparticlebot_host.so.

There is no CPU fallback anywhere in this package.
"""
import ctypes as C

import numpy as np

from . import _analysis, _capi
from ._analysis import van_hove_distinct_lists, van_hove_lists  # noqa: F401
from ._capi import SimParams, make_params, pbSimConfig, pbSimStats  # noqa: F401

__all__ = ["Sim", "Ensemble", "DeviceArray", "legacy", "SimParams", "make_params", "library_paths", "self_test",
           "radial_distribution", "mean_squared_displacement", "moments_summary", "correlation_values",
           "connected_correlation", "time_correlation_summary", "field_values", "structure_factor_values",
           "half_plane_vectors", "phasor_table", "scattering_summary", "van_hove_summary",
           "deformation_gradient", "mean_d2min", "coherent_scattering_summary", "four_point_summary",
           "bond_dynamics_summary"]


def phasor_table():
    """The phasor table the device adds (pbPhasorTable): an int32 array (4096, 2), row j = (C[j], S[j]) =
    (rint(cos(2 pi j / 4096) 2^30), rint(sin(2 pi j / 4096) 2^30)).  Needs no GPU."""
    table = np.zeros((_capi.PHASOR_STEPS, 2), np.int32)
    _capi.check(_capi.lib().pbPhasorTable(_capi.np_ptr(table), table.size), "pbPhasorTable")
    return table


def half_plane_vectors(nmax):
    """All (nx, ny) with |nx|, |ny| <= nmax and (ny > 0 or (ny == 0 and nx > 0)) as an int32 array (2 nmax^2 + 2 nmax, 2):
    one of every pair k, -k (S(-k) adds nothing), without (0, 0)."""
    nmax = int(nmax)
    if nmax < 0:
        raise ValueError("half_plane_vectors: nmax must be >= 0")
    out = [(nx, 0) for nx in range(1, nmax + 1)]
    out += [(nx, ny) for ny in range(1, nmax + 1) for nx in range(-nmax, nmax + 1)]
    return np.array(out, np.int32).reshape(-1, 2)


def structure_factor_values(rows):
    """The rows of structure_factor() as a dict of arrays of the rows' shape: nx, ny, measured as they are; re, im, re2,
    im2 as object arrays of Python ints composed from their 128 bits (hi * 2^32 + lo; units of 2^-30 for the density,
    2^-50 otherwise); and "s" = (re^2 + im^2) / (2^60 measured) as floats, NaN where nothing was measured: S(k) for
    the density."""
    from fractions import Fraction
    rows = np.asarray(rows)
    out = {name: rows[name] for name in ("nx", "ny", "measured")}
    for name in ("re", "im", "re2", "im2"):
        out[name] = _capi.compose_128(rows, name)
    s = [float(Fraction(re * re + im * im, int(m) << 60)) if m else float("nan")
         for re, im, m in zip(out["re"].reshape(-1), out["im"].reshape(-1), rows["measured"].reshape(-1))]
    out["s"] = np.array(s, np.float64).reshape(rows.shape)
    return out


def radial_distribution(counts, r_max, density, n):
    """g(r) from the radial pair counts of radial_counts(r_max, bins) (pure Python, float64): counts[..., b] ordered
    pairs among n bots fell into the annulus [b, b + 1) * r_max / bins, an ideal gas of number density `density` (the
    caller's choice: a free blob has no box) would put n * density * annulus area there.  Returns (r, g): the bin
    centres and counts / (n * density * pi * (r_hi^2 - r_lo^2)), shaped like counts."""
    counts = np.asarray(counts, np.float64)
    bins = counts.shape[-1]
    edges = np.arange(bins + 1, dtype=np.float64) * (float(r_max) / bins)
    area = np.pi * (edges[1:] ** 2 - edges[:-1] ** 2)
    return 0.5 * (edges[1:] + edges[:-1]), counts / (float(n) * float(density) * area)


def mean_squared_displacement(row, subtract_drift=False):
    """The mean squared displacement since the mark from one row of rearrangement() (pure Python): sum_q2 / 2^40 /
    measured, and with subtract_drift the squared mean displacement (sum_qx^2 + sum_qy^2) / measured^2 / 2^40 taken
    off, which leaves the variance about the common drift.  Formed from the integers as one exact fraction and
    converted to float once; NaN when no bot was measured."""
    from fractions import Fraction
    m = int(row["measured"])
    if m == 0:
        return float("nan")
    num = int(row["sum_q2"]) * m
    if subtract_drift:
        num -= int(row["sum_qx"]) ** 2 + int(row["sum_qy"]) ** 2
    return float(Fraction(num, m * m << 40))


def deformation_gradient(row):
    """The macroscopic deformation gradient of a member from one row of strain() (pure Python): F = X Y^-1 with the
    row's sums over all used bonds, the affine map that carries the marked bond vectors onto the present ones in the
    least-squares sense.  A 2 x 2 float64 array, every entry formed from the integers as one exact fraction and
    converted once; NaN where the marked bonds do not span the plane (det Y <= 0)."""
    from fractions import Fraction
    a, b, c = int(row["yxx"]), int(row["yxy"]), int(row["yyy"])
    det = a * c - b * b
    if det <= 0:
        return np.full((2, 2), np.nan)
    xxx, xxy, xyx, xyy = (int(row[k]) for k in ("xxx", "xxy", "xyx", "xyy"))
    return np.array([[float(Fraction(xxx * c - xxy * b, det)), float(Fraction(xxy * a - xxx * b, det))],
                     [float(Fraction(xyx * c - xyy * b, det)), float(Fraction(xyy * a - xyx * b, det))]], np.float64)


def mean_d2min(row):
    """The mean non-affine displacement D2min per fitted bot from one row of strain() (pure Python), in world units
    squared: sum_d2 / 2^40 / fitted as one exact fraction converted once; NaN when no bot was fitted."""
    from fractions import Fraction
    m = int(row["fitted"])
    return float(Fraction(int(row["sum_d2"]), m << 40)) if m else float("nan")


def time_correlation_summary(row, lag0=None):
    """What one row of time_correlation() says about its lag, in float64 from the integers (pure Python; every quotient
    is formed as one exact fraction and converted once).  Lengths in world units, from the units of 2^-20:
      mean_lag_steps = sum_steps / origins;
      msd = msd / samples;  msd_drift_corrected = (msd - (sum_qx^2 + sum_qy^2) / samples) / samples, the spread about
      the common drift;
      vacf = the mean of v(t) . v(t - lag);  vacf_normalised = that over the mean |v|^2 of `lag0`, the same member's
      lag-0 row (None without one, or when its vacf is 0);
      overlap = overlap / samples, the fraction Q of bots that moved less than the overlap radius.
    Every value is None for a row with no samples."""
    from fractions import Fraction
    keys = ("mean_lag_steps", "msd", "msd_drift_corrected", "vacf", "vacf_normalised", "overlap")
    m = int(row["samples"])
    if m == 0:
        return dict.fromkeys(keys)
    two = 1 << 40
    msd, vacf, sx, sy = (int(row[k]) for k in ("msd", "vacf", "sum_qx", "sum_qy"))
    norm = None
    if lag0 is not None and int(lag0["samples"]) and int(lag0["vacf"]):
        norm = float(Fraction(vacf * int(lag0["samples"]), m * int(lag0["vacf"])))
    origins = int(row["origins"])
    return {"mean_lag_steps": float(Fraction(int(row["sum_steps"]), origins)) if origins else None,
            "msd": float(Fraction(msd, m * two)),
            "msd_drift_corrected": float(Fraction(msd * m - sx * sx - sy * sy, m * m * two)),
            "vacf": float(Fraction(vacf, m * two)),
            "vacf_normalised": norm,
            "overlap": float(Fraction(int(row["overlap"]), m))}


def scattering_summary(row):
    """What one row of scattering() says, in float64 from the integers (pure Python; every quotient is formed as one
    exact fraction and converted once): fs_re = re / (2^30 samples), the self-intermediate scattering function
    F_s(k, lag); fs_im = im / (2^30 samples), its imaginary part (collective drift along k);
    mean_lag_steps = sum_steps / origins.  The first two are None for a row with no samples, the last for one with no
    origins."""
    from fractions import Fraction
    m, origins = int(row["samples"]), int(row["origins"])
    return {"fs_re": float(Fraction(int(row["re"]), m << 30)) if m else None,
            "fs_im": float(Fraction(int(row["im"]), m << 30)) if m else None,
            "mean_lag_steps": float(Fraction(int(row["sum_steps"]), origins)) if origins else None}


def coherent_scattering_summary(row):
    """What one row of coherent_scattering() says, in float64 from the integers (pure Python; every quotient is formed
    as one exact fraction and converted once): f_re = re / (2^60 bots_then), the coherent intermediate scattering
    function F(k, lag), at lag 0 the time-averaged S(k); f_im = im / (2^60 bots_then), its imaginary part (a density
    wave that travels along k); mean_lag_steps = sum_steps / origins.  The first two are None for a row with no
    measured bot, the last for one with no origins."""
    from fractions import Fraction
    m, origins = int(row["bots_then"]), int(row["origins"])
    return {"f_re": float(Fraction(int(row["re"]), m << 60)) if m else None,
            "f_im": float(Fraction(int(row["im"]), m << 60)) if m else None,
            "mean_lag_steps": float(Fraction(int(row["sum_steps"]), origins)) if origins else None}


def four_point_summary(rows):
    """What the rows of one (member, lag) of four_point() say, in float64 from the integers (pure Python ints; every
    quotient is formed as one exact fraction and converted once).  `rows` is the list over the vectors, or one row.
    With O = origins and Nbar = samples / O:  mean_overlap = overlap / samples, the fraction of the measured bots that
    stayed within the radius;  chi4 = (overlap2 / O - (overlap / O)^2) / Nbar, the four-point susceptibility;  s4, per
    vector, = (power / O - (re^2 + im^2) / O^2) / (2^60 Nbar), the structure factor of the slow bots;
    mean_lag_steps = sum_steps / O.  All are None for a lag with no origins, and all but the last for one with no
    measured pair."""
    from fractions import Fraction
    rows = [rows] if isinstance(rows, dict) else list(rows)
    first = rows[0]
    o, m = int(first["origins"]), int(first["samples"])
    if not o or not m:
        return {"mean_overlap": None, "chi4": None, "s4": [None] * len(rows),
                "mean_lag_steps": float(Fraction(int(first["sum_steps"]), o)) if o else None}
    q, q2 = int(first["overlap"]), int(first["overlap2"])
    # (x / O - y / O^2) / (m / O) = (x O - y) / (O m)
    s4 = [float(Fraction(int(r["power"]) * o - int(r["re"]) ** 2 - int(r["im"]) ** 2, (o * m) << 60)) for r in rows]
    return {"mean_overlap": float(Fraction(q, m)), "chi4": float(Fraction(q2 * o - q * q, o * m)), "s4": s4,
            "mean_lag_steps": float(Fraction(int(first["sum_steps"]), o))}


def bond_dynamics_summary(row):
    """What one row of bond_dynamics() says, in float64 from the integers (pure Python ints; every quotient is formed as
    one exact fraction and converted once).  With C = sum_k cage_samples[k - 1], the caged bots:
    bond_survival = bonds_kept / bonds_then, the bond-breaking correlation;  fraction_lost = bots_lost / samples;
    cage_msd = (sum_k cage_q2[k - 1] / k^2) / (2^40 C), the mean squared cage-relative displacement in world units;
    plain_msd = plain_q2 / (2^40 C), the plain one of the same bots;  cage_overlap = sum_k cage_overlap[k - 1] / C;
    crowded_fraction = crowded / (samples + crowded);  mean_lag_steps = sum_steps / origins.  A value whose denominator
    is 0 is None."""
    from fractions import Fraction

    def quotient(num, den):
        return float(Fraction(num, den)) if den else None

    caged = sum(int(c) for c in row["cage_samples"])
    cage = sum(Fraction(int(q), k * k) for k, q in enumerate(row["cage_q2"], 1))
    samples, crowded = int(row["samples"]), int(row["crowded"])
    return {"bond_survival": quotient(int(row["bonds_kept"]), int(row["bonds_then"])),
            "fraction_lost": quotient(int(row["bots_lost"]), samples),
            "cage_msd": quotient(cage, caged << 40), "plain_msd": quotient(int(row["plain_q2"]), caged << 40),
            "cage_overlap": quotient(sum(int(c) for c in row["cage_overlap"]), caged),
            "crowded_fraction": quotient(crowded, samples + crowded),
            "mean_lag_steps": quotient(int(row["sum_steps"]), int(row["origins"]))}


def van_hove_summary(row, width):
    """What one row of van_hove() says, in float64 from the integers (pure Python; every quotient is formed as one exact
    fraction and converted once): msd = msd / (2^40 samples), the mean squared displacement in world units;
    msd_in_widths = that over width^2, which says how many bins of `width` the distribution spans;
    alpha2 = <r^4> / (2 <r^2>^2) - 1 = q4 samples / (2 msd^2) - 1, the non-Gaussian parameter in two dimensions (0 for a
    Gaussian; nan where msd == 0); mean_lag_steps = sum_steps / origins.  msd and msd_in_widths are nan for a row with
    no samples, mean_lag_steps for one with no origins."""
    from fractions import Fraction
    m, origins, msd, q4 = (int(row[k]) for k in ("samples", "origins", "msd", "q4"))
    nan = float("nan")
    mean = Fraction(msd, m << 40) if m else None
    w2 = Fraction(float(width)) ** 2
    return {"msd": float(mean) if m else nan,
            "msd_in_widths": float(mean / w2) if m and w2 else nan,
            "alpha2": float(Fraction(q4 * m, 2 * msd * msd) - 1) if msd else nan,
            "mean_lag_steps": float(Fraction(int(row["sum_steps"]), origins)) if origins else nan}


def field_values(cells):
    """The cells of field_map() as a dict of arrays of the cells' shape: count, dead, sum_qr, sum_wx, sum_wy as they are,
    and rr, vv as object arrays of Python ints composed from their 128 bits (hi * 2^32 + lo).  The sums are in units of
    2^-20, rr and vv in units of 2^-40."""
    cells = np.asarray(cells)
    out = {name: cells[name] for name in ("count", "dead", "sum_qr", "sum_wx", "sum_wy")}
    for name in ("rr", "vv"):
        out[name] = _capi.compose_128(cells, name)
    return out


def correlation_values(rows):
    """One member's rows of pair_correlation() as a dict of lists of Python ints, one entry per bin: pairs, and dot, ax,
    ay composed from their 128 bits (hi * 2^32 + lo).  dot is in units of 2^-40, ax and ay in units of 2^-20."""
    rows = np.asarray(rows)
    if rows.ndim != 1:
        raise ValueError("correlation_values: the rows of one member, shaped (bins,)")
    out = {"pairs": [int(v) for v in rows["pairs"]]}
    for name in ("dot", "ax", "ay"):
        out[name] = list(_capi.compose_128(rows, name))
    return out


def connected_correlation(rows, totals):
    """(C, C / C0) of one member from pair_correlation(): float64[bins] each.  With m = sum_a / measured the connected
    correlation of a bin is C = (dot - 2 m . (ax, ay) + |m|^2 pairs) / pairs / 2^40 and C0 = sum_a2 / measured - |m|^2,
    the variance of a.  Every quotient is formed from the integers as one exact fraction and converted once; NaN for an
    empty bin, and for the ratio when C0 is 0."""
    from fractions import Fraction
    v = correlation_values(rows)
    M, sx, sy = int(totals["measured"]), int(totals["sum_ax"]), int(totals["sum_ay"])
    nan = float("nan")
    c = np.full(len(v["pairs"]), nan)
    ratio = c.copy()
    if M == 0:
        return c, ratio
    c0 = Fraction(int(totals["sum_a2"]) * M - sx * sx - sy * sy, M * M)  # units of 2^-40, like the numerators below
    for b, pairs in enumerate(v["pairs"]):
        if pairs:
            num = v["dot"][b] * M * M - 2 * M * (sx * v["ax"][b] + sy * v["ay"][b]) + (sx * sx + sy * sy) * pairs
            cb = Fraction(num, M * M * pairs)
            c[b] = float(cb / (1 << 40))
            if c0:
                ratio[b] = float(cb / c0)
    return c, ratio


def moments_summary(row):
    """What one row of moments() / series_of() says about the member, in float64 from the integers (pure Python; every
    quotient is formed as one exact fraction and converted once).  Lengths in world units, from the units of 2^-20:
      centroid (x, y); gyration (gxx, gyy, gxy): the second moments of the positions about the centroid;
      gyration_eigenvalues (larger, smaller) of that tensor; major_axis_angle of the larger one's axis, in (-pi/2, pi/2];
      mean_radius, radius_variance; covered_area = pi * sum r^2;
      centroid_velocity (vx, vy); velocity_variance = mean |v|^2 - |mean v|^2.
    Every value is None when no bot was measured."""
    import math
    from fractions import Fraction
    keys = ("centroid", "gyration", "gyration_eigenvalues", "major_axis_angle", "mean_radius", "radius_variance",
            "covered_area", "centroid_velocity", "velocity_variance")
    m = int(row["measured"])
    if m == 0:
        return dict.fromkeys(keys)
    one, two = 1 << 20, 1 << 40
    sx, sy, sr, swx, swy = (int(row[k]) for k in ("sum_qx", "sum_qy", "sum_qr", "sum_wx", "sum_wy"))
    xx, yy, xy, rr, vv = (int(row[k]) for k in ("xx", "yy", "xy", "rr", "vv"))
    central = lambda s2, a, b: Fraction(s2 * m - a * b, m * m * two)  # mean of the product minus the product of the means
    gxx, gyy, gxy = central(xx, sx, sx), central(yy, sy, sy), central(xy, sx, sy)
    fxx, fyy, fxy = float(gxx), float(gyy), float(gxy)
    half, root = 0.5 * float(gxx + gyy), math.hypot(0.5 * float(gxx - gyy), fxy)
    return {"centroid": (float(Fraction(sx, m * one)), float(Fraction(sy, m * one))),
            "gyration": (fxx, fyy, fxy),
            "gyration_eigenvalues": (half + root, half - root),
            "major_axis_angle": 0.5 * math.atan2(2.0 * fxy, float(gxx - gyy)),
            "mean_radius": float(Fraction(sr, m * one)),
            "radius_variance": float(central(rr, sr, sr)),
            "covered_area": math.pi * float(Fraction(rr, two)),
            "centroid_velocity": (float(Fraction(swx, m * one)), float(Fraction(swy, m * one))),
            "velocity_variance": float(Fraction(vv * m - swx * swx - swy * swy, m * m * two))}


def self_test(div_samples=1 << 32):
    """pbSelfTest: fast exact sqrt/division forms vs the compiler's IEEE forms, on the GPU."""
    vals = [C.c_ulonglong() for _ in range(4)]
    _capi.check(_capi.lib().pbSelfTest(int(div_samples), *[C.byref(v) for v in vals]), "pbSelfTest")
    keys = ("sqrt_checked", "sqrt_mismatches", "div_checked", "div_mismatches")
    return {k: int(v.value) for k, v in zip(keys, vals)}


def _self_test(symbol, *args):
    """A self test of the (checked, mismatches) kind: the counts `symbol` writes after `args`, as a dict."""
    checked, bad = C.c_ulonglong(), C.c_ulonglong()
    _capi.check(getattr(_capi.lib(), symbol)(*args, C.byref(checked), C.byref(bad)), symbol)
    return {"checked": int(checked.value), "mismatches": int(bad.value)}


def self_test_hold_threshold(c):
    """pbSelfTestHoldThreshold: `sqrtf(x) < c` against `x < T(c)` on the GPU for every non-negative float x."""
    return _self_test("pbSelfTestHoldThreshold", float(c))


def self_test_magnitude_root():
    """pbSelfTestMagnitudeRoot: the unclamped one-Newton-step root of the both-sums form's attraction magnitude
    against sqrtf on the GPU for every float of [2^-96, FLT_MAX)."""
    return _self_test("pbSelfTestMagnitudeRoot")


def self_test_term_root():
    """pbSelfTestTermRoot: the both-sums form's in-trip root of a pair term's squared magnitude (contact terms
    included) on the GPU for all 2^32 bit patterns: guarded to sqrtf, or bit-equal to sqrtf."""
    return _self_test("pbSelfTestTermRoot")


def self_test_pair_geometry(first_slice=0, slices=64):
    """pbSelfTestPairGeometry: pbDistUnitFast against sqrtf and IEEE division on EVERY (d2, numerator)
    mantissa pair of `slices` of the 64 slices of d2 in [1, 4) (all 64: 2^47 pairs, ~90 s of one MI355X)."""
    return _self_test("pbSelfTestPairGeometry", int(first_slice), int(slices))


def self_test_division(first_slice=0, slices=64):
    """pbSelfTestDivision: pbDiv2Fast against IEEE division on EVERY (denominator, numerator) mantissa pair of
    `slices` of the 64 slices of the denominator range (all 64: 2^46 quotients)."""
    return _self_test("pbSelfTestDivision", int(first_slice), int(slices))


def force_forms():
    """The forms table of the exact per-step force kernel (pbForceFormCount / pbForceFormGet): a list of
    dicts flat / lanes_per_bot / attraction_sums / offsets64, index = row number."""
    L = _capi.lib()
    out = []
    for i in range(L.pbForceFormCount()):
        f = _capi.pbForceForm()
        _capi.check(L.pbForceFormGet(i, C.byref(f)), "pbForceFormGet")
        out.append(_capi.row_dict(f))
    return out


def force_form_kernel_name(index, payload=0):
    """Row `index` of the forms table as rocprofv3 names its kernel (pbForceFormKernelName; no device needed)."""
    buf = C.create_string_buffer(2048)
    _capi.check(_capi.lib().pbForceFormKernelName(int(index), int(payload), buf, len(buf)), "pbForceFormKernelName")
    return buf.value.decode()


def library_paths():
    return {"hip": _capi.HIP_SO, "host": _capi.HOST_SO}


class DeviceArray:
    """A caller-owned device buffer allocated through allocateArray() (particlebot.cuh:20)."""

    def __init__(self, shape, dtype=np.float32, fill=None):
        self.shape = tuple(np.atleast_1d(shape).tolist()) if not isinstance(shape, tuple) else shape
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        _capi.lib().allocateArray(C.byref(p), max(self.nbytes, 1))
        self.ptr = p
        if fill is not None:
            self.upload(np.full(self.shape, fill, dtype=self.dtype))

    @classmethod
    def from_host(cls, a):
        a = np.ascontiguousarray(a)
        d = cls(a.shape, a.dtype)
        d.upload(a)
        return d

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.nbytes == self.nbytes, (a.nbytes, self.nbytes)
        if self.nbytes:
            _capi.lib().copyArrayToDevice(self.ptr, _capi.np_ptr(a), 0, self.nbytes)

    def download(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if self.nbytes:
            _capi.lib().copyArrayFromDevice(_capi.np_ptr(out), self.ptr, None, self.nbytes)
        return out

    def free(self):
        if self.ptr is not None and self.ptr.value:
            _capi.lib().freeArray(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _Legacy:
    """The reference's `extern "C"` boundary (particlebot.cuh:15-121), one call per entry point.
    Arguments are DeviceArray objects; semantics are the reference's."""

    def __getattr__(self, name):
        return getattr(_capi.lib(), name)

    def set_parameters(self, params, wall_half=64.0):
        L = _capi.lib()
        L.pbSetWallHalfExtent(float(wall_half))
        L.setParameters(C.byref(params))

    def integrate(self, pos, vel, rad, dt, n, time=0.0):
        _capi.lib().integrateSystem(pos.ptr, vel.ptr, rad.ptr, dt, n, time)

    def calc_hash(self, hash_, index, pos, n):
        _capi.lib().calcHash(hash_.ptr, index.ptr, pos.ptr, n)

    def sort(self, hash_, index, n):
        _capi.lib().sortParticlebots(hash_.ptr, index.ptr, n)

    def reorder(self, cell_start, cell_end, spos, svel, srad, hash_, index, pos, vel, rad, n, num_cells):
        _capi.lib().reorderDataAndFindCellStart(cell_start.ptr, cell_end.ptr, spos.ptr, svel.ptr,
                                               srad.ptr, hash_.ptr, index.ptr, pos.ptr, vel.ptr,
                                               rad.ptr, n, num_cells)

    def update_rad(self, pos, abs_a, abs_r, rad, phase, time, dt, dead, n):
        _capi.lib().updateRad_light_wave(pos.ptr, abs_a.ptr, abs_r.ptr, rad.ptr, phase.ptr, time, dt,
                                        dead.ptr, n)

    def update_phase(self, pos, phase, spacing, max_d, min_d, n):
        _capi.lib().updatePhase(pos.ptr, phase.ptr, spacing, max_d, min_d, n)

    def rng_setup(self, state, n):
        _capi.lib().curand_setup(state.ptr, n)

    def add_noise(self, state, val, std, n):
        _capi.lib().add_normal_noise(state.ptr, val.ptr, std, n)

    def collide(self, new_vel, abs_a, abs_r, spos, svel, srad, index, cell_start, cell_end, n, num_cells, dt):
        _capi.lib().collide(new_vel.ptr, abs_a.ptr, abs_r.ptr, spos.ptr, svel.ptr, srad.ptr, index.ptr,
                           cell_start.ptr, cell_end.ptr, n, num_cells, dt)

    def sync(self):
        _capi.lib().threadSync()


legacy = _Legacy()


class ClockSample:
    """Shader clock held while the enclosed work runs (pbClockSampleBegin/End): a sleeping wave on its
    own stream spans `seconds` of real time; .mhz afterwards.  Diagnostic for the roofline report."""

    def __init__(self, seconds):
        self._h = C.c_void_p()
        _capi.check(_capi.lib().pbClockSampleBegin(C.byref(self._h), float(seconds)), "pbClockSampleBegin")

    def end(self):
        mhz, sec = C.c_double(), C.c_double()
        _capi.check(_capi.lib().pbClockSampleEnd(self._h, C.byref(mhz), C.byref(sec)), "pbClockSampleEnd")
        self._h = None
        self.mhz, self.seconds = mhz.value, sec.value
        return self.mhz


class Sim:
    """One resident simulation on the current GPU (pbSim* in include/particlebot_hip.h)."""

    nsims = 1  # members in the batch (an Ensemble has its own count)
    # a member's state, in pbSimGetStateOf's order: name -> (dtype, values per bot)
    _STATE = {"pos": (np.float32, 2), "vel": (np.float32, 2), "rad": (np.float32, 1), "phase": (np.float32, 1),
              "dead": (np.int32, 1), "absForce_a": (np.float32, 1), "absForce_r": (np.float32, 1)}

    def __init__(self, params, wall_half=0.0, keepalive=None):
        self._keep = keepalive
        self.params = params
        self.n = int(params.nCells)
        h = C.c_void_p()
        _capi.check(_capi.lib().pbSimCreate(C.byref(h), C.byref(params), float(wall_half)), "pbSimCreate")
        self._h = h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _capi.lib().pbSimDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _in(a, dtype, count):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
        assert a.size == count, (a.size, count)
        return a

    def _put(self, symbol, member, what, **arrays):
        """Upload arrays of one member's state (original bot order; None leaves an array as it is) through `symbol`,
        which takes them in the order given; `what` names the call in an error."""
        held = [self._in(a, self._STATE[k][0], self._STATE[k][1] * self.n) for k, a in arrays.items()]
        _capi.check(getattr(_capi.lib(), symbol)(self._h, int(member), *[_capi.np_ptr(a) for a in held]), what)

    def _get_state_of(self, member, out, what):
        """One member's state into `out` (None: a new dict); an array `out` lacks is made."""
        out = {} if out is None else out
        for k, (dtype, width) in self._STATE.items():
            if out.get(k) is None:
                out[k] = np.empty((self.n, width) if width > 1 else self.n, dtype)
        _capi.check(_capi.lib().pbSimGetStateOf(self._h, int(member), *[_capi.np_ptr(out[k]) for k in self._STATE]),
                    what)
        if not self.config()["attraction_sums"]:
            out["absForce_a"] = None  # a dead value in this batch: not maintained (set_force_sums)
        return out

    def set_state(self, pos=None, vel=None, rad=None, phase=None, dead=None):
        self._put("pbSimSetStateOf", 0, "pbSimSetState", pos=pos, vel=vel, rad=rad, phase=phase, dead=dead)

    def set_forces(self, absForce_a, absForce_r):
        """Overwrite absForce_a / absForce_r (original bot order): the two arrays the next step's
        radius actuation reads.  With set_state this restores a complete mid-run state."""
        self._put("pbSimSetForcesOf", 0, "pbSimSetForcesOf", absForce_a=absForce_a, absForce_r=absForce_r)

    def get_state(self, out=None):
        """The state in original bot order.  `out`: a dict returned by an earlier call, whose arrays are then
        written in place (a caller that reads back often keeps its host buffers: fresh pages cost more than
        the copy)."""
        return self._get_state_of(0, out, "pbSimGetState")

    # (per member, as every analysis takes `member`: a Sim is a batch of one, so anything that has nsims has these)
    def set_state_of(self, member, pos=None, vel=None, rad=None, phase=None, dead=None):
        self._put("pbSimSetStateOf", member, "pbSimSetStateOf", pos=pos, vel=vel, rad=rad, phase=phase, dead=dead)

    def get_state_of(self, member):
        return self._get_state_of(member, None, "pbSimGetStateOf")

    @property
    def time(self):
        t = C.c_float()
        _capi.check(_capi.lib().pbSimGetTime(self._h, C.byref(t)))
        return t.value

    @time.setter
    def time(self, t):
        _capi.check(_capi.lib().pbSimSetTime(self._h, float(t)))

    @property
    def phase_draws(self):
        d = C.c_uint()
        _capi.check(_capi.lib().pbSimGetPhaseDraws(self._h, C.byref(d)))
        return d.value

    @phase_draws.setter
    def phase_draws(self, d):
        _capi.check(_capi.lib().pbSimSetPhaseDraws(self._h, int(d)))

    def step(self, nsteps, dt=0.01, sort_interval=180.0):
        done = C.c_int()
        _capi.check(_capi.lib().pbSimStep(self._h, dt, sort_interval, int(nsteps), C.byref(done)), "pbSimStep")
        return done.value

    def step_timed(self, nsteps, dt=0.01, sort_interval=180.0):
        done = C.c_int()
        ms = C.c_float()
        _capi.check(_capi.lib().pbSimStepTimed(self._h, dt, sort_interval, int(nsteps), C.byref(done),
                                               C.byref(ms)), "pbSimStepTimed")
        return done.value, ms.value

    def step_timed_wall(self, nsteps, dt=0.01, sort_interval=180.0):
        """(steps done, device ms between HIP events, host wall ms from entry to the drained stream) of the same
        launches (pbSimStepTimedWall): synchronise before calling."""
        done, ms, wall = C.c_int(), C.c_float(), C.c_double()
        _capi.check(_capi.lib().pbSimStepTimedWall(self._h, dt, sort_interval, int(nsteps), C.byref(done), C.byref(ms),
                                                   C.byref(wall)), "pbSimStepTimedWall")
        return done.value, ms.value, wall.value

    def synchronize(self):
        _capi.check(_capi.lib().pbSimSynchronize(self._h))

    def centroid(self):
        cx, cy = C.c_double(), C.c_double()
        _capi.check(_capi.lib().pbSimCentroid(self._h, C.byref(cx), C.byref(cy)), "pbSimCentroid")
        return cx.value, cy.value

    def stats(self):
        s = pbSimStats()
        _capi.check(_capi.lib().pbSimGetStats(self._h, C.byref(s)))
        return _capi.row_dict(s)

    def config(self):
        """What the next step() launches: force_variant / force_kind / lanes_per_bot / resident /
        fast_math_ok / payload / rng (pbSimGetConfig)."""
        c = pbSimConfig()
        _capi.check(_capi.lib().pbSimGetConfig(self._h, C.byref(c)))
        return _capi.row_dict(c)

    def force_kernel_name(self):
        """The per-step force kernel the next step() launches, as rocprofv3 names it (pbSimForceKernelName)."""
        buf = C.create_string_buffer(2048)
        _capi.check(_capi.lib().pbSimForceKernelName(self._h, buf, len(buf)), "pbSimForceKernelName")
        return buf.value.decode()

    def set_force_variant(self, variant):
        """0/1/2: exact kernels (bit-identical to the oracle; 2 is the default).  3: streamlined
        arithmetic, opt-in, not bit-identical (include/particlebot_hip.h)."""
        _capi.check(_capi.lib().pbSimSetForceVariant(self._h, int(variant)))

    def set_stream_walk(self, mode):
        """-1 (default): the streamlined kernel's neighbour walk is chosen at every re-sort; 0 row by row; 1 flattened
        (pbSimSetStreamWalk; bit-identical either way)."""
        _capi.check(_capi.lib().pbSimSetStreamWalk(self._h, int(mode)), "pbSimSetStreamWalk")

    def stream_walk_trips(self):
        """(row-by-row, flattened) trips per wave summed over the batch, from the last automatic choice."""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        _capi.check(_capi.lib().pbSimGetStreamWalkTrips(self._h, C.byref(a), C.byref(b)), "pbSimGetStreamWalkTrips")
        return a.value, b.value

    def set_force_sums(self, mode):
        """0 (default): absForce_a only when a member reads it (constrained_contraction); otherwise it
        is a dead value, not computed, and get_state() returns NaN for it.  1: always maintained."""
        _capi.check(_capi.lib().pbSimSetForceSums(self._h, int(mode)))

    def select_force_form(self, index):
        """Pin the batch to row `index` of the force-kernel forms table (force_forms()); -1: automatic."""
        _capi.check(_capi.lib().pbSimSelectForceForm(self._h, int(index)), "pbSimSelectForceForm")

    def set_lanes_per_bot(self, lanes):
        _capi.check(_capi.lib().pbSimSetLanesPerBot(self._h, int(lanes)))

    def set_tail_tiles(self, tiles):
        """Split-lane tail tiles per XCD of the throughput form: -1 automatic (default), 0 off, else that many
        (pbSimSetTailTiles; bit-identical either way).  config()["tail_tiles"] is what the next step uses."""
        _capi.check(_capi.lib().pbSimSetTailTiles(self._h, int(tiles)), "pbSimSetTailTiles")

    def set_resident(self, mode):
        """0 automatic, 1 never, 2 whenever the simulation fits one workgroup (<= 1024 bots)."""
        _capi.check(_capi.lib().pbSimSetResident(self._h, int(mode)))

    def set_resort_every_step(self, on):
        _capi.check(_capi.lib().pbSimSetResortEveryStep(self._h, 1 if on else 0))

    def colors(self, member=0):
        """The reference's updateCol colours of one member, (n, 4) float32 RGBA in original order, computed now from
        its state (alpha 1)."""
        out = np.empty((self.n, 4), np.float32)
        _capi.check(_capi.lib().pbSimGetColorsOf(self._h, int(member), _capi.np_ptr(out)), "pbSimGetColorsOf")
        return out

    def set_centroid_trail(self, on):
        """Record the reference's centroid trail (calcCOG) every centroid_int seconds into a ring of centroid_steps."""
        _capi.check(_capi.lib().pbSimSetCentroidTrail(self._h, 1 if on else 0), "pbSimSetCentroidTrail")

    def centroid_trail(self, member=0):
        """(xy, times, records): the ring verbatim ((centroid_steps, 2) float32, y still + 2000), the fp32 start time of
        the step that wrote each slot (NaN: never written) and the number of records so far."""
        steps = int(self.params.centroid_steps)
        xy = np.empty((steps, 2), np.float32)
        times = np.empty(steps, np.float32)
        rec = C.c_uint(0)
        _capi.check(_capi.lib().pbSimGetCentroidTrailOf(self._h, int(member), _capi.np_ptr(xy), _capi.np_ptr(times),
                                                        C.byref(rec)), "pbSimGetCentroidTrailOf")
        return xy, times, int(rec.value)

    def render(self, width, height, center=(0.0, 0.0), half_extent=1.0, light_radius=0.25, style="plain", member=0):
        """One frame of `member` rasterised on the device from the resident state (pbSimRenderOf): uint8
        [height, width, 3], byte for byte the host frame writer's picture of the same state.  style "reference": the
        device colours, and the centroid trail when set_centroid_trail(True)."""
        if style not in ("plain", "reference"):
            raise ValueError(style)
        view = _capi.pbRenderView(int(width), int(height), float(center[0]), float(center[1]), float(half_extent),
                                  float(light_radius), 1 if style == "reference" else 0)
        out = np.empty((int(height), int(width), 3), np.uint8)
        _capi.check(_capi.lib().pbSimRenderOf(self._h, int(member), C.byref(view), _capi.np_ptr(out)), "pbSimRenderOf")
        return out

    def _span(self, symbol):
        """(count so far, device milliseconds of the last one) as the span clock behind `symbol` holds them."""
        n, ms = C.c_ulonglong(0), C.c_float(0.0)
        _capi.check(getattr(_capi.lib(), symbol)(self._h, C.byref(n), C.byref(ms)), symbol)
        return int(n.value), float(ms.value)

    def render_stats(self):
        """(frames rendered, device milliseconds of the last frame's launches)."""
        return self._span("pbSimGetRenderStats")

    def clusters(self, gap=0.0):
        """Cluster analysis of every member's state as it is now, on the device (pbSimClusterStats): a list of dicts
        (clusters, largest, largest_label, isolated, links, max_degree, rounds), one per member."""
        rows = (_capi.pbClusterStats * self.nsims)()
        _capi.check(_capi.lib().pbSimClusterStats(self._h, float(gap), rows), "pbSimClusterStats")
        return [_capi.row_dict(r) for r in rows]

    def cluster_labels(self, gap=0.0, member=0):
        """(labels, degree) of one member: uint32 arrays in original bot order (pbSimClusterLabelsOf)."""
        out = _analysis.per_bot(_analysis.CLUSTER_LABELS, self.n, lambda *p: _capi.check(
            _capi.lib().pbSimClusterLabelsOf(self._h, int(member), float(gap), *p), "pbSimClusterLabelsOf"))
        return out["labels"], out["degree"]

    def cluster_times(self):
        """(analyses run so far, device milliseconds of the last one)."""
        return self._span("pbSimGetClusterTimes")

    def contacts(self, gap=0.0, member=0):
        """The contact network of one member's state as it is now, from the device (pbSimContactsOf): a dict with
        offsets (uint32, n + 1: a CSR adjacency in original bot order, ascending `other` per bot), other (uint32, E),
        gap (float32, E: dist - (ri + rj), negative in contact) and force (float32, E x 2: the pair law's force ON the
        owning bot FROM other).  Every undirected link appears twice, once under each end."""
        return _analysis.contacts(self.n, lambda *a: _capi.check(
            _capi.lib().pbSimContactsOf(self._h, int(member), float(gap), *a), "pbSimContactsOf"))

    def contact_virial(self, gap=0.0, member=0):
        """Per-bot virial of one member's contact network (pbSimContactVirialOf): float64, n x 4, the columns
        sxx = sum rx fx, sxy = sum rx fy, syx = sum ry fx, syy = sum ry fy over the bot's entries in CSR order."""
        out = np.empty((self.n, 4), np.float64)
        _capi.check(_capi.lib().pbSimContactVirialOf(self._h, int(member), float(gap), _capi.np_ptr(out)),
                    "pbSimContactVirialOf")
        return out

    def contact_times(self):
        """(exports run so far, device milliseconds of the last one)."""
        return self._span("pbSimGetContactTimes")

    def radial_counts(self, r_max, bins, member=None):
        """Radial pair counts of every member's state as it is now, on the device (pbSimRadialCounts): uint64,
        (nsims, bins), or (bins,) for one member.  The ordered pair (i, j) is in bin int(dist * (float32(bins) / r_max))
        in fp32; every count is even.  radial_distribution() turns them into g(r)."""
        out = np.zeros((self.nsims, int(bins)), np.uint64)
        _capi.check(_capi.lib().pbSimRadialCounts(self._h, float(r_max), int(bins), _capi.np_ptr(out)),
                    "pbSimRadialCounts")
        return out if member is None else out[int(member)]

    def structure(self, gap=0.0):
        """Hexatic order of every member's state as it is now, on the device (pbSimStructureStats): a list of dicts, one
        per member: bonds (directed), psi6_re / psi6_im (sums in units of 2^-30), coordination (bots with 0..6 and 7 or
        more neighbours) and psi6, the complex mean over the bonds.  Bonds are the cluster analysis' links for `gap`."""
        rows = (_capi.pbStructureStats * self.nsims)()
        _capi.check(_capi.lib().pbSimStructureStats(self._h, float(gap), rows), "pbSimStructureStats")
        return [_capi.structure_row(r) for r in rows]

    def hexatic(self, gap=0.0, member=0):
        """(psi6, neighbours) of one member: complex128[n] and uint32[n] in original bot order (pbSimHexaticOf); psi6 of
        a bot is the mean of e^(6 i theta) over its bonds, 0 without neighbours."""
        out = _analysis.per_bot(_analysis.HEXATIC, self.n, lambda *p: _capi.check(
            _capi.lib().pbSimHexaticOf(self._h, int(member), float(gap), *p), "pbSimHexaticOf"))
        return out["psi6"], out["neighbours"]

    def structure_times(self):
        """(structure analyses run so far, device milliseconds of the last one)."""
        return self._span("pbSimGetStructureTimes")

    def mark_reference(self, gap=0.0):
        """Keep every member's positions and link network at `gap` on the device as the reference that rearrangement()
        compares against (pbSimMarkReference).  A new mark replaces the old one; re-sorts and set_state do not
        invalidate it; it is not part of a checkpoint."""
        _capi.check(_capi.lib().pbSimMarkReference(self._h, float(gap)), "pbSimMarkReference")

    def clear_reference(self):
        """Free the mark (pbSimClearReference)."""
        _capi.check(_capi.lib().pbSimClearReference(self._h), "pbSimClearReference")

    def reference_info(self):
        """The mark held: a dict of marked (bool), gap, time (fp32, when it was taken) and entries (directed links of
        the whole batch); zeros without one (pbSimGetReferenceInfo)."""
        held, gap, t, e = C.c_int(0), C.c_float(0.0), C.c_float(0.0), C.c_ulonglong(0)
        _capi.check(_capi.lib().pbSimGetReferenceInfo(self._h, C.byref(held), C.byref(gap), C.byref(t), C.byref(e)),
                    "pbSimGetReferenceInfo")
        return {"marked": bool(held.value), "gap": float(gap.value), "time": float(t.value), "entries": int(e.value)}

    def rearrangement(self):
        """Every member's state as it is now against the mark, on the device (pbSimRearrangementStats): a list of dicts,
        one per member: bonds_marked / bonds_now / bonds_kept (directed links at the mark, now, and in both),
        bots_unchanged / bots_lost / bots_gained, measured, sum_qx / sum_qy (displacement sums, units of 2^-20), sum_q2
        (the sum of squared displacements as one Python int, units of 2^-40) and max_q2.  mean_squared_displacement()
        turns a row into the MSD."""
        rows = (_capi.pbRearrangementStats * self.nsims)()
        _capi.check(_capi.lib().pbSimRearrangementStats(self._h, rows), "pbSimRearrangementStats")
        return [_capi.rearrangement_row(r) for r in rows]

    def rearrangement_of(self, member=0):
        """One member per bot, original order (pbSimRearrangementOf): a dict of disp (float32, n x 2: dx, dy since the
        mark, verbatim) and marked, now, kept (uint32: the bot's links at the mark, now, and in both)."""
        return _analysis.per_bot(_analysis.REARRANGEMENT_OF, self.n, lambda *p: _capi.check(
            _capi.lib().pbSimRearrangementOf(self._h, int(member), *p), "pbSimRearrangementOf"))

    def rearrangement_times(self):
        """(marks and compares run so far, device milliseconds of the last one)."""
        return self._span("pbSimGetRearrangementTimes")

    def strain(self, threshold=0.0):
        """Every member's local strain and non-affine displacement against the mark, on the device (pbSimStrainStats):
        a list of dicts of Python ints, one per member: fitted / unfitted (bots with and without a Falk-Langer fit),
        above (fitted bots with D2min > threshold, in world units squared), bonds_used / bonds_dropped, the sums yxx,
        yxy, yyy, xxx, xxy, xyx, xyy, w of the moments over all used bonds, sum_d2 and max_d2 (all in units of 2^-40).
        deformation_gradient() and mean_d2min() turn a row into floats."""
        rows = (_capi.pbStrainStats * self.nsims)()
        _capi.check(_capi.lib().pbSimStrainStats(self._h, float(threshold), rows), "pbSimStrainStats")
        return [_capi.row_dict(r) for r in rows]

    def strain_of(self, member=0):
        """One member per bot, original order (pbSimStrainOf): a dict of moments (int64, n x 9: k, Yxx, Yxy, Yyy, Xxx,
        Xxy, Xyx, Xyy, W), gradient (float64, n x 2 x 2: the local deformation gradient J, zero for an unfitted bot) and
        d2min (float64, units of 2^-40: the device's value)."""
        return _analysis.per_bot(_analysis.STRAIN_OF, self.n, lambda *p: _capi.check(
            _capi.lib().pbSimStrainOf(self._h, int(member), *p), "pbSimStrainOf"))

    def strain_times(self):
        """(strain analyses run so far, device milliseconds of the last one)."""
        return self._span("pbSimGetStrainTimes")

    def moments(self):
        """Every member's row of integer moments of the state as it is now, from the device (pbSimMoments): a list of
        dicts of Python ints, one per member: time, step, measured, sum_qx / sum_qy / sum_qr / sum_wx / sum_wy (units of
        2^-20), the box min_qx / max_qx / min_qy / max_qy, and xx, yy, xy, rr, vv (the 128-bit sums composed, units of
        2^-40).  moments_summary() turns a row into centroid, gyration tensor, radii and velocities."""
        rows = (_capi.pbMomentsRow * self.nsims)()
        _capi.check(_capi.lib().pbSimMoments(self._h, rows), "pbSimMoments")
        return [_capi.row_dict(r) for r in rows]

    def set_series(self, interval, capacity):
        """Record such a row per member into a device ring of `capacity` rows in front of every step whose start time
        passes the schedule's gate at `interval` (0: every step) while step() runs (pbSimSetSeries).  Restarts the
        series at record 0; capacity 0 switches it off.  Recording changes no state bit."""
        _capi.check(_capi.lib().pbSimSetSeries(self._h, float(interval), int(capacity)), "pbSimSetSeries")

    def series_info(self):
        """A dict of interval, capacity (0: off) and records taken so far (pbSimGetSeriesInfo)."""
        return _analysis.read_info(_analysis.SERIES_INFO, lambda *p: _capi.check(
            _capi.lib().pbSimGetSeriesInfo(self._h, *p), "pbSimGetSeriesInfo"))

    def series_of(self, member=0, first=None, count=None):
        """Records first .. first + count of one member in the order taken, as moments() gives rows (pbSimGetSeriesOf).
        first defaults to the oldest record the ring still holds, count to everything from `first` on."""
        info = self.series_info()
        if first is None:
            first = info["records"] - min(info["records"], info["capacity"])
        if count is None:
            count = max(info["records"] - int(first), 0)
        rows = (_capi.pbMomentsRow * max(int(count), 1))()
        _capi.check(_capi.lib().pbSimGetSeriesOf(self._h, int(member), int(first), int(count), rows), "pbSimGetSeriesOf")
        return [_capi.row_dict(r) for r in rows[:int(count)]]

    def series_times(self):
        """(records taken so far, device milliseconds of the last row's launches)."""
        return self._span("pbSimGetSeriesTimes")

    def pair_correlation(self, kind, r_max, bins, member=None):
        """Pair correlations of every member's state as it is now, on the device (pbSimPairCorrelation): all pairs binned
        by distance as radial_counts bins them, with the sums of a_i . a_j per bin.  kind: "velocity" (a = v),
        "displacement" (a = the displacement since mark_reference) or "radius" (a = (rad, 0)), or the PB_CORR_* int; a is
        in units of 2^-20.  Returns (rows, totals): rows a structured array (nsims, bins) of pairs, dot_lo / dot_hi,
        ax_lo / ax_hi, ay_lo / ay_hi (each 128-bit value is hi * 2^32 + lo with 0 <= lo < 2^32; correlation_values()
        composes them), totals a list of dicts (measured, sum_ax, sum_ay, sum_a2, pairs), one per member; with member=k
        that member's (bins,) rows and its dict.  connected_correlation() turns both into C(r)."""
        rows = np.zeros((self.nsims, max(int(bins), 1)), _capi.CORRELATION_BIN_DTYPE)
        tot = (_capi.pbCorrelationTotals * self.nsims)()
        _capi.check(_capi.lib().pbSimPairCorrelation(self._h, _capi.correlation_kind(kind), float(r_max), int(bins),
                                                     _capi.np_ptr(rows), tot), "pbSimPairCorrelation")
        totals = [_capi.row_dict(t) for t in tot]
        return (rows, totals) if member is None else (rows[int(member)], totals[int(member)])

    def correlation_times(self):
        """(pair correlations run so far, device milliseconds of the last one)."""
        return self._span("pbSimGetCorrelationTimes")

    def set_time_correlation(self, interval, lags, overlap_radius):
        """Keep a device ring of `lags` snapshots (x, y, vx, vy of every bot, original order), one taken in front of
        every step whose start time passes the schedule's gate at `interval` (0: every step, -1: only by
        time_correlation_record()) while step() runs, and add every record against the `lags` latest ones into a table
        per member and lag (pbSimSetTimeCorrelation).  overlap_radius is the a of the overlap function.  Restarts at
        record 0; lags 0 switches it off.  Recording changes no state bit."""
        _capi.check(_capi.lib().pbSimSetTimeCorrelation(self._h, float(interval), int(lags), float(overlap_radius)),
                    "pbSimSetTimeCorrelation")

    def time_correlation_record(self):
        """One record now, of the state as it is (pbSimTimeCorrelationRecord)."""
        _capi.check(_capi.lib().pbSimTimeCorrelationRecord(self._h), "pbSimTimeCorrelationRecord")

    def time_correlation_info(self):
        """A dict of interval, lags (0: off), overlap_radius and records taken so far (pbSimGetTimeCorrelationInfo)."""
        return _analysis.read_info(_analysis.TIME_CORRELATION_INFO, lambda *p: _capi.check(
            _capi.lib().pbSimGetTimeCorrelationInfo(self._h, *p), "pbSimGetTimeCorrelationInfo"))

    def time_correlation(self):
        """The table as it stands (pbSimGetTimeCorrelation): per member a list of `lags` dicts of Python ints, lag 0
        first: lag, origins, sum_steps, samples, sum_qx / sum_qy (units of 2^-20), msd and vacf (the 128-bit sums
        composed, units of 2^-40), overlap, max_q2.  time_correlation_summary() turns a row into MSD, VACF and Q."""
        lags = self.time_correlation_info()["lags"]
        rows = (_capi.pbTimeCorrelationRow * max(self.nsims * lags, 1))()
        _capi.check(_capi.lib().pbSimGetTimeCorrelation(self._h, rows), "pbSimGetTimeCorrelation")
        return _analysis.lag_table(self.nsims, lags, lambda g: _capi.row_dict(rows[g]))

    def time_correlation_times(self):
        """(records taken so far, device milliseconds of the last record's launches)."""
        return self._span("pbSimGetTimeCorrelationTimes")

    def field_map(self, nx, ny, center, half, member=None):
        """A field map of every member's state as it is now, on the device (pbSimFieldMap): nx x ny cells over the view
        centred on center = (x, y) with half extent `half` (one number, or (halfX, halfY)).  Returns (cells, totals):
        cells a structured array (nsims, ny, nx), row 0 the lowest y, of count, dead, sum_qr, sum_wx, sum_wy (units of
        2^-20) and rr_lo / rr_hi, vv_lo / vv_hi (each 128-bit value is hi * 2^32 + lo with 0 <= lo < 2^32, units of
        2^-40; field_values() composes them into Python ints); totals a list of dicts (measured, inside, outside,
        unmeasured), one per member.  With member=k only that member is mapped (pbSimFieldMapOf): its (ny, nx) cells and
        its dict."""
        view = _capi.field_view(nx, ny, center, half)
        if member is not None:
            cells, tot = _analysis.field_cells(1, nx, ny)[0], _capi.pbFieldTotals()
            _capi.check(_capi.lib().pbSimFieldMapOf(self._h, int(member), C.byref(view), _capi.np_ptr(cells),
                                                    C.byref(tot)), "pbSimFieldMapOf")
            return cells, _capi.row_dict(tot)
        cells, tot = _analysis.field_cells(self.nsims, nx, ny), (_capi.pbFieldTotals * self.nsims)()
        _capi.check(_capi.lib().pbSimFieldMap(self._h, C.byref(view), _capi.np_ptr(cells), tot), "pbSimFieldMap")
        return cells, [_capi.row_dict(t) for t in tot]

    def field_times(self):
        """(field maps computed so far, device milliseconds of the last one's launches)."""
        return self._span("pbSimGetFieldTimes")

    def structure_factor(self, vectors, box_log2, kind="density", member=None):
        """The structure factor of every member's state as it is now, on the device (pbSimStructureFactor): per member
        and wavevector k = (2 pi / 2^box_log2)(nx, ny) of `vectors`, an (nvec, 2) array of ints, the exact integer sums
        of a exp(i k.r) over the measured bots, the phasor being an entry of phasor_table().  kind: "density" (a = 1),
        "radius" (a = the quantised radius) or "velocity" (a = wx into re / im, wy into re2 / im2).  Returns a
        structured array (nsims, nvec) of nx, ny, measured and re_lo / re_hi, im_lo / im_hi, re2_lo / re2_hi, im2_lo /
        im2_hi (each 128-bit value is hi * 2^32 + lo with 0 <= lo < 2^32; units of 2^-30 for the density, 2^-50
        otherwise; structure_factor_values() composes them and S(k)).  With member=k only that member's (nvec,) rows
        (pbSimStructureFactorOf)."""
        (held, nvec), code = _analysis.held_vectors(vectors), _capi.sk_kind(kind)
        ptr = _capi.np_ptr(held)
        if member is not None:
            rows = _analysis.structure_factor_rows(1, nvec)[0]
            _capi.check(_capi.lib().pbSimStructureFactorOf(self._h, int(member), code, int(box_log2), ptr, nvec,
                                                           _capi.np_ptr(rows)), "pbSimStructureFactorOf")
            return rows
        rows = _analysis.structure_factor_rows(self.nsims, nvec)
        _capi.check(_capi.lib().pbSimStructureFactor(self._h, code, int(box_log2), ptr, nvec, _capi.np_ptr(rows)),
                    "pbSimStructureFactor")
        return rows

    def structure_factor_times(self):
        """(structure factors computed so far, device milliseconds of the last one's launches)."""
        return self._span("pbSimGetStructureFactorTimes")

    def set_scattering(self, interval, lags, box_log2, vectors):
        """Keep a device ring of `lags` snapshots of the quantised positions (original order), one taken in front of
        every step whose start time passes the schedule's gate at `interval` (0: every step, -1: only by
        scattering_record()) while step() runs, and add every record against the `lags` latest ones into a table per
        member, lag and wavevector k = (2 pi / 2^box_log2)(nx, ny) of `vectors`, an (nvec, 2) array of ints, nvec
        1 ... 256 (pbSimSetScattering): the self-intermediate scattering function as exact integer phasor sums.
        Restarts at record 0; lags 0 switches it off (vectors may then be None).  Recording changes no state bit."""
        if int(lags) == 0 and vectors is None:
            vectors = np.zeros((0, 2), np.int32)
        held, nvec = _analysis.held_vectors(vectors)
        _capi.check(_capi.lib().pbSimSetScattering(self._h, float(interval), int(lags), int(box_log2),
                                                   _capi.np_ptr(held), nvec), "pbSimSetScattering")

    def scattering_record(self):
        """One record now, of the state as it is (pbSimScatteringRecord)."""
        _capi.check(_capi.lib().pbSimScatteringRecord(self._h), "pbSimScatteringRecord")

    def scattering_info(self):
        """A dict of interval, lags (0: off), box_log2, nvec and records taken so far (pbSimGetScatteringInfo)."""
        return _analysis.read_info(_analysis.SCATTERING_INFO, lambda *p: _capi.check(
            _capi.lib().pbSimGetScatteringInfo(self._h, *p), "pbSimGetScatteringInfo"))

    def scattering(self):
        """The table as it stands (pbSimGetScattering): per member a list over lags (lag 0 first) of lists over the
        vectors (list order) of dicts of Python ints: lag, nx, ny, origins, sum_steps, samples, re, im (units of 2^-30).
        scattering_summary() turns a row into F_s."""
        info = self.scattering_info()
        lags, nvec = info["lags"], info["nvec"]
        rows = (_capi.pbScatteringRow * max(self.nsims * lags * nvec, 1))()
        _capi.check(_capi.lib().pbSimGetScattering(self._h, rows), "pbSimGetScattering")
        return _analysis.lag_table(self.nsims, lags, lambda g: _capi.row_dict(rows[g]), nvec)

    def scattering_times(self):
        """(records taken so far, device milliseconds of the last record's launches)."""
        return self._span("pbSimGetScatteringTimes")

    def set_van_hove(self, interval, lags, width, bins):
        """Keep a device ring of `lags` snapshots of the positions (original order), one taken in front of every step
        whose start time passes the schedule's gate at `interval` (0: every step, -1: only by van_hove_record()) while
        step() runs, and add every record against the `lags` latest ones into a table per member and lag
        (pbSimSetVanHove): the self van Hove function as exact integer histograms of the displacement's length (`bins`
        bins of `width`) and of its x and y components (2 bins each, from -bins width to bins width), with the sums of
        its second and fourth powers.  Restarts at record 0; lags 0 switches it off.  Recording changes no state bit."""
        _capi.check(_capi.lib().pbSimSetVanHove(self._h, float(interval), int(lags), float(width), int(bins)),
                    "pbSimSetVanHove")

    def van_hove_record(self):
        """One record now, of the state as it is (pbSimVanHoveRecord)."""
        _capi.check(_capi.lib().pbSimVanHoveRecord(self._h), "pbSimVanHoveRecord")

    def van_hove_info(self):
        """A dict of interval, lags (0: off), width, bins and records taken so far (pbSimGetVanHoveInfo)."""
        return _analysis.read_info(_analysis.VAN_HOVE_INFO, lambda *p: _capi.check(
            _capi.lib().pbSimGetVanHoveInfo(self._h, *p), "pbSimGetVanHoveInfo"))

    def van_hove(self):
        """The table as it stands (pbSimGetVanHove): per member a list over lags (lag 0 first) of dicts of Python ints:
        lag, origins, sum_steps, samples, beyond_r, beyond_x, beyond_y, msd (units of 2^-40), q4 (units of 2^-80), and
        the histograms radial (bins ints), x and y (2 bins ints each, index j covering [(j - bins) width,
        (j - bins + 1) width)) as lists.  van_hove_summary() turns a row into msd and alpha2."""
        info = self.van_hove_info()
        lags, bins = info["lags"], info["bins"]
        rows = (_capi.pbVanHoveRow * max(self.nsims * lags, 1))()
        counts = (C.c_ulonglong * max(self.nsims * lags * 5 * bins, 1))()
        _capi.check(_capi.lib().pbSimGetVanHove(self._h, rows, counts), "pbSimGetVanHove")
        return van_hove_lists(rows, counts, self.nsims, lags, bins)

    def van_hove_times(self):
        """(records taken so far, device milliseconds of the last record's launches)."""
        return self._span("pbSimGetVanHoveTimes")

    def set_van_hove_distinct(self, interval, lags, width, bins):
        """Keep a device ring of `lags` snapshots of the positions, taken as set_van_hove() takes them, and add every
        record against the `lags` latest ones into a table per member and lag (pbSimSetVanHoveDistinct): the distinct van
        Hove function as exact integer counts of the ordered pairs (a bot then, ANOTHER bot now) by distance, `bins` bins
        of `width` with bins * width below 2048.  Restarts at record 0; lags 0 switches it off.  Recording changes no
        state bit."""
        _capi.check(_capi.lib().pbSimSetVanHoveDistinct(self._h, float(interval), int(lags), float(width), int(bins)),
                    "pbSimSetVanHoveDistinct")

    def van_hove_distinct_record(self):
        """One record now, of the state as it is (pbSimVanHoveDistinctRecord)."""
        _capi.check(_capi.lib().pbSimVanHoveDistinctRecord(self._h), "pbSimVanHoveDistinctRecord")

    def van_hove_distinct_info(self):
        """A dict of interval, lags (0: off), width, bins and records taken so far (pbSimGetVanHoveDistinctInfo)."""
        return _analysis.read_info(_analysis.VAN_HOVE_DISTINCT_INFO, lambda *p: _capi.check(
            _capi.lib().pbSimGetVanHoveDistinctInfo(self._h, *p), "pbSimGetVanHoveDistinctInfo"))

    def van_hove_distinct(self):
        """The table as it stands (pbSimGetVanHoveDistinct): per member a list over lags (lag 0 first) of dicts of Python
        ints: lag, origins, sum_steps, centres, partners, pairs, and counts (bins ints; bin k covers
        [k width, (k + 1) width))."""
        info = self.van_hove_distinct_info()
        lags, bins = info["lags"], info["bins"]
        rows = (_capi.pbVanHoveDistinctRow * max(self.nsims * lags, 1))()
        counts = (C.c_ulonglong * max(self.nsims * lags * bins, 1))()
        _capi.check(_capi.lib().pbSimGetVanHoveDistinct(self._h, rows, counts), "pbSimGetVanHoveDistinct")
        return van_hove_distinct_lists(rows, counts, self.nsims, lags, bins)

    def van_hove_distinct_times(self):
        """(records taken so far, device milliseconds of the last record's launches)."""
        return self._span("pbSimGetVanHoveDistinctTimes")

    def set_coherent_scattering(self, interval, lags, box_log2, vectors):
        """Keep a device ring of `lags` records of the density modes rho(k) = sum exp(i k.r) of every member, one taken
        in front of every step whose start time passes the schedule's gate at `interval` (0: every step, -1: only by
        coherent_scattering_record()) while step() runs, and add the product of every record's modes with those of
        the `lags` latest ones into a table per member, lag and wavevector k = (2 pi / 2^box_log2)(nx, ny) of
        `vectors`, an (nvec, 2) array of ints, nvec 1 ... 256 (pbSimSetCoherent): the coherent intermediate scattering
        function as exact 192-bit integer sums.  Restarts at record 0; lags 0 switches it off (vectors may then be
        None).  Recording changes no state bit."""
        if int(lags) == 0 and vectors is None:
            vectors = np.zeros((0, 2), np.int32)
        held, nvec = _analysis.held_vectors(vectors)
        _capi.check(_capi.lib().pbSimSetCoherent(self._h, float(interval), int(lags), int(box_log2),
                                                 _capi.np_ptr(held), nvec), "pbSimSetCoherent")

    def coherent_scattering_record(self):
        """One record now, of the state as it is (pbSimCoherentRecord)."""
        _capi.check(_capi.lib().pbSimCoherentRecord(self._h), "pbSimCoherentRecord")

    def coherent_scattering_info(self):
        """A dict of interval, lags (0: off), box_log2, nvec and records taken so far (pbSimGetCoherentInfo)."""
        return _analysis.read_info(_analysis.COHERENT_INFO, lambda *p: _capi.check(
            _capi.lib().pbSimGetCoherentInfo(self._h, *p), "pbSimGetCoherentInfo"))

    def coherent_scattering(self):
        """The table as it stands (pbSimGetCoherent): per member a list over lags (lag 0 first) of lists over the
        vectors (list order) of dicts of Python ints: lag, nx, ny, origins, sum_steps, bots_now, bots_then, re, im
        (units of 2^-60).  coherent_scattering_summary() turns a row into F."""
        info = self.coherent_scattering_info()
        lags, nvec = info["lags"], info["nvec"]
        rows = (_capi.pbCoherentRow * max(self.nsims * lags * nvec, 1))()
        _capi.check(_capi.lib().pbSimGetCoherent(self._h, rows), "pbSimGetCoherent")
        return _analysis.lag_table(self.nsims, lags, lambda g: _capi.coherent_row(rows[g]), nvec)

    def coherent_scattering_times(self):
        """(records taken so far, device milliseconds of the last record's launches)."""
        return self._span("pbSimGetCoherentTimes")

    def set_four_point(self, interval, lags, overlap_radius, box_log2, vectors):
        """Keep a device ring of `lags` records of every bot's quantised position, one taken in front of every step
        whose start time passes the schedule's gate at `interval` (0: every step, -1: only by four_point_record())
        while step() runs, and per pair of a record with one of the `lags` latest ones form the overlap count Q (bots
        within `overlap_radius`, in [0, 2048), of where they were) and, per wavevector
        k = (2 pi / 2^box_log2)(nx, ny) of `vectors`, an (nvec, 2) array of ints, nvec 1 ... 256, the density mode of the
        overlapping bots at their earlier positions; Q, Q^2, the modes and their squared magnitudes are summed over the
        origins as exact integers (pbSimSetFourPoint): chi_4 and S_4(k, lag).  Restarts at record 0; lags 0 switches it
        off (vectors may then be None).  Recording changes no state bit."""
        if int(lags) == 0 and vectors is None:
            vectors = np.zeros((0, 2), np.int32)
        held, nvec = _analysis.held_vectors(vectors)
        _capi.check(_capi.lib().pbSimSetFourPoint(self._h, float(interval), int(lags), float(overlap_radius),
                                                  int(box_log2), _capi.np_ptr(held), nvec), "pbSimSetFourPoint")

    def four_point_record(self):
        """One record now, of the state as it is (pbSimFourPointRecord)."""
        _capi.check(_capi.lib().pbSimFourPointRecord(self._h), "pbSimFourPointRecord")

    def four_point_info(self):
        """A dict of interval, lags (0: off), overlap_radius, box_log2, nvec and records taken so far
        (pbSimGetFourPointInfo)."""
        return _analysis.read_info(_analysis.FOUR_POINT_INFO, lambda *p: _capi.check(
            _capi.lib().pbSimGetFourPointInfo(self._h, *p), "pbSimGetFourPointInfo"))

    def four_point(self):
        """The table as it stands (pbSimGetFourPoint): per member a list over lags (lag 0 first) of lists over the
        vectors (list order) of dicts of Python ints: lag, nx, ny, origins, sum_steps, samples, overlap, overlap2, re,
        im (units of 2^-30), power (units of 2^-60).  four_point_summary() turns a lag's rows into chi_4 and S_4."""
        info = self.four_point_info()
        lags, nvec = info["lags"], info["nvec"]
        rows = (_capi.pbFourPointRow * max(self.nsims * lags * nvec, 1))()
        _capi.check(_capi.lib().pbSimGetFourPoint(self._h, rows), "pbSimGetFourPoint")
        return _analysis.lag_table(self.nsims, lags, lambda g: _capi.four_point_row(rows[g]), nvec)

    def four_point_times(self):
        """(records taken so far, device milliseconds of the last record's launches)."""
        return self._span("pbSimGetFourPointTimes")

    def set_bond_dynamics(self, interval, lags, link_gap, max_radius, overlap_radius):
        """Keep a device ring of `lags` records of every bot's quantised position and of the list of its up to 8
        neighbours under the cluster analysis' link rule at `link_gap`, among the bots whose radius is at most
        `max_radius`; one record is taken in front of every step whose start time passes the schedule's gate at
        `interval` (0: every step, -1: only by bond_dynamics_record()) while step() runs.  Per pair of a record with one
        of the `lags` latest ones the surviving links and, per bot, the displacement relative to the neighbours it had
        are summed over the origins as exact integers (pbSimSetBondDynamics); a caged bot overlaps if that displacement
        is shorter than `overlap_radius`, in [0, 256).  Restarts at record 0; lags 0 switches it off.  Recording changes
        no state bit."""
        _capi.check(_capi.lib().pbSimSetBondDynamics(self._h, float(interval), int(lags), float(link_gap),
                                                     float(max_radius), float(overlap_radius)), "pbSimSetBondDynamics")

    def bond_dynamics_record(self):
        """One record now, of the state as it is (pbSimBondDynamicsRecord)."""
        _capi.check(_capi.lib().pbSimBondDynamicsRecord(self._h), "pbSimBondDynamicsRecord")

    def bond_dynamics_info(self):
        """A dict of interval, lags (0: off), link_gap, max_radius, overlap_radius and records taken so far
        (pbSimGetBondDynamicsInfo)."""
        return _analysis.read_info(_analysis.BOND_DYNAMICS_INFO, lambda *p: _capi.check(
            _capi.lib().pbSimGetBondDynamicsInfo(self._h, *p), "pbSimGetBondDynamicsInfo"))

    def bond_dynamics(self):
        """The table as it stands (pbSimGetBondDynamics): per member a list over lags (lag 0 first) of dicts of Python
        ints: lag, origins, sum_steps, samples, crowded, bonds_then, bonds_now, bonds_kept, bots_unchanged, bots_lost,
        bots_gained, plain_q2, and the lists over k = 1 ... 8 cage_samples, cage_overlap and cage_q2 (units of 2^-40,
        k^2 times the cage-relative sum).  bond_dynamics_summary() turns a row into the quotients."""
        lags = self.bond_dynamics_info()["lags"]
        rows = (_capi.pbBondRow * max(self.nsims * lags, 1))()
        _capi.check(_capi.lib().pbSimGetBondDynamics(self._h, rows), "pbSimGetBondDynamics")
        return _analysis.lag_table(self.nsims, lags, lambda g: _capi.bond_row(rows[g]))

    def bond_dynamics_times(self):
        """(records taken so far, device milliseconds of the last record's launches)."""
        return self._span("pbSimGetBondDynamicsTimes")


class Ensemble(Sim):
    """A batch of independent simulations of equal size stepped by the same launches
    (pbSimCreateBatch): seeds of a Monte-Carlo run, points of a parameter sweep."""

    def __init__(self, params_list, wall_half=0.0, keepalive=None):
        self._keep = keepalive
        self.nsims = len(params_list)
        arr = (SimParams * self.nsims)(*params_list)
        self.params = params_list[0]
        self.n = int(params_list[0].nCells)
        h = C.c_void_p()
        _capi.check(_capi.lib().pbSimCreateBatch(C.byref(h), arr, self.nsims, float(wall_half)), "pbSimCreateBatch")
        self._h = h

    def centroids(self):
        out = np.empty((self.nsims, 2), np.float64)
        _capi.check(_capi.lib().pbSimCentroids(self._h, out.ctypes.data_as(C.POINTER(C.c_double))), "pbSimCentroids")
        return out

    def centroid_sums(self):
        """The reference's own fp32 centroid sums per member (bots added serially in order, particlebot.cpp:335-338):
        what its CSV's centroid columns are divided from, bit for bit."""
        out = np.empty((self.nsims, 2), np.float32)
        _capi.check(_capi.lib().pbSimCentroidSums(self._h, out.ctypes.data_as(C.POINTER(C.c_float))), "pbSimCentroidSums")
        return out
