"""What Sim (over pbSim*) and HostSim (over pbHost*) both know about the analyses, stated once: the fields of each
recorder's info call, the per-bot buffers, the two-pass contact export, the buffers of a field map and of a structure
factor, and the nesting of a lag table.  Plain data and plain functions; each class passes its own way of making the C
call, a callable that takes the trailing arguments and raises when the call is refused."""
import ctypes as C

import numpy as np

from . import _capi

# the values an info call fills, in the C call's order: (name, ctype)
SERIES_INFO = (("interval", C.c_float), ("capacity", C.c_uint), ("records", C.c_ulonglong))
TIME_CORRELATION_INFO = (("interval", C.c_float), ("lags", C.c_uint), ("overlap_radius", C.c_float),
                         ("records", C.c_ulonglong))
SCATTERING_INFO = (("interval", C.c_float), ("lags", C.c_uint), ("box_log2", C.c_int), ("nvec", C.c_uint),
                   ("records", C.c_ulonglong))
VAN_HOVE_INFO = (("interval", C.c_float), ("lags", C.c_uint), ("width", C.c_float), ("bins", C.c_uint),
                 ("records", C.c_ulonglong))
VAN_HOVE_DISTINCT_INFO = VAN_HOVE_INFO
COHERENT_INFO = SCATTERING_INFO
FOUR_POINT_INFO = (("interval", C.c_float), ("lags", C.c_uint), ("overlap_radius", C.c_float), ("box_log2", C.c_int),
                   ("nvec", C.c_uint), ("records", C.c_ulonglong))
BOND_DYNAMICS_INFO = (("interval", C.c_float), ("lags", C.c_uint), ("link_gap", C.c_float), ("max_radius", C.c_float),
                      ("overlap_radius", C.c_float), ("records", C.c_ulonglong))


def read_info(spec, call):
    """The dict of an info call: call(*pointers) fills one C value per entry of `spec`; floats for c_float, else ints."""
    vals = [ctype() for _, ctype in spec]
    call(*[C.byref(v) for v in vals])
    return {name: (float if ctype is C.c_float else int)(v.value) for (name, ctype), v in zip(spec, vals)}


# the arrays a per-bot call fills, in the C call's order: (name, dtype, shape after the bot index)
CLUSTER_LABELS = (("labels", np.uint32, ()), ("degree", np.uint32, ()))
HEXATIC = (("psi6", np.complex128, ()), ("neighbours", np.uint32, ()))
REARRANGEMENT_OF = (("disp", np.float32, (2,)), ("marked", np.uint32, ()), ("now", np.uint32, ()),
                    ("kept", np.uint32, ()))
STRAIN_OF = (("moments", np.int64, (len(_capi.PB_STRAIN_MOMENTS),)), ("gradient", np.float64, (2, 2)),
             ("d2min", np.float64, ()))


def per_bot(spec, n, call):
    """The dict name -> array (n, ...) of a per-bot call: call(*pointers) fills one array per entry of `spec`."""
    out = {name: np.empty((n,) + tail, dtype) for name, dtype, tail in spec}
    call(*[_capi.np_ptr(a) for a in out.values()])
    return out


def contacts(n, call):
    """The contact export in its two passes: call(offsets, links, capacity, count) first without buffers, which counts
    the links, then with n + 1 offsets and room for that many; the links' columns taken apart."""
    count = C.c_ulonglong(0)
    call(None, None, 0, C.byref(count))
    offsets = np.empty(n + 1, np.uint32)
    links = np.empty(int(count.value), _capi.CONTACT_LINK_DTYPE)
    call(_capi.np_ptr(offsets), _capi.np_ptr(links), links.size, C.byref(count))
    return {"offsets": offsets, "other": links["other"].copy(), "gap": links["gap"].copy(),
            "force": np.stack([links["fx"], links["fy"]], axis=1)}


def field_cells(nsims, nx, ny):
    """Zeroed cells (nsims, ny, nx) for a field map; (nsims, 1, 1) where the engine will refuse the view (a call that is
    refused gets no buffer to speak of)."""
    fits = 1 <= int(nx) <= 1024 and 1 <= int(ny) <= 1024 and nsims * int(nx) * int(ny) * 64 <= 1 << 31
    return np.zeros((nsims,) + ((int(ny), int(nx)) if fits else (1, 1)), _capi.FIELD_CELL_DTYPE)


def held_vectors(vectors):
    """(array to pass, nvec) of a wavevector list: an empty list still has an address, and the engine refuses it."""
    vec = _capi.sk_vectors(vectors)
    return (vec if vec.shape[0] else np.zeros((1, 2), np.int32)), vec.shape[0]


def structure_factor_rows(nsims, nvec):
    """Zeroed rows (nsims, nvec) for a structure factor; (nsims, 1) where the engine will refuse the list."""
    fits = 1 <= nvec <= _capi.SK_MAX_VECTORS and nsims * nvec * 80 <= 1 << 31
    return np.zeros((nsims, nvec if fits else 1), _capi.SK_ROW_DTYPE)


def lag_table(nsims, lags, row, nvec=None):
    """A lag recorder's flat table as nested lists: [member][lag] of row(g), or [member][lag][vector] with nvec; g is the
    flat index, members outermost."""
    if nvec is None:
        return [[row(m * lags + l) for l in range(lags)] for m in range(nsims)]
    return [[[row((m * lags + l) * nvec + k) for k in range(nvec)] for l in range(lags)] for m in range(nsims)]


def van_hove_lists(rows, counts, nsims, lags, bins):
    """The rows and counters of pbSimGetVanHove as van_hove() returns them: per member a list over lags of dicts, each
    van_hove_row() plus radial (bins ints), x and y (2 bins ints each)."""
    def row(g):
        c = [int(v) for v in counts[g * 5 * bins:(g + 1) * 5 * bins]]
        d = _capi.van_hove_row(rows[g])
        d["radial"], d["x"], d["y"] = c[:bins], c[bins:3 * bins], c[3 * bins:]
        return d
    return lag_table(nsims, lags, row)


def van_hove_distinct_lists(rows, counts, nsims, lags, bins):
    """The rows and counters of pbSimGetVanHoveDistinct as van_hove_distinct() returns them: per member a list over lags
    of dicts, each row_dict() plus counts (bins ints)."""
    def row(g):
        d = _capi.row_dict(rows[g])
        d["counts"] = [int(v) for v in counts[g * bins:(g + 1) * bins]]
        return d
    return lag_table(nsims, lags, row)
