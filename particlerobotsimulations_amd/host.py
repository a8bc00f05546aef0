"""ctypes binding of libparticlebot_host.so: the C++ host side (class Particlebot, the .cfg loader)
behind a handful of C wrappers (csrc/pb_capi.cpp)."""
import ctypes as C
import os
from functools import partial

import numpy as np

from . import _analysis, _capi

PB_MAX_OBSTACLES = 10


class FlatConfig(C.Structure):
    """pbFlatConfig in csrc/pb_capi.cpp: a resolved configuration without pointers."""
    _fields_ = [
        ("gridSizeX", C.c_uint32), ("gridSizeY", C.c_uint32), ("numCells", C.c_uint32),
        ("worldOriginX", C.c_float), ("worldOriginY", C.c_float),
        ("cellSizeX", C.c_float), ("cellSizeY", C.c_float),
        ("nCells", C.c_uint32), ("nDead", C.c_int32),
        ("gravity", C.c_float), ("spring", C.c_float), ("damping", C.c_float), ("shear", C.c_float),
        ("attraction", C.c_float), ("boundaryDamping", C.c_float), ("friction", C.c_float),
        ("massFactor", C.c_float), ("frictionFactor", C.c_float), ("radFactor", C.c_float),
        ("attractionFactor", C.c_float),
        ("constraint", C.c_float), ("constraint_contraction", C.c_float),
        ("centroid_steps", C.c_int32), ("centroid_int", C.c_float), ("centroid_radius", C.c_float),
        ("light_x", C.c_float), ("light_y", C.c_float), ("phase_update_interval", C.c_float),
        ("control", C.c_int32), ("config", C.c_int32),
        ("min_radius", C.c_float), ("max_radius", C.c_float), ("rise_period", C.c_float),
        ("freq", C.c_float),
        ("nobstacles", C.c_int32),
        ("x1obs", C.c_float * PB_MAX_OBSTACLES), ("x2obs", C.c_float * PB_MAX_OBSTACLES),
        ("y1obs", C.c_float * PB_MAX_OBSTACLES), ("y2obs", C.c_float * PB_MAX_OBSTACLES),
        ("n_cir_obstacles", C.c_int32),
        ("x_cir_obs", C.c_float * PB_MAX_OBSTACLES), ("y_cir_obs", C.c_float * PB_MAX_OBSTACLES),
        ("r_cir_obs", C.c_float * PB_MAX_OBSTACLES),
        ("Nx", C.c_int32), ("phase_std", C.c_float), ("seed", C.c_uint32),
        ("light_shadow", C.c_uint32), ("testing", C.c_uint32),
        ("constrained_contraction", C.c_uint32), ("display_shadow", C.c_uint32),
        ("time_to_dead", C.c_float), ("max_time", C.c_float),
        ("timestep", C.c_float), ("sort_interval", C.c_float), ("dump_interval", C.c_float),
        ("camera_x", C.c_float), ("camera_y", C.c_float), ("light_radius", C.c_float),
        ("display_interval", C.c_int32), ("video_interval", C.c_int32),
        ("csv_filename", C.c_char * 300), ("video_filename", C.c_char * 300),
        ("wallHalf", C.c_float), ("rngKind", C.c_int32), ("forceVariant", C.c_int32),
    ]


_lib = None
_ptr = _capi.np_ptr  # an array's address, for a void * argument
_P, _F, _I, _U, _S = C.c_void_p, C.c_float, C.c_int, C.c_uint, C.c_char_p
_ULL, _PULL = C.c_ulonglong, C.POINTER(C.c_ulonglong)
# every pbHost* function libparticlebot_host.so exports (csrc/pb_capi.cpp, csrc/pb_host_resources.cpp):
# name -> (restype, argtypes).  An analysis wrapper takes the handle first and returns 0 or -1.
SYMBOLS = {
    "pbHostLoadConfig": (_I, [_S, _S, C.POINTER(FlatConfig)]),
    "pbHostCreate": (_P, [_S, _S, _I]),
    "pbHostDestroy": (None, [_P]),
    "pbHostReset": (None, [_P]),
    "pbHostUpdate": (None, [_P]),
    "pbHostAdvance": (_I, [_P, _I]),
    "pbHostStepsUntilDump": (_I, [_P, _I]),
    "pbHostTime": (_F, [_P]),
    "pbHostSetTime": (None, [_P, _F]),
    "pbHostFinished": (_I, [_P]),
    "pbHostDump": (_I, [_P, _S, _S]),
    "pbHostLoadFromFile": (_I, [_P, _S]),
    "pbHostWriteFrame": (_I, [_P, _S, _I, _I, _F, _F, _F]),
    "pbHostWriteFrameStyle": (_I, [_P, _S, _I, _I, _F, _F, _F, _I]),
    "pbHostRenderFrame": (_I, [_P, _S, _P, _I, _I, _F, _F, _F, _I]),
    "pbHostRenderStats": (_I, [_P, _PULL, C.POINTER(_F)]),
    "pbHostClusterStats": (_I, [_P, _F, _P]),
    "pbHostClusterLabels": (_I, [_P, _F, _P, _P]),
    "pbHostContacts": (_I, [_P, _F, _P, _P, _ULL, _PULL]),
    "pbHostContactVirial": (_I, [_P, _F, _P]),
    "pbHostRadialCounts": (_I, [_P, _F, _U, _P]),
    "pbHostStructureStats": (_I, [_P, _F, _P]),
    "pbHostHexatic": (_I, [_P, _F, _P, _P]),
    "pbHostMarkReference": (_I, [_P, _F]),
    "pbHostRearrangementStats": (_I, [_P, _P]),
    "pbHostRearrangementOf": (_I, [_P, _P, _P, _P, _P]),
    "pbHostStrainStats": (_I, [_P, _F, _P]),
    "pbHostStrainOf": (_I, [_P, _P, _P, _P]),
    "pbHostMoments": (_I, [_P, _P]),
    "pbHostSetSeries": (_I, [_P, _F, _U]),
    "pbHostSeriesInfo": (_I, [_P, _P, _P, _P]),
    "pbHostSeriesRows": (_I, [_P, _ULL, _P, _ULL, _PULL]),
    "pbHostPairCorrelation": (_I, [_P, _I, _F, _U, _P, _P]),
    "pbHostSetTimeCorrelation": (_I, [_P, _F, _U, _F]),
    "pbHostTimeCorrelationRecord": (_I, [_P]),
    "pbHostTimeCorrelationInfo": (_I, [_P, _P, _P, _P, _P]),
    "pbHostTimeCorrelationRows": (_I, [_P, _P, _ULL, _PULL]),
    "pbHostSetScattering": (_I, [_P, _F, _U, _I, _P, _U]),
    "pbHostScatteringRecord": (_I, [_P]),
    "pbHostScatteringInfo": (_I, [_P, _P, _P, _P, _P, _P]),
    "pbHostScatteringRows": (_I, [_P, _P, _ULL, _PULL]),
    "pbHostSetVanHove": (_I, [_P, _F, _U, _F, _U]),
    "pbHostVanHoveRecord": (_I, [_P]),
    "pbHostVanHoveInfo": (_I, [_P, _P, _P, _P, _P, _P]),
    "pbHostVanHoveRows": (_I, [_P, _P, _P, _ULL, _PULL]),
    "pbHostSetVanHoveDistinct": (_I, [_P, _F, _U, _F, _U]),
    "pbHostVanHoveDistinctRecord": (_I, [_P]),
    "pbHostVanHoveDistinctInfo": (_I, [_P, _P, _P, _P, _P, _P]),
    "pbHostVanHoveDistinctRows": (_I, [_P, _P, _P, _ULL, _PULL]),
    "pbHostSetCoherent": (_I, [_P, _F, _U, _I, _P, _U]),
    "pbHostCoherentRecord": (_I, [_P]),
    "pbHostCoherentInfo": (_I, [_P, _P, _P, _P, _P, _P]),
    "pbHostCoherentRows": (_I, [_P, _P, _ULL, _PULL]),
    "pbHostSetFourPoint": (_I, [_P, _F, _U, _F, _I, _P, _U]),
    "pbHostFourPointRecord": (_I, [_P]),
    "pbHostFourPointInfo": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "pbHostFourPointRows": (_I, [_P, _P, _ULL, _PULL]),
    "pbHostSetBondDynamics": (_I, [_P, _F, _U, _F, _F, _F]),
    "pbHostBondDynamicsRecord": (_I, [_P]),
    "pbHostBondDynamicsInfo": (_I, [_P, _P, _P, _P, _P, _P, _P]),
    "pbHostBondDynamicsRows": (_I, [_P, _P, _ULL, _PULL]),
    "pbHostFieldMap": (_I, [_P, _P, _P, _P]),
    "pbHostStructureFactor": (_I, [_P, _I, _I, _P, _U, _P]),
    "pbHostSetDisplay": (None, [_P, _I]),
    "pbHostCentroidTrail": (_I, [_P, _P, _P, C.POINTER(_U)]),
    "pbHostSaveCheckpoint": (_I, [_P, _S]),
    "pbHostLoadCheckpoint": (_I, [_P, _S]),
    "pbHostDrawDead": (_I, [_P, _P]),
    "pbHostGetArray": (_I, [_P, _I, _P]),
    "pbHostSetArray": (_I, [_P, _I, _P, _I, _I]),
    "pbHostLibcRandDraws": (None, [_U, _I, _P]),
    "pbHostLibmCheck": (_I, [_I, _U, _PULL, _PULL, _PULL]),
    "pbHostLibcVersion": (_S, []),
    "pbHostXorwowOutputs": (None, [_I, _ULL, _U, _U, _P]),
    "pbHostXorwowNormals": (None, [_I, _U, _U, _U, _P]),
    "pbHostXorwowJumpMatrix": (None, [_U, _P]),
    "pbHostEngineHandle": (_P, [_P]),
    "pbHostNumBots": (_U, [_P]),
    "pbHostCentroidSteps": (_I, [_P]),
    "pbHostGetResources": (_I, [_P]),
    "pbHostParseCpuList": (_I, [_S, C.POINTER(_I), _I]),
}


def lib():
    """Load libparticlebot_host.so and bind every symbol of SYMBOLS.  Raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    _capi.lib()  # libparticlebot_hip.so first (RTLD_GLOBAL), the host library links against it
    if not os.path.exists(_capi.HOST_SO):
        raise RuntimeError(f"{_capi.HOST_SO} not found: run __graft_entry__.build()")
    L = C.CDLL(_capi.HOST_SO)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def libc_rand_draws(seed, n):
    """n outputs of the class's private glibc-compatible generator after seeding with `seed`."""
    out = np.empty(n, np.int32)
    lib().pbHostLibcRandDraws(int(seed), int(n), _ptr(out))
    return out


def _overrides(over):
    if not over:
        return None
    return "\n".join(f"{k}\n{v}" for k, v in over.items()).encode()


def load_config(cfg_path=None, **over):
    """Resolve a .cfg exactly as the runner does; returns a FlatConfig."""
    out = FlatConfig()
    rc = lib().pbHostLoadConfig(os.fsencode(cfg_path) if cfg_path else None, _overrides(over), C.byref(out))
    if rc != 0:
        raise FileNotFoundError(cfg_path)
    return out


class HostSim:
    """class Particlebot driven from Python (engine: 'fused' or 'legacy')."""

    def __init__(self, cfg_path=None, engine="fused", reset=True, **over):
        self._h = lib().pbHostCreate(os.fsencode(cfg_path) if cfg_path else None, _overrides(over),
                                     {"fused": 0, "legacy": 1, "host": 2}[engine])
        if not self._h:
            raise FileNotFoundError(cfg_path)
        self.n = lib().pbHostNumBots(self._h)
        if reset:
            lib().pbHostReset(self._h)

    def close(self):
        if getattr(self, "_h", None):
            lib().pbHostDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, symbol, refused, *args):
        """One wrapper call on this handle; a non-zero return raises RuntimeError(refused)."""
        if getattr(lib(), symbol)(self._h, *args) != 0:
            raise RuntimeError(refused)

    def update(self):
        lib().pbHostUpdate(self._h)

    def advance(self, nsteps):
        return lib().pbHostAdvance(self._h, int(nsteps))

    def steps_until_dump(self, max_steps=1 << 20):
        return lib().pbHostStepsUntilDump(self._h, int(max_steps))

    @property
    def time(self):
        return lib().pbHostTime(self._h)

    @time.setter
    def time(self, t):
        """Particlebot::setTime: moves the clock, of the class and of its engine; nothing else changes."""
        lib().pbHostSetTime(self._h, float(t))

    @property
    def finished(self):
        return bool(lib().pbHostFinished(self._h))

    def dump(self, path, mode="a"):
        if lib().pbHostDump(self._h, os.fsencode(path), mode.encode()) != 0:
            raise OSError(path)

    def load_from_file(self, path):
        if lib().pbHostLoadFromFile(self._h, os.fsencode(path)) != 0:
            raise OSError(path)

    def draw_dead(self):
        out = np.empty(self.n, np.int32)
        lib().pbHostDrawDead(self._h, _ptr(out))
        return out

    def reset(self):
        lib().pbHostReset(self._h)

    def set_display(self, on):
        """Particlebot::setDisplay: the reference's colour buffer and centroid trail (create with reset=False, call
        this, then reset())."""
        lib().pbHostSetDisplay(self._h, 1 if on else 0)

    def centroid_trail(self):
        """(xy, times, records): the centroid ring ((centroid_steps, 2) float32, y still + 2000), the start time of the
        step that wrote each slot (NaN: never) and the records made so far.  Needs set_display(True)."""
        steps = max(0, lib().pbHostCentroidSteps(self._h))
        xy = np.empty((steps, 2), np.float32)
        times = np.empty(steps, np.float32)
        rec = C.c_uint(0)
        self._call("pbHostCentroidTrail", "centroid_trail: set_display(True) first", _ptr(xy), _ptr(times), C.byref(rec))
        return xy, times, int(rec.value)

    def write_frame(self, path, size=800, center=(0.0, 0.0), half_extent=0.0, style="plain", renderer="host"):
        """Binary PPM of the arena seen from above (Particlebot::writeFramePPM; style "reference":
        writeFramePPMReference, the device colours and the centroid trail).  half_extent <= 0:
        the reference's camera, centred on (camera_x, 0), half extent camera_y * tan(30 deg).
        size: pixels of a square frame, or (width, height).  renderer "device": the same bytes rasterised on the GPU
        from the resident state (Particlebot::writeFramePPMDevice; fused engine only)."""
        L = lib()
        width, height = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        if style not in ("plain", "reference"):
            raise ValueError(style)
        if renderer not in ("host", "device"):
            raise ValueError(renderer)
        if renderer == "device":
            if L.pbHostRenderFrame(self._h, os.fsencode(path), None, width, height, center[0], center[1], half_extent,
                                   1 if style == "reference" else 0) != 0:
                raise OSError(f"writeFramePPMDevice({path}) failed")
            return
        if style != "plain":
            if L.pbHostWriteFrameStyle(self._h, os.fsencode(path), width, height, center[0], center[1],
                                       half_extent, 1) != 0:
                raise OSError(f"writeFramePPMReference({path}) failed")
            return
        if L.pbHostWriteFrame(self._h, os.fsencode(path), width, height, center[0], center[1],
                              half_extent) != 0:
            raise OSError(f"writeFramePPM({path}) failed")

    def render(self, width, height, center=(0.0, 0.0), half_extent=0.0, style="plain"):
        """The frame write_frame(..., renderer="device") writes, as a uint8 array [height, width, 3] (fused engine
        only; Particlebot::renderFrame)."""
        if style not in ("plain", "reference"):
            raise ValueError(style)
        out = np.empty((int(height), int(width), 3), np.uint8)
        self._call("pbHostRenderFrame",
                   "renderFrame failed (the device rasteriser needs the fused engine and a valid view)", None, _ptr(out),
                   int(width), int(height), center[0], center[1], half_extent, 1 if style == "reference" else 0)
        return out

    def render_stats(self):
        """(frames rendered on the device, device milliseconds of the last frame's launches)."""
        n, ms = C.c_ulonglong(0), C.c_float(0.0)
        self._call("pbHostRenderStats", "render_stats: the device rasteriser needs the fused engine", C.byref(n),
                   C.byref(ms))
        return int(n.value), float(ms.value)

    def clusters(self, gap=0.0):
        """Cluster analysis of the state as it is now, on the device (pbSimClusterStats; fused engine only): a dict with
        clusters, largest, largest_label, isolated, links, max_degree and rounds.  Bots are linked when
        dist - (ri + rj) < gap in fp32; a label is the smallest original index of a component."""
        row = _capi.pbClusterStats()
        self._call("pbHostClusterStats", "clusters: the cluster analysis needs the fused engine and a finite gap >= 0",
                   float(gap), C.byref(row))
        return _capi.row_dict(row)

    def cluster_labels(self, gap=0.0):
        """(labels, degree): two uint32 arrays in original bot order (pbSimClusterLabelsOf; fused engine only)."""
        out = _analysis.per_bot(_analysis.CLUSTER_LABELS, self.n, partial(
            self._call, "pbHostClusterLabels",
            "cluster_labels: the cluster analysis needs the fused engine and a finite gap >= 0", float(gap)))
        return out["labels"], out["degree"]

    def contacts(self, gap=0.0):
        """The contact network of the state as it is now, from the device (pbSimContactsOf; fused engine only): a dict
        with offsets (uint32, n + 1: CSR in original bot order, ascending `other`), other (uint32, E), gap (float32, E)
        and force (float32, E x 2: the pair law's force on the owning bot from other)."""
        return _analysis.contacts(self.n, partial(
            self._call, "pbHostContacts", "contacts: the contact export needs the fused engine and a finite gap >= 0",
            float(gap)))

    def contact_virial(self, gap=0.0):
        """Per-bot virial of the contact network (pbSimContactVirialOf; fused engine only): float64, n x 4, the columns
        sxx, sxy, syx, syy summed over each bot's entries in CSR order."""
        out = np.empty((self.n, 4), np.float64)
        self._call("pbHostContactVirial",
                   "contact_virial: the contact export needs the fused engine and a finite gap >= 0", float(gap),
                   _ptr(out))
        return out

    def radial_counts(self, r_max, bins, member=None):
        """Radial pair counts of the state as it is now, on the device (pbSimRadialCounts; fused engine only): uint64,
        (1, bins), or (bins,) with member=0.  Ordered pairs, bin int(dist * (float32(bins) / r_max)) in fp32."""
        out = np.zeros((1, int(bins)), np.uint64)
        self._call("pbHostRadialCounts", "radial_counts: the structure analysis needs the fused engine, a finite r_max "
                   "> 0 and 1 ... 4096 bins", float(r_max), int(bins), _ptr(out))
        return out if member is None else out[int(member)]

    def structure(self, gap=0.0):
        """Hexatic order of the state as it is now, on the device (pbSimStructureStats; fused engine only): a list with
        one dict: bonds, psi6_re, psi6_im, coordination and psi6, the complex mean over the directed bonds."""
        row = _capi.pbStructureStats()
        self._call("pbHostStructureStats",
                   "structure: the structure analysis needs the fused engine and a finite gap >= 0", float(gap),
                   C.byref(row))
        return [_capi.structure_row(row)]

    def hexatic(self, gap=0.0, member=0):
        """(psi6, neighbours): complex128[n] and uint32[n] in original bot order (pbSimHexaticOf; fused engine only)."""
        if int(member) != 0:
            raise IndexError(member)
        out = _analysis.per_bot(_analysis.HEXATIC, self.n, partial(
            self._call, "pbHostHexatic", "hexatic: the structure analysis needs the fused engine and a finite gap >= 0",
            float(gap)))
        return out["psi6"], out["neighbours"]

    def mark_reference(self, gap=0.0):
        """Keep the positions and the link network at `gap` on the device as the reference of rearrangement()
        (pbSimMarkReference; fused engine only).  A new mark replaces the old one."""
        self._call("pbHostMarkReference",
                   "mark_reference: the rearrangement analysis needs the fused engine and a finite gap >= 0", float(gap))

    def rearrangement(self):
        """The state as it is now against the mark, on the device (pbSimRearrangementStats; fused engine only): a list
        with one dict: bonds_marked / bonds_now / bonds_kept (directed), bots_unchanged / bots_lost / bots_gained,
        measured, sum_qx / sum_qy (units of 2^-20), sum_q2 (a Python int, units of 2^-40) and max_q2."""
        row = _capi.pbRearrangementStats()
        self._call("pbHostRearrangementStats",
                   "rearrangement: the rearrangement analysis needs the fused engine and a marked reference",
                   C.byref(row))
        return [_capi.rearrangement_row(row)]

    def rearrangement_of(self, member=0):
        """Per bot, original order (pbSimRearrangementOf; fused engine only): a dict of disp (float32, n x 2: dx, dy since
        the mark) and marked, now, kept (uint32: bonds at the mark, now, and in both)."""
        if int(member) != 0:
            raise IndexError(member)
        return _analysis.per_bot(_analysis.REARRANGEMENT_OF, self.n, partial(
            self._call, "pbHostRearrangementOf",
            "rearrangement_of: the rearrangement analysis needs the fused engine and a marked reference"))

    def strain(self, threshold=0.0):
        """Local strain and D2min against the mark, on the device (pbSimStrainStats; fused engine only): a list with one
        dict of Python ints: fitted / unfitted / above (fitted bots with D2min > threshold), bonds_used / bonds_dropped,
        the sums yxx ... w of the moments, sum_d2 and max_d2 (units of 2^-40)."""
        row = _capi.pbStrainStats()
        self._call("pbHostStrainStats", "strain: the strain analysis needs the fused engine, a marked reference and a "
                   "finite threshold >= 0", float(threshold), C.byref(row))
        return [_capi.row_dict(row)]

    def strain_of(self, member=0):
        """Per bot, original order (pbSimStrainOf; fused engine only): a dict of moments (int64, n x 9), gradient
        (float64, n x 2 x 2: the local deformation gradient J) and d2min (float64, units of 2^-40)."""
        if int(member) != 0:
            raise IndexError(member)
        return _analysis.per_bot(_analysis.STRAIN_OF, self.n, partial(
            self._call, "pbHostStrainOf", "strain_of: the strain analysis needs the fused engine and a marked reference"))

    def moments(self):
        """The row of integer moments of the state as it is now, on the device (pbSimMoments; fused engine only): a list
        with one dict of Python ints, the 128-bit sums xx, yy, xy, rr, vv composed."""
        row = _capi.pbMomentsRow()
        self._call("pbHostMoments", "moments: the time series needs the fused engine", C.byref(row))
        return [_capi.row_dict(row)]

    def set_series(self, interval, capacity):
        """Record such a row into a device ring of `capacity` rows in front of every step whose start time passes the
        schedule's gate at `interval` (0: every step) while the simulation advances (pbSimSetSeries; fused engine only).
        Restarts at record 0; capacity 0 switches the series off."""
        self._call("pbHostSetSeries", "set_series: the time series needs the fused engine, a finite interval >= 0 and a "
                   "ring of at most 2^31 bytes", float(interval), int(capacity))

    def series_info(self):
        """A dict of interval, capacity (0: off) and records taken so far (pbSimGetSeriesInfo; fused engine only)."""
        return _analysis.read_info(_analysis.SERIES_INFO, partial(
            self._call, "pbHostSeriesInfo", "series_info: the time series needs the fused engine"))

    def series_rows(self, first=0):
        """The records from number `first` up to the last one taken, in order, as moments() gives rows
        (Particlebot::seriesRows; fused engine only)."""
        info = self.series_info()
        cap = max(info["records"] - int(first), 1)
        rows, count = (_capi.pbMomentsRow * cap)(), C.c_ulonglong(0)
        self._call("pbHostSeriesRows", "series_rows: the time series needs the fused engine, the series on and records "
                   "that the ring still holds", int(first), rows, cap, C.byref(count))
        return [_capi.row_dict(r) for r in rows[:int(count.value)]]

    def pair_correlation(self, kind, r_max, bins, member=None):
        """Pair correlations of the state as it is now, on the device (pbSimPairCorrelation; fused engine only): (rows,
        totals) as Sim.pair_correlation gives them, rows shaped (1, bins), or (bins,) with a single totals dict for
        member=0."""
        rows = np.zeros((1, max(int(bins), 1)), _capi.CORRELATION_BIN_DTYPE)
        tot = _capi.pbCorrelationTotals()
        self._call("pbHostPairCorrelation", "pair_correlation: the correlation analysis needs the fused engine, a known "
                   "kind, a finite r_max > 0 and 1 ... 1024 bins", _capi.correlation_kind(kind), float(r_max), int(bins),
                   _ptr(rows), C.byref(tot))
        totals = [_capi.row_dict(tot)]
        return (rows, totals) if member is None else (rows[int(member)], totals[int(member)])

    def set_time_correlation(self, interval, lags, overlap_radius):
        """Keep a device ring of `lags` snapshots, one taken in front of every step whose start time passes the
        schedule's gate at `interval` (0: every step, -1: only by time_correlation_record()) while the simulation
        advances, and sum MSD, VACF and the overlap count per lag over all time origins (pbSimSetTimeCorrelation; fused
        engine only).  Restarts at record 0; lags 0 switches it off."""
        self._call("pbHostSetTimeCorrelation", "set_time_correlation: the time correlation needs the fused engine, a "
                   "finite interval >= 0 (or -1), at most 64 lags and an overlap radius in [0, 2048)", float(interval),
                   int(lags), float(overlap_radius))

    def time_correlation_record(self):
        """One record now, of the state as it is (pbSimTimeCorrelationRecord; fused engine only)."""
        self._call("pbHostTimeCorrelationRecord", "time_correlation_record: the time correlation needs the fused engine "
                   "and the correlation on")

    def time_correlation_info(self):
        """A dict of interval, lags (0: off), overlap_radius and records taken so far (pbSimGetTimeCorrelationInfo;
        fused engine only)."""
        return _analysis.read_info(_analysis.TIME_CORRELATION_INFO, partial(
            self._call, "pbHostTimeCorrelationInfo",
            "time_correlation_info: the time correlation needs the fused engine"))

    def time_correlation(self):
        """The table as it stands, as Sim.time_correlation gives it: a list with one list of `lags` dicts of Python
        ints, lag 0 first (Particlebot::timeCorrelationRows; fused engine only)."""
        lags = self.time_correlation_info()["lags"]
        cap = max(lags, 1)
        rows, count = (_capi.pbTimeCorrelationRow * cap)(), C.c_ulonglong(0)
        self._call("pbHostTimeCorrelationRows", "time_correlation: the time correlation needs the fused engine, the "
                   "correlation on and fewer than 2^31 samples per lag", rows, cap, C.byref(count))
        return _analysis.lag_table(1, lags, lambda g: _capi.row_dict(rows[g]))

    def set_scattering(self, interval, lags, box_log2, vectors):
        """Keep a device ring of `lags` snapshots of the quantised positions, taken as the time correlation takes its
        own, and sum the integer phasors of every bot's displacement per lag and wavevector
        (2 pi / 2^box_log2)(nx, ny) of `vectors` over all time origins (pbSimSetScattering; fused engine only).
        Restarts at record 0; lags 0 switches it off."""
        held, nvec = _analysis.held_vectors(vectors if vectors is not None else np.zeros((0, 2), np.int32))
        self._call("pbHostSetScattering", "set_scattering: the scattering needs the fused engine, a finite interval >= 0 "
                   "(or -1), at most 64 lags, box_log2 in -8 ... 12 and 1 ... 256 vectors", float(interval), int(lags),
                   int(box_log2), _ptr(held), nvec)

    def scattering_record(self):
        """One record now, of the state as it is (pbSimScatteringRecord; fused engine only)."""
        self._call("pbHostScatteringRecord",
                   "scattering_record: the scattering needs the fused engine and the scattering on")

    def scattering_info(self):
        """A dict of interval, lags (0: off), box_log2, nvec and records taken so far (pbSimGetScatteringInfo; fused
        engine only)."""
        return _analysis.read_info(_analysis.SCATTERING_INFO, partial(
            self._call, "pbHostScatteringInfo", "scattering_info: the scattering needs the fused engine"))

    def scattering(self):
        """The table as it stands, as Sim.scattering gives it: a list with one list over lags of lists over the vectors
        of dicts of Python ints (Particlebot::scatteringRows; fused engine only)."""
        info = self.scattering_info()
        lags, nvec = info["lags"], info["nvec"]
        cap = max(lags * nvec, 1)
        rows, count = (_capi.pbScatteringRow * cap)(), C.c_ulonglong(0)
        self._call("pbHostScatteringRows", "scattering: the scattering needs the fused engine, the scattering on and "
                   "fewer than 2^31 samples per lag", rows, cap, C.byref(count))
        return _analysis.lag_table(1, lags, lambda g: _capi.row_dict(rows[g]), nvec)

    def set_van_hove(self, interval, lags, width, bins):
        """Keep a device ring of `lags` position snapshots, one per step whose start passes the schedule's gate at
        `interval` (0: every step, -1: only by van_hove_record()), and add every record against the `lags` latest ones
        into exact integer histograms of the displacement per lag: `bins` radial bins of `width` and 2 bins of each
        component (pbSimSetVanHove; fused engine only).  Restarts at record 0; lags 0 switches it off."""
        self._call("pbHostSetVanHove", "set_van_hove: the van Hove function needs the fused engine, a finite interval "
                   ">= 0 (or -1), lags <= 64, a width in (0, 2048) and 1 ... 1024 bins", float(interval), int(lags),
                   float(width), int(bins))

    def van_hove_record(self):
        """One record now, of the state as it is (pbSimVanHoveRecord; fused engine only)."""
        self._call("pbHostVanHoveRecord",
                   "van_hove_record: the van Hove function needs the fused engine and the analysis on")

    def van_hove_info(self):
        """A dict of interval, lags (0: off), width, bins and records taken so far (pbSimGetVanHoveInfo; fused engine
        only)."""
        return _analysis.read_info(_analysis.VAN_HOVE_INFO, partial(
            self._call, "pbHostVanHoveInfo", "van_hove_info: the van Hove function needs the fused engine"))

    def van_hove(self):
        """The table as it stands, as Sim.van_hove gives it: a list with one list over lags of dicts of Python ints, the
        histograms radial, x and y as lists (Particlebot::vanHoveRows; fused engine only)."""
        info = self.van_hove_info()
        lags, bins = info["lags"], info["bins"]
        cap = max(lags, 1)
        rows, counts = (_capi.pbVanHoveRow * cap)(), (C.c_ulonglong * max(cap * 5 * bins, 1))()
        count = C.c_ulonglong(0)
        self._call("pbHostVanHoveRows", "van_hove: the van Hove function needs the fused engine, the analysis on and "
                   "fewer than 2^31 samples per lag", rows, counts, cap, C.byref(count))
        return _analysis.van_hove_lists(rows, counts, 1, lags, bins)

    def set_van_hove_distinct(self, interval, lags, width, bins):
        """Keep a device ring of `lags` position snapshots, taken as set_van_hove() takes them, and add every record
        against the `lags` latest ones into exact integer counts per lag of the ordered pairs (a bot then, another bot
        now) by distance: `bins` bins of `width` (pbSimSetVanHoveDistinct; fused engine only).  Restarts at record 0;
        lags 0 switches it off."""
        self._call("pbHostSetVanHoveDistinct", "set_van_hove_distinct: the distinct van Hove function needs the fused "
                   "engine, a finite interval >= 0 (or -1), lags <= 64, 1 ... 1024 bins and a width with bins * width < "
                   "2048", float(interval), int(lags), float(width), int(bins))

    def van_hove_distinct_record(self):
        """One record now, of the state as it is (pbSimVanHoveDistinctRecord; fused engine only)."""
        self._call("pbHostVanHoveDistinctRecord", "van_hove_distinct_record: the distinct van Hove function needs the "
                   "fused engine and the analysis on")

    def van_hove_distinct_info(self):
        """A dict of interval, lags (0: off), width, bins and records taken so far (pbSimGetVanHoveDistinctInfo; fused
        engine only)."""
        return _analysis.read_info(_analysis.VAN_HOVE_DISTINCT_INFO, partial(
            self._call, "pbHostVanHoveDistinctInfo",
            "van_hove_distinct_info: the distinct van Hove function needs the fused engine"))

    def van_hove_distinct(self):
        """The table as it stands, as Sim.van_hove_distinct gives it: a list with one list over lags of dicts of Python
        ints with `counts` as a list (Particlebot::vanHoveDistinctRows; fused engine only)."""
        info = self.van_hove_distinct_info()
        lags, bins = info["lags"], info["bins"]
        cap = max(lags, 1)
        rows, counts = (_capi.pbVanHoveDistinctRow * cap)(), (C.c_ulonglong * max(cap * bins, 1))()
        count = C.c_ulonglong(0)
        self._call("pbHostVanHoveDistinctRows", "van_hove_distinct: the distinct van Hove function needs the fused "
                   "engine, the analysis on and fewer than 2^31 centres per lag", rows, counts, cap, C.byref(count))
        return _analysis.van_hove_distinct_lists(rows, counts, 1, lags, bins)

    def field_map(self, nx, ny, center, half, member=None):
        """A field map of the state as it is now, on the device (pbSimFieldMap; fused engine only): (cells, totals) as
        Sim.field_map gives them, cells shaped (1, ny, nx), or (ny, nx) with a single totals dict for member=0."""
        view = _capi.field_view(nx, ny, center, half)
        cells, tot = _analysis.field_cells(1, nx, ny), _capi.pbFieldTotals()
        self._call("pbHostFieldMap", "field_map: the field map needs the fused engine, 1 ... 1024 cells per axis and "
                   "finite half extents > 0", C.byref(view), _ptr(cells), C.byref(tot))
        totals = [_capi.row_dict(tot)]
        return (cells, totals) if member is None else (cells[int(member)], totals[int(member)])

    def structure_factor(self, vectors, box_log2, kind="density", member=None):
        """The structure factor of the state as it is now, on the device (pbSimStructureFactor; fused engine only): the
        rows as Sim.structure_factor gives them, shaped (1, nvec), or (nvec,) for member=0."""
        (held, nvec), code = _analysis.held_vectors(vectors), _capi.sk_kind(kind)
        rows = _analysis.structure_factor_rows(1, nvec)
        self._call("pbHostStructureFactor", "structure_factor: the structure factor needs the fused engine, a known "
                   "kind, box_log2 in -8 ... 12 and 1 ... 4096 vectors", code, int(box_log2), _ptr(held), nvec, _ptr(rows))
        return rows if member is None else rows[int(member)]

    def save_checkpoint(self, path):
        rc = lib().pbHostSaveCheckpoint(self._h, os.fsencode(path))
        if rc != 0:
            raise OSError(f"saveCheckpoint({path}) failed ({rc})")

    def load_checkpoint(self, path):
        rc = lib().pbHostLoadCheckpoint(self._h, os.fsencode(path))
        if rc != 0:
            raise OSError(f"loadCheckpoint({path}) failed ({rc})")

    def get(self, name):
        which, dt, w = {"pos": (0, np.float32, 2), "vel": (1, np.float32, 2), "rad": (2, np.float32, 1),
                        "phase": (3, np.float32, 1), "dead": (5, np.int32, 1), "col": (6, np.float32, 4)}[name]
        out = np.empty((self.n, w) if w > 1 else self.n, dtype=dt)
        assert lib().pbHostGetArray(self._h, which, _ptr(out)) == 0
        return out

    def set(self, name, data, start=0):
        which = {"pos": 0, "vel": 1, "rad": 2, "phase": 3}[name]
        data = np.ascontiguousarray(data, np.float32)
        count = data.shape[0]
        assert lib().pbHostSetArray(self._h, which, _ptr(data), int(start), int(count)) == 0
