"""ctypes binding of libparticlebot_hip.so (the C-ABI declared in include/particlebot_hip.h).

No fallback: if the HIP library is missing, importing the symbols raises.  Nothing here touches
oracle/.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_PKG, "lib")
HIP_SO = os.path.join(LIB_DIR, "libparticlebot_hip.so")
HOST_SO = os.path.join(LIB_DIR, "libparticlebot_host.so")

PB_MAX_OBSTACLES = 10
PB_OK = 0


class uint2(C.Structure):
    _fields_ = [("x", C.c_uint), ("y", C.c_uint)]


class float2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class SimParams(C.Structure):
    """include/particlebot_kernel.h (layout of the reference's particlebot_kernel.cuh:58-120):
    256 bytes, checked against the C++ struct by a static_assert in csrc/pb_device.hpp."""
    _fields_ = [
        ("gridSize", uint2), ("numCells", C.c_uint),
        ("_pad0", C.c_uint),  # float2 is 8-byte aligned in HIP (and CUDA): hole after numCells
        ("worldOrigin", float2), ("cellSize", float2),
        ("nCells", C.c_uint), ("nDead", C.c_int), ("maxParticlebotsPerCell", C.c_uint),
        ("gravity", C.c_float), ("spring", C.c_float), ("damping", C.c_float), ("shear", C.c_float),
        ("attraction", C.c_float), ("boundaryDamping", C.c_float), ("friction", C.c_float),
        ("massFactor", C.c_float), ("frictionFactor", C.c_float), ("radFactor", C.c_float),
        ("attractionFactor", C.c_float),
        ("constraint", C.c_float), ("constraint_contraction", C.c_float),
        ("centroid_steps", C.c_int), ("centroid_int", C.c_float), ("centroid_radius", C.c_float),
        ("light_x", C.c_float), ("light_y", C.c_float), ("phase_update_interval", C.c_float),
        ("control", C.c_int), ("config", C.c_int),
        ("min_radius", C.c_float), ("max_radius", C.c_float), ("rise_period", C.c_float),
        ("freq", C.c_float),
        ("nobstacles", C.c_int),
        ("x1obs", C.POINTER(C.c_float)), ("x2obs", C.POINTER(C.c_float)),
        ("y1obs", C.POINTER(C.c_float)), ("y2obs", C.POINTER(C.c_float)),
        ("n_cir_obstacles", C.c_int),
        ("x_cir_obs", C.POINTER(C.c_float)), ("y_cir_obs", C.POINTER(C.c_float)),
        ("r_cir_obs", C.POINTER(C.c_float)),
        ("Nx", C.c_int), ("phase_std", C.c_float), ("seed", C.c_uint),
        ("light_shadow", C.c_uint), ("testing", C.c_uint), ("constrained_contraction", C.c_uint),
        ("display_shadow", C.c_uint), ("time_to_dead", C.c_float), ("max_time", C.c_float),
    ]


class pbRngState(C.Structure):
    """48 bytes = sizeof(curandStateXORWOW) (include/particlebot_hip.h)."""
    _fields_ = [("d", C.c_uint), ("v", C.c_uint * 5), ("boxmuller_flag", C.c_int), ("kind", C.c_int),
                ("boxmuller_extra", C.c_float), ("reserved", C.c_float * 3)]


PB_RNG_COUNTER, PB_RNG_XORWOW_CURAND, PB_RNG_XORWOW_ROCRAND = 0, 1, 2


class pbSimStats(C.Structure):
    _fields_ = [("steps", C.c_ulonglong), ("fused_launches", C.c_ulonglong),
                ("plain_launches", C.c_ulonglong), ("state_launches", C.c_ulonglong),
                ("resorts", C.c_ulonglong), ("phase_updates", C.c_ulonglong),
                ("resident_launches", C.c_ulonglong)]


class pbSimConfig(C.Structure):
    _fields_ = [("force_variant", C.c_int), ("force_kind", C.c_int), ("lanes_per_bot", C.c_int),
                ("resident", C.c_int), ("fast_math_ok", C.c_int), ("payload", C.c_int), ("rng", C.c_int), ("offsets64", C.c_int),
                ("attraction_sums", C.c_int), ("dead_sum_form", C.c_int), ("stream_walk", C.c_int),
                ("tail_tiles", C.c_int), ("tail_lanes", C.c_int)]


class pbRenderView(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("centerX", C.c_float), ("centerY", C.c_float),
                ("halfExtent", C.c_float), ("lightRadius", C.c_float), ("style", C.c_int)]


class pbMoment128(C.Structure):
    _fields_ = [("lo", C.c_ulonglong), ("hi", C.c_longlong)]


def row_dict(row):
    """A C row as a dict, by one rule for every structure here: `reserved` is left out; a pbMoment128 becomes the 128-bit
    sum hi * 2^32 + lo as one Python int; an array field a list of ints; a c_float a float; anything else an int."""
    d = {}
    for name, kind in row._fields_:
        if name == "reserved":
            continue
        v = getattr(row, name)
        if kind is pbMoment128:
            d[name] = (int(v.hi) << 32) + int(v.lo)
        elif issubclass(kind, C.Array):
            d[name] = [int(x) for x in v]
        else:
            d[name] = float(v) if kind is C.c_float else int(v)
    return d


def compose_128(records, name):
    """The 128-bit column `name` of a numpy record array (one of the *_DTYPEs): records[name + "_hi"] * 2^32 +
    records[name + "_lo"] as an object array of Python ints, shaped like `records`."""
    flat = [(int(h) << 32) + int(l)
            for h, l in zip(records[name + "_hi"].reshape(-1), records[name + "_lo"].reshape(-1))]
    big = np.empty(len(flat), object)
    big[:] = flat
    return big.reshape(records.shape)


class pbClusterStats(C.Structure):
    _fields_ = [("clusters", C.c_uint), ("largest", C.c_uint), ("largest_label", C.c_uint), ("isolated", C.c_uint),
                ("links", C.c_ulonglong), ("max_degree", C.c_uint), ("rounds", C.c_uint)]


class pbContactLink(C.Structure):
    _fields_ = [("other", C.c_uint), ("gap", C.c_float), ("fx", C.c_float), ("fy", C.c_float)]


class pbStructureStats(C.Structure):
    _fields_ = [("bonds", C.c_ulonglong), ("psi6_re", C.c_longlong), ("psi6_im", C.c_longlong),
                ("coordination", C.c_uint * 8)]


def structure_row(r):
    """A pbStructureStats row as a dict: row_dict(r), and psi6 = (psi6_re + i psi6_im) / 2^30 / bonds as a Python complex
    (0 without bonds): the mean of e^(6 i theta) over the member's directed bonds."""
    d = row_dict(r)
    bonds = d["bonds"]
    d["psi6"] = complex(d["psi6_re"] / 1073741824.0, d["psi6_im"] / 1073741824.0) / bonds if bonds else 0j
    return d


class pbRearrangementStats(C.Structure):
    _fields_ = [("bonds_marked", C.c_ulonglong), ("bonds_now", C.c_ulonglong), ("bonds_kept", C.c_ulonglong),
                ("bots_unchanged", C.c_uint), ("bots_lost", C.c_uint), ("bots_gained", C.c_uint), ("measured", C.c_uint),
                ("sum_qx", C.c_longlong), ("sum_qy", C.c_longlong),
                ("sum_q2_lo", C.c_ulonglong), ("sum_q2_hi", C.c_ulonglong), ("max_q2", C.c_ulonglong)]


def rearrangement_row(r):
    """A pbRearrangementStats row as a dict of Python ints: row_dict(r) with sum_q2, the 128-bit sum of two 64-bit halves
    (sum_q2_hi * 2^64 + sum_q2_lo), as one int.  Bond counts are directed; sum_qx / sum_qy are in units of 2^-20, sum_q2
    and max_q2 in units of 2^-40."""
    d = row_dict(r)
    lo, hi = d.pop("sum_q2_lo"), d.pop("sum_q2_hi")
    d["sum_q2"] = (hi << 64) | lo
    return d


class pbMomentsRow(C.Structure):
    _fields_ = [("step", C.c_ulonglong), ("time", C.c_float), ("measured", C.c_uint),
                ("sum_qx", C.c_longlong), ("sum_qy", C.c_longlong), ("sum_qr", C.c_longlong),
                ("sum_wx", C.c_longlong), ("sum_wy", C.c_longlong),
                ("min_qx", C.c_int), ("max_qx", C.c_int), ("min_qy", C.c_int), ("max_qy", C.c_int),
                ("xx", pbMoment128), ("yy", pbMoment128), ("xy", pbMoment128), ("rr", pbMoment128), ("vv", pbMoment128)]


class pbStrainStats(C.Structure):
    _fields_ = [("fitted", C.c_uint), ("unfitted", C.c_uint), ("above", C.c_uint), ("reserved", C.c_uint),
                ("bonds_used", C.c_ulonglong), ("bonds_dropped", C.c_ulonglong),
                ("yxx", pbMoment128), ("yxy", pbMoment128), ("yyy", pbMoment128), ("xxx", pbMoment128),
                ("xxy", pbMoment128), ("xyx", pbMoment128), ("xyy", pbMoment128), ("w", pbMoment128),
                ("sum_d2", pbMoment128), ("max_d2", C.c_ulonglong)]


PB_STRAIN_MOMENTS = ("k", "yxx", "yxy", "yyy", "xxx", "xxy", "xyx", "xyy", "w")  # a bot's nine words, in order


class pbCorrelationBin(C.Structure):
    _fields_ = [("pairs", C.c_ulonglong), ("dot", pbMoment128), ("ax", pbMoment128), ("ay", pbMoment128)]


class pbCorrelationTotals(C.Structure):
    _fields_ = [("measured", C.c_uint), ("reserved", C.c_uint), ("sum_ax", C.c_longlong), ("sum_ay", C.c_longlong),
                ("sum_a2", pbMoment128), ("pairs", C.c_ulonglong)]


PB_CORR_KINDS = {"velocity": 0, "displacement": 1, "radius": 2}
# pbCorrelationBin as a numpy record: each 128-bit value is hi * 2^32 + lo, normalised to 0 <= lo < 2^32
CORRELATION_BIN_DTYPE = np.dtype([("pairs", np.uint64), ("dot_lo", np.uint64), ("dot_hi", np.int64),
                                  ("ax_lo", np.uint64), ("ax_hi", np.int64), ("ay_lo", np.uint64), ("ay_hi", np.int64)])


def correlation_kind(kind):
    """PB_CORR_* from an int or from "velocity" | "displacement" | "radius"."""
    if isinstance(kind, str):
        if kind not in PB_CORR_KINDS:
            raise ValueError(f"pair_correlation: unknown kind {kind!r}")
        return PB_CORR_KINDS[kind]
    return int(kind)


class pbTimeCorrelationRow(C.Structure):
    _fields_ = [("lag", C.c_uint), ("reserved", C.c_uint), ("origins", C.c_ulonglong), ("sum_steps", C.c_ulonglong),
                ("samples", C.c_ulonglong), ("sum_qx", C.c_longlong), ("sum_qy", C.c_longlong),
                ("msd", pbMoment128), ("vacf", pbMoment128), ("overlap", C.c_ulonglong), ("max_q2", C.c_ulonglong)]


class pbFieldView(C.Structure):
    _fields_ = [("nx", C.c_uint), ("ny", C.c_uint), ("centerX", C.c_float), ("centerY", C.c_float),
                ("halfX", C.c_float), ("halfY", C.c_float)]


class pbFieldCell(C.Structure):
    _fields_ = [("count", C.c_uint), ("dead", C.c_uint), ("sum_qr", C.c_longlong), ("sum_wx", C.c_longlong),
                ("sum_wy", C.c_longlong), ("rr", pbMoment128), ("vv", pbMoment128)]


class pbFieldTotals(C.Structure):
    _fields_ = [("measured", C.c_uint), ("inside", C.c_uint), ("outside", C.c_uint), ("unmeasured", C.c_uint)]


# pbFieldCell as a numpy record: each 128-bit value is hi * 2^32 + lo, normalised to 0 <= lo < 2^32
FIELD_CELL_DTYPE = np.dtype([("count", np.uint32), ("dead", np.uint32), ("sum_qr", np.int64), ("sum_wx", np.int64),
                             ("sum_wy", np.int64), ("rr_lo", np.uint64), ("rr_hi", np.int64), ("vv_lo", np.uint64),
                             ("vv_hi", np.int64)])


def field_view(nx, ny, center, half):
    """A pbFieldView of nx x ny cells centred on `center` = (x, y); `half` is one half extent or (halfX, halfY)."""
    hx, hy = (half, half) if np.isscalar(half) else half
    return pbFieldView(int(nx), int(ny), float(center[0]), float(center[1]), float(hx), float(hy))


class pbStructureFactorRow(C.Structure):
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("measured", C.c_uint), ("reserved", C.c_uint),
                ("re", pbMoment128), ("im", pbMoment128), ("re2", pbMoment128), ("im2", pbMoment128)]


# pbStructureFactorRow as a numpy record: each 128-bit value is hi * 2^32 + lo, normalised to 0 <= lo < 2^32
SK_ROW_DTYPE = np.dtype([("nx", np.int32), ("ny", np.int32), ("measured", np.uint32), ("reserved", np.uint32),
                         ("re_lo", np.uint64), ("re_hi", np.int64), ("im_lo", np.uint64), ("im_hi", np.int64),
                         ("re2_lo", np.uint64), ("re2_hi", np.int64), ("im2_lo", np.uint64), ("im2_hi", np.int64)])
SK_KINDS = {"density": 0, "radius": 1, "velocity": 2}
SK_MAX_VECTORS = 4096
PHASOR_STEPS = 4096


def sk_kind(kind):
    """PB_SK_* of a kind given by name or by number; a number the engine does not know goes through for it to refuse."""
    if isinstance(kind, str):
        if kind not in SK_KINDS:
            raise ValueError("structure_factor: kind must be 'density', 'radius' or 'velocity', not %r" % (kind,))
        return SK_KINDS[kind]
    return int(kind)


def sk_vectors(vectors):
    """The caller's wavevectors as a C-contiguous (nvec, 2) int32 array; every entry must be an int32's."""
    v = np.asarray(vectors)
    if v.ndim != 2 or v.shape[1] != 2 or v.dtype.kind not in "iu":
        raise ValueError("structure_factor: vectors must be an (nvec, 2) array of integers")
    if v.size and (int(v.min()) < -(1 << 31) or int(v.max()) >= 1 << 31):
        raise ValueError("structure_factor: every nx and ny must fit an int")
    return np.ascontiguousarray(v, np.int32)


class pbScatteringRow(C.Structure):
    _fields_ = [("lag", C.c_uint), ("nx", C.c_int), ("ny", C.c_int), ("reserved", C.c_uint),
                ("origins", C.c_ulonglong), ("sum_steps", C.c_ulonglong), ("samples", C.c_ulonglong),
                ("re", C.c_longlong), ("im", C.c_longlong)]


SCATTER_MAX_LAGS = 64
SCATTER_MAX_VECTORS = 256


class pbVanHoveRow(C.Structure):
    _fields_ = [("lag", C.c_uint), ("reserved", C.c_uint), ("origins", C.c_ulonglong), ("sum_steps", C.c_ulonglong),
                ("samples", C.c_ulonglong), ("beyond_r", C.c_ulonglong), ("beyond_x", C.c_ulonglong),
                ("beyond_y", C.c_ulonglong), ("msd", pbMoment128), ("q4", C.c_ulonglong * 3)]


VANHOVE_MAX_LAGS = 64
VANHOVE_MAX_BINS = 1024


def van_hove_row(r):
    """A pbVanHoveRow as a dict of Python ints: row_dict(r) (msd in units of 2^-40) with q4 composed from its three
    little-endian 64-bit limbs (units of 2^-80)."""
    d = row_dict(r)
    d["q4"] = d["q4"][0] + (d["q4"][1] << 64) + (d["q4"][2] << 128)
    return d


class pbVanHoveDistinctRow(C.Structure):
    _fields_ = [("lag", C.c_uint), ("reserved", C.c_uint), ("origins", C.c_ulonglong), ("sum_steps", C.c_ulonglong),
                ("centres", C.c_ulonglong), ("partners", C.c_ulonglong), ("pairs", C.c_ulonglong)]


class pbCoherentRow(C.Structure):
    _fields_ = [("lag", C.c_uint), ("nx", C.c_int), ("ny", C.c_int), ("reserved", C.c_uint),
                ("origins", C.c_ulonglong), ("sum_steps", C.c_ulonglong), ("bots_now", C.c_ulonglong),
                ("bots_then", C.c_ulonglong), ("re", C.c_ulonglong * 3), ("im", C.c_ulonglong * 3)]


COHERENT_MAX_LAGS = 64
COHERENT_MAX_VECTORS = 256


def signed_192(limbs):
    """The signed 192-bit two's-complement value of three little-endian 64-bit limbs as one Python int."""
    v = int(limbs[0]) + (int(limbs[1]) << 64) + (int(limbs[2]) << 128)
    return v - (1 << 192) if v >> 191 else v


def coherent_row(r):
    """A pbCoherentRow as a dict of Python ints: row_dict(r) with re and im composed from their limbs (units of 2^-60)."""
    d = row_dict(r)
    d["re"], d["im"] = signed_192(d["re"]), signed_192(d["im"])
    return d


class pbFourPointRow(C.Structure):
    _fields_ = [("lag", C.c_uint), ("nx", C.c_int), ("ny", C.c_int), ("reserved", C.c_uint),
                ("origins", C.c_ulonglong), ("sum_steps", C.c_ulonglong), ("samples", C.c_ulonglong),
                ("overlap", C.c_ulonglong), ("overlap2", C.c_ulonglong * 2), ("re", C.c_ulonglong * 2),
                ("im", C.c_ulonglong * 2), ("power", C.c_ulonglong * 3), ("reserved2", C.c_ulonglong)]


# pbFourPointRow as a numpy record
FOUR_POINT_ROW_DTYPE = np.dtype([("lag", np.uint32), ("nx", np.int32), ("ny", np.int32), ("reserved", np.uint32),
                                 ("origins", np.uint64), ("sum_steps", np.uint64), ("samples", np.uint64),
                                 ("overlap", np.uint64), ("overlap2", np.uint64, (2,)), ("re", np.uint64, (2,)),
                                 ("im", np.uint64, (2,)), ("power", np.uint64, (3,)), ("reserved2", np.uint64)])
FOURPOINT_MAX_LAGS = 64
FOURPOINT_MAX_VECTORS = 256


def signed_128(limbs):
    """The signed 128-bit two's-complement value of two little-endian 64-bit limbs as one Python int."""
    v = int(limbs[0]) + (int(limbs[1]) << 64)
    return v - (1 << 128) if v >> 127 else v


def four_point_row(r):
    """A pbFourPointRow as a dict of Python ints: row_dict(r) with overlap2 and power composed from their limbs as
    unsigned values, re and im as signed 128-bit ones (units of 2^-30; power in units of 2^-60)."""
    d = row_dict(r)
    del d["reserved2"]
    d["overlap2"] = int(d["overlap2"][0]) + (int(d["overlap2"][1]) << 64)
    d["re"], d["im"], d["power"] = signed_128(d["re"]), signed_128(d["im"]), signed_192(d["power"])
    return d


class pbBondRow(C.Structure):
    _fields_ = [("lag", C.c_uint), ("reserved", C.c_uint), ("origins", C.c_ulonglong), ("sum_steps", C.c_ulonglong),
                ("samples", C.c_ulonglong), ("crowded", C.c_ulonglong), ("bonds_then", C.c_ulonglong),
                ("bonds_now", C.c_ulonglong), ("bonds_kept", C.c_ulonglong), ("bots_unchanged", C.c_ulonglong),
                ("bots_lost", C.c_ulonglong), ("bots_gained", C.c_ulonglong), ("plain_q2", pbMoment128),
                ("cage_samples", C.c_ulonglong * 8), ("cage_overlap", C.c_ulonglong * 8), ("cage_q2", pbMoment128 * 8)]


# pbBondRow as a numpy record: each 128-bit value is hi * 2^32 + lo, normalised to 0 <= lo < 2^32; cage_q2 is (8, 2)
# words, (lo, hi) per k, the hi read as a signed word
BOND_ROW_DTYPE = np.dtype([("lag", np.uint32), ("reserved", np.uint32), ("origins", np.uint64), ("sum_steps", np.uint64),
                           ("samples", np.uint64), ("crowded", np.uint64), ("bonds_then", np.uint64),
                           ("bonds_now", np.uint64), ("bonds_kept", np.uint64), ("bots_unchanged", np.uint64),
                           ("bots_lost", np.uint64), ("bots_gained", np.uint64), ("plain_q2_lo", np.uint64),
                           ("plain_q2_hi", np.int64), ("cage_samples", np.uint64, (8,)),
                           ("cage_overlap", np.uint64, (8,)), ("cage_q2", np.uint64, (8, 2))])
BOND_MAX_LAGS = 64
BOND_WIDTH = 8


def bond_row(r):
    """A pbBondRow as a dict of Python ints: the counts as they are, plain_q2 and the eight cage_q2 composed as
    hi * 2^32 + lo (units of 2^-40; cage_q2[k - 1] is k^2 times the cage-relative sum)."""
    d = {}
    for name, kind in r._fields_:
        if name == "reserved":
            continue
        v = getattr(r, name)
        if name == "cage_q2":
            d[name] = [(int(m.hi) << 32) + int(m.lo) for m in v]
        elif kind is pbMoment128:
            d[name] = (int(v.hi) << 32) + int(v.lo)
        elif issubclass(kind, C.Array):
            d[name] = [int(x) for x in v]
        else:
            d[name] = int(v)
    return d


# pbContactLink as a numpy record
CONTACT_LINK_DTYPE = np.dtype([("other", np.uint32), ("gap", np.float32), ("fx", np.float32), ("fy", np.float32)])


class pbForceForm(C.Structure):
    _fields_ = [("flat", C.c_int), ("lanes_per_bot", C.c_int), ("attraction_sums", C.c_int), ("offsets64", C.c_int)]


# every symbol include/particlebot_hip.h declares: name -> (restype, argtypes)
_VP = C.c_void_p
_F = C.c_float
_U = C.c_uint
_I = C.c_int
SYMBOLS = {
    "cudaInit": (None, [_I, _VP]),
    "cudaGLInit": (None, [_I, _VP]),
    "allocateArray": (None, [C.POINTER(_VP), C.c_size_t]),
    "freeArray": (None, [_VP]),
    "threadSync": (None, []),
    "copyArrayFromDevice": (None, [_VP, _VP, _VP, _I]),
    "copyArrayToDevice": (None, [_VP, _VP, _I, _I]),
    "registerGLBufferObject": (None, [_U, C.POINTER(_VP)]),
    "unregisterGLBufferObject": (None, [_VP]),
    "mapGLBufferObject": (_VP, [C.POINTER(_VP)]),
    "unmapGLBufferObject": (None, [_VP]),
    "pbCreateBuffer": (_U, [C.c_size_t]),
    "pbBufferSubData": (None, [_U, C.c_size_t, C.c_size_t, _VP]),
    "pbDeleteBuffer": (None, [_U]),
    "setParameters": (None, [C.POINTER(SimParams)]),
    "pbSetWallHalfExtent": (None, [_F]),
    "integrateSystem": (None, [_VP, _VP, _VP, _F, _U, _F]),
    "calcHash": (None, [_VP, _VP, _VP, _I]),
    "reorderDataAndFindCellStart": (None, [_VP] * 10 + [_U, _U]),
    "updateRad_light_wave": (None, [_VP, _VP, _VP, _VP, _VP, _F, _F, _VP, _I]),
    "curand_setup": (None, [_VP, _I]),
    "add_normal_noise": (None, [_VP, _VP, _F, _I]),
    "updatePhase": (None, [_VP, _VP, _F, _F, _F, _I]),
    "updateCol": (None, [_VP, _VP, _I, _VP, _VP, _VP]),
    "collide": (None, [_VP] * 9 + [_U, _U, _F]),
    "calcCOG": (None, [_VP, _VP, _VP, _I, _F, _I, _F]),
    "sortParticlebots": (None, [_VP, _VP, _U]),
    "pbGetLastErrorString": (C.c_char_p, []),
    "pbGetDevice": (_I, [C.POINTER(_I)]),
    "pbDevicePciBusId": (_I, [_I, C.c_char_p, _I]),
    "pbDeviceMemoryLive": (_I, [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "pbSetDevice": (_I, [_I]),
    "pbSimCreate": (_I, [C.POINTER(_VP), C.POINTER(SimParams), _F]),
    "pbSimDestroy": (None, [_VP]),
    "pbSimCreateBatch": (_I, [C.POINTER(_VP), C.POINTER(SimParams), _I, _F]),
    "pbSimBatchSize": (_I, [_VP, C.POINTER(_U), C.POINTER(_U)]),
    "pbSimSetStateOf": (_I, [_VP, _U, _VP, _VP, _VP, _VP, _VP]),
    "pbSimSetStateRangeOf": (_I, [_VP, _U, _U, _U, _VP, _VP, _VP, _VP, _VP]),
    "pbSimGetStateOf": (_I, [_VP, _U] + [_VP] * 7),
    "pbSimCentroids": (_I, [_VP, C.POINTER(C.c_double)]),
    "pbSimCentroidSums": (_I, [_VP, C.POINTER(C.c_float)]),
    "pbSimGetColorsOf": (_I, [_VP, _U, _VP]),
    "pbSimSetCentroidTrail": (_I, [_VP, _I]),
    "pbSimGetCentroidTrailOf": (_I, [_VP, _U, _VP, _VP, C.POINTER(_U)]),
    "pbSimRenderOf": (_I, [_VP, _U, C.POINTER(pbRenderView), _VP]),
    "pbSimGetRenderStats": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimClusterStats": (_I, [_VP, _F, C.POINTER(pbClusterStats)]),
    "pbSimClusterLabelsOf": (_I, [_VP, _U, _F, _VP, _VP]),
    "pbSimGetClusterTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimContactsOf": (_I, [_VP, _U, _F, _VP, _VP, C.c_ulonglong, C.POINTER(C.c_ulonglong)]),
    "pbSimContactVirialOf": (_I, [_VP, _U, _F, _VP]),
    "pbSimGetContactTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimRadialCounts": (_I, [_VP, _F, _U, _VP]),
    "pbSimStructureStats": (_I, [_VP, _F, C.POINTER(pbStructureStats)]),
    "pbSimHexaticOf": (_I, [_VP, _U, _F, _VP, _VP]),
    "pbSimGetStructureTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimMarkReference": (_I, [_VP, _F]),
    "pbSimClearReference": (_I, [_VP]),
    "pbSimGetReferenceInfo": (_I, [_VP, C.POINTER(_I), C.POINTER(_F), C.POINTER(_F), C.POINTER(C.c_ulonglong)]),
    "pbSimRearrangementStats": (_I, [_VP, C.POINTER(pbRearrangementStats)]),
    "pbSimRearrangementOf": (_I, [_VP, _U, _VP, _VP, _VP, _VP]),
    "pbSimGetRearrangementTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimStrainStats": (_I, [_VP, _F, C.POINTER(pbStrainStats)]),
    "pbSimStrainOf": (_I, [_VP, _U, _VP, _VP, _VP]),
    "pbSimGetStrainTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimMoments": (_I, [_VP, C.POINTER(pbMomentsRow)]),
    "pbSimSetSeries": (_I, [_VP, _F, _U]),
    "pbSimGetSeriesInfo": (_I, [_VP, C.POINTER(_F), C.POINTER(_U), C.POINTER(C.c_ulonglong)]),
    "pbSimGetSeriesOf": (_I, [_VP, _U, C.c_ulonglong, _U, C.POINTER(pbMomentsRow)]),
    "pbSimGetSeriesTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimPairCorrelation": (_I, [_VP, _I, _F, _U, _VP, C.POINTER(pbCorrelationTotals)]),
    "pbSimGetCorrelationTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimSetTimeCorrelation": (_I, [_VP, _F, _U, _F]),
    "pbSimTimeCorrelationRecord": (_I, [_VP]),
    "pbSimGetTimeCorrelationInfo": (_I, [_VP, C.POINTER(_F), C.POINTER(_U), C.POINTER(_F), C.POINTER(C.c_ulonglong)]),
    "pbSimGetTimeCorrelation": (_I, [_VP, C.POINTER(pbTimeCorrelationRow)]),
    "pbSimGetTimeCorrelationTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimFieldMap": (_I, [_VP, C.POINTER(pbFieldView), _VP, C.POINTER(pbFieldTotals)]),
    "pbSimFieldMapOf": (_I, [_VP, _U, C.POINTER(pbFieldView), _VP, C.POINTER(pbFieldTotals)]),
    "pbSimGetFieldTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimStructureFactor": (_I, [_VP, _I, _I, _VP, _U, _VP]),
    "pbSimStructureFactorOf": (_I, [_VP, _U, _I, _I, _VP, _U, _VP]),
    "pbSimGetStructureFactorTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbPhasorTable": (_I, [_VP, _U]),
    "pbSimSetScattering": (_I, [_VP, _F, _U, _I, _VP, _U]),
    "pbSimScatteringRecord": (_I, [_VP]),
    "pbSimGetScatteringInfo": (_I, [_VP, C.POINTER(_F), C.POINTER(_U), C.POINTER(_I), C.POINTER(_U),
                                    C.POINTER(C.c_ulonglong)]),
    "pbSimGetScattering": (_I, [_VP, C.POINTER(pbScatteringRow)]),
    "pbSimGetScatteringTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimSetVanHove": (_I, [_VP, _F, _U, _F, _U]),
    "pbSimVanHoveRecord": (_I, [_VP]),
    "pbSimGetVanHoveInfo": (_I, [_VP, C.POINTER(_F), C.POINTER(_U), C.POINTER(_F), C.POINTER(_U),
                                 C.POINTER(C.c_ulonglong)]),
    "pbSimGetVanHove": (_I, [_VP, C.POINTER(pbVanHoveRow), C.POINTER(C.c_ulonglong)]),
    "pbSimGetVanHoveTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimSetVanHoveDistinct": (_I, [_VP, _F, _U, _F, _U]),
    "pbSimVanHoveDistinctRecord": (_I, [_VP]),
    "pbSimGetVanHoveDistinctInfo": (_I, [_VP, C.POINTER(_F), C.POINTER(_U), C.POINTER(_F), C.POINTER(_U),
                                         C.POINTER(C.c_ulonglong)]),
    "pbSimGetVanHoveDistinct": (_I, [_VP, C.POINTER(pbVanHoveDistinctRow), C.POINTER(C.c_ulonglong)]),
    "pbSimGetVanHoveDistinctTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimSetCoherent": (_I, [_VP, _F, _U, _I, _VP, _U]),
    "pbSimCoherentRecord": (_I, [_VP]),
    "pbSimGetCoherentInfo": (_I, [_VP, C.POINTER(_F), C.POINTER(_U), C.POINTER(_I), C.POINTER(_U),
                                  C.POINTER(C.c_ulonglong)]),
    "pbSimGetCoherent": (_I, [_VP, C.POINTER(pbCoherentRow)]),
    "pbSimGetCoherentTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimSetFourPoint": (_I, [_VP, _F, _U, _F, _I, _VP, _U]),
    "pbSimFourPointRecord": (_I, [_VP]),
    "pbSimGetFourPointInfo": (_I, [_VP, C.POINTER(_F), C.POINTER(_U), C.POINTER(_F), C.POINTER(_I), C.POINTER(_U),
                                   C.POINTER(C.c_ulonglong)]),
    "pbSimGetFourPoint": (_I, [_VP, C.POINTER(pbFourPointRow)]),
    "pbSimGetFourPointTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimSetBondDynamics": (_I, [_VP, _F, _U, _F, _F, _F]),
    "pbSimBondDynamicsRecord": (_I, [_VP]),
    "pbSimGetBondDynamicsInfo": (_I, [_VP, C.POINTER(_F), C.POINTER(_U), C.POINTER(_F), C.POINTER(_F), C.POINTER(_F),
                                      C.POINTER(C.c_ulonglong)]),
    "pbSimGetBondDynamics": (_I, [_VP, C.POINTER(pbBondRow)]),
    "pbSimGetBondDynamicsTimes": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(_F)]),
    "pbSimGetLayoutOf": (_I, [_VP, _U, _VP, _VP, C.POINTER(_I)]),
    "pbSimSetLayoutOf": (_I, [_VP, _U, _VP, _VP]),
    "pbSimSetForcesOf": (_I, [_VP, _U, _VP, _VP]),
    "pbSimSetState": (_I, [_VP, _VP, _VP, _VP, _VP, _VP]),
    "pbSimGetState": (_I, [_VP] * 8),
    "pbSimSetTime": (_I, [_VP, _F]),
    "pbSimGetTime": (_I, [_VP, C.POINTER(_F)]),
    "pbSimGetPhaseDraws": (_I, [_VP, C.POINTER(_U)]),
    "pbSimSetPhaseDraws": (_I, [_VP, _U]),
    "pbSimStep": (_I, [_VP, _F, _F, _I, C.POINTER(_I)]),
    "pbSimStepTimed": (_I, [_VP, _F, _F, _I, C.POINTER(_I), C.POINTER(_F)]),
    "pbSimStepTimedWall": (_I, [_VP, _F, _F, _I, C.POINTER(_I), C.POINTER(_F), C.POINTER(C.c_double)]),
    "pbSimSynchronize": (_I, [_VP]),
    "pbSimCentroid": (_I, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pbSimGetStats": (_I, [_VP, C.POINTER(pbSimStats)]),
    "pbSimSetResortEveryStep": (_I, [_VP, _I]),
    "pbSimSetMinDistanceMode": (_I, [_VP, _I]),
    "pbSetMinDistanceMode": (_I, [_I]),
    "pbGetMinDistanceMode": (_I, []),
    "pbHostSqrtThreshold": (C.c_float, [C.c_float]),
    "pbSimSetForceVariant": (_I, [_VP, _I]),
    "pbSimSetLanesPerBot": (_I, [_VP, _I]),
    "pbSimSetTailTiles": (_I, [_VP, _I]),
    "pbForceXcdTile": (_I, [_U, _U, _U, C.POINTER(_U), C.POINTER(_U)]),
    "pbSimSetResident": (_I, [_VP, _I]),
    "pbSimGetConfig": (_I, [_VP, C.POINTER(pbSimConfig)]),
    "pbSimSetForceSums": (_I, [_VP, _I]),
    "pbSimSetStreamWalk": (_I, [_VP, _I]),
    "pbSimGetStreamWalkTrips": (_I, [_VP, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "pbForceFormCount": (_I, []),
    "pbForceFormGet": (_I, [_I, C.POINTER(pbForceForm)]),
    "pbSimSelectForceForm": (_I, [_VP, _I]),
    "pbSimForceKernelName": (_I, [_VP, C.c_char_p, C.c_size_t]),
    "pbForceFormKernelName": (_I, [_I, _I, C.c_char_p, C.c_size_t]),
    "pbSimSetRng": (_I, [_VP, _I]),
    "pbSimGetRngStatesOf": (_I, [_VP, _U, _VP]),
    "pbSetRngKind": (_I, [_I]),
    "pbGetRngKind": (_I, []),
    "pbClockSampleBegin": (_I, [C.POINTER(_VP), C.c_double]),
    "pbClockSampleEnd": (_I, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pbSelfTest": (_I, [C.c_ulonglong] + [C.POINTER(C.c_ulonglong)] * 4),
    "pbSelfTestHoldThreshold": (_I, [C.c_float, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "pbSelfTestMagnitudeRoot": (_I, [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "pbSelfTestTermRoot": (_I, [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "pbSelfTestPairGeometry": (_I, [_U, _U, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "pbSelfTestDivision": (_I, [_U, _U, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
}

_lib = None


def lib():
    """Load libparticlebot_hip.so and bind every declared symbol.  Raises if the library or a
    symbol is missing: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(HIP_SO):
        raise RuntimeError(
            f"{HIP_SO} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    L = C.CDLL(HIP_SO, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc, what="call"):
    if rc != PB_OK:
        msg = lib().pbGetLastErrorString()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def np_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def make_params(d):
    """Build a SimParams from a dict of scalar fields + obstacle lists.  Returns (params, keepalive)."""
    P = SimParams()
    keep = []
    lists = {"x1obs", "x2obs", "y1obs", "y2obs", "x_cir_obs", "y_cir_obs", "r_cir_obs"}
    for k, v in d.items():
        if k in lists:
            continue
        if k == "gridSize":
            P.gridSize = uint2(int(v[0]), int(v[1]))
        elif k == "worldOrigin":
            P.worldOrigin = float2(float(v[0]), float(v[1]))
        elif k == "cellSize":
            P.cellSize = float2(float(v[0]), float(v[1]))
        else:
            setattr(P, k, v)
    for k in lists:
        vals = list(d.get(k, []))[:PB_MAX_OBSTACLES]
        arr = (C.c_float * max(1, len(vals)))(*[float(x) for x in vals])
        keep.append(arr)
        setattr(P, k, C.cast(arr, C.POINTER(C.c_float)))
    return P, keep
