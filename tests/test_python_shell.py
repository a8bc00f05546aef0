"""The Python shell over pbSim* and pbHost* states each fact once (no GPU needed):
1. _capi.row_dict, the one rule that turns a C row into a dict, on hand-built rows: one row per clause of the rule.
2. Sim and HostSim agree on the parameters of every method both define, but for a known few.
3. host.SYMBOLS names every pbHost* function of the host library's sources, and host.lib() binds them all at once.
4. Every recorder's info call returns exactly the keys of its spec, in order, and a refusing wrapper raises the method's
   own text."""
import ctypes as C
import glob
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_dict_composes_a_negative_128_bit_sum_and_keeps_the_float():
    from particlerobotsimulations_amd import _capi
    r = _capi.pbMomentsRow(step=7, time=0.25, measured=3, sum_qx=-5, sum_qy=6, sum_qr=7, sum_wx=-8, sum_wy=9,
                           min_qx=-10, max_qx=11, min_qy=-12, max_qy=13)
    r.xx.lo, r.xx.hi = 5, -1                      # -2^32 + 5
    r.yy.lo, r.yy.hi = (1 << 32) - 1, 2           # 3 * 2^32 - 1
    r.xy.lo, r.xy.hi = 0, -(1 << 63)              # the most negative value: -2^95
    r.rr.lo, r.rr.hi = 1 << 40, 0                 # lo need not be normalised below 2^32
    r.vv.lo, r.vv.hi = 0, 0
    d = _capi.row_dict(r)
    assert d == {"step": 7, "time": 0.25, "measured": 3, "sum_qx": -5, "sum_qy": 6, "sum_qr": 7, "sum_wx": -8,
                 "sum_wy": 9, "min_qx": -10, "max_qx": 11, "min_qy": -12, "max_qy": 13,
                 "xx": -4294967291, "yy": 12884901887, "xy": -39614081257132168796771975168, "rr": 1099511627776,
                 "vv": 0}
    assert list(d) == [name for name, _ in _capi.pbMomentsRow._fields_]
    assert type(d["time"]) is float and all(type(v) is int for k, v in d.items() if k != "time")


def test_row_dict_turns_an_array_field_into_a_list_of_ints():
    from particlerobotsimulations_amd import _capi
    r = _capi.pbStructureStats(bonds=12, psi6_re=-3, psi6_im=4)
    r.coordination[:] = [1, 0, 2, 0, 0, 0, 5, 4294967295]
    d = _capi.row_dict(r)
    assert d == {"bonds": 12, "psi6_re": -3, "psi6_im": 4, "coordination": [1, 0, 2, 0, 0, 0, 5, 4294967295]}
    assert type(d["coordination"]) is list and all(type(v) is int for v in d["coordination"])
    # structure_row adds only psi6
    s = _capi.structure_row(r)
    assert s == dict(d, psi6=complex(-3 / 2 ** 30, 4 / 2 ** 30) / 12) and list(s)[-1] == "psi6"


def test_row_dict_leaves_reserved_out():
    from particlerobotsimulations_amd import _capi
    t = _capi.pbCorrelationTotals(measured=9, reserved=0xDEAD, sum_ax=-2, sum_ay=3, pairs=72)
    t.sum_a2.lo, t.sum_a2.hi = 7, 1
    d = _capi.row_dict(t)
    assert d == {"measured": 9, "sum_ax": -2, "sum_ay": 3, "sum_a2": 4294967303, "pairs": 72}
    assert list(d) == ["measured", "sum_ax", "sum_ay", "sum_a2", "pairs"]


def test_rearrangement_row_composes_its_two_64_bit_halves_on_top_of_row_dict():
    from particlerobotsimulations_amd import _capi
    r = _capi.pbRearrangementStats(bonds_marked=10, bonds_now=8, bonds_kept=6, bots_unchanged=1, bots_lost=2,
                                   bots_gained=3, measured=4, sum_qx=-7, sum_qy=9, sum_q2_lo=(1 << 64) - 1, sum_q2_hi=2,
                                   max_q2=11)
    plain = _capi.row_dict(r)  # the rule itself knows nothing of the halves
    assert plain["sum_q2_lo"] == 18446744073709551615 and plain["sum_q2_hi"] == 2 and "sum_q2" not in plain
    d = _capi.rearrangement_row(r)
    assert d == {"bonds_marked": 10, "bonds_now": 8, "bonds_kept": 6, "bots_unchanged": 1, "bots_lost": 2,
                 "bots_gained": 3, "measured": 4, "sum_qx": -7, "sum_qy": 9, "max_q2": 11,
                 "sum_q2": 55340232221128654847}  # 2 * 2^64 + 2^64 - 1: halves of 64 bits, not hi * 2^32 + lo
    assert list(d)[-2:] == ["max_q2", "sum_q2"]


# where HostSim, which holds one simulation, takes no member (or another camera): as they were before the shell was folded
KNOWN_DIFFERENCES = {
    "centroid_trail": ("(self, member=0)", "(self)"),
    "cluster_labels": ("(self, gap=0.0, member=0)", "(self, gap=0.0)"),
    "contact_virial": ("(self, gap=0.0, member=0)", "(self, gap=0.0)"),
    "contacts": ("(self, gap=0.0, member=0)", "(self, gap=0.0)"),
    "render": ("(self, width, height, center=(0.0, 0.0), half_extent=1.0, light_radius=0.25, style='plain', member=0)",
               "(self, width, height, center=(0.0, 0.0), half_extent=0.0, style='plain')"),
}


def test_sim_and_hostsim_agree_on_the_parameters_of_every_method_both_define():
    import particlerobotsimulations_amd as pb
    from particlerobotsimulations_amd import host

    def public(cls):
        return {n for n, f in inspect.getmembers(cls, inspect.isfunction) if not n.startswith("_")}

    both = public(pb.Sim) & public(host.HostSim)
    assert len(both) == 38 and {"strain_of", "hexatic", "field_map", "structure_factor", "van_hove"} <= both
    differ = {}
    for name in sorted(both):
        a, b = inspect.signature(getattr(pb.Sim, name)), inspect.signature(getattr(host.HostSim, name))
        if [(p.name, p.default, p.kind) for p in a.parameters.values()] != \
                [(p.name, p.default, p.kind) for p in b.parameters.values()]:
            differ[name] = (str(a), str(b))
    assert differ == KNOWN_DIFFERENCES


def test_a_sim_is_a_batch_of_one_with_the_per_member_state_calls():
    import particlerobotsimulations_amd as pb
    assert pb.Sim.nsims == 1 and "nsims" in vars(pb.Sim)
    for name in ("set_state_of", "get_state_of"):  # whatever has nsims can be asked for one member's state
        assert name in vars(pb.Sim) and name not in vars(pb.Ensemble)
    assert str(inspect.signature(pb.Ensemble.set_state_of)) == \
        "(self, member, pos=None, vel=None, rad=None, phase=None, dead=None)"
    assert str(inspect.signature(pb.Ensemble.get_state_of)) == "(self, member)"


def test_host_symbols_cover_every_pbhost_function_of_the_host_library():
    from particlerobotsimulations_amd import host
    definition = re.compile(r"^[A-Za-z_][\w \*]*?\b(pbHost\w+)\s*\([^;]*?\)\s*\{", re.M | re.S)  # at column 0, with a body
    defined = set()
    for path in glob.glob(os.path.join(ROOT, "particlerobotsimulations_amd", "csrc", "*.cpp")):
        with open(path) as f:
            defined |= set(definition.findall(f.read()))
    assert len(defined) > 60 and {"pbHostWriteFrame", "pbHostGetResources", "pbHostVanHoveDistinctRows"} <= defined
    assert defined == set(host.SYMBOLS)
    L = host.lib()
    for name, (res, args) in host.SYMBOLS.items():
        fn = getattr(L, name)
        if name != "pbHostGetResources":  # (ensemble.host_resources() narrows this one's pointer to its own structure)
            assert fn.restype == res and fn.argtypes == args, name


def test_write_frame_is_bound_before_any_frame_is_written():
    from particlerobotsimulations_amd import host
    fn = host.lib().pbHostWriteFrame
    assert fn.argtypes == [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float]
    assert fn.restype is C.c_int


INFO = [  # (method, spec name, keys in order, HostSim's RuntimeError on an engine without the analysis)
    ("series_info", "SERIES_INFO", ["interval", "capacity", "records"],
     "series_info: the time series needs the fused engine"),
    ("time_correlation_info", "TIME_CORRELATION_INFO", ["interval", "lags", "overlap_radius", "records"],
     "time_correlation_info: the time correlation needs the fused engine"),
    ("scattering_info", "SCATTERING_INFO", ["interval", "lags", "box_log2", "nvec", "records"],
     "scattering_info: the scattering needs the fused engine"),
    ("van_hove_info", "VAN_HOVE_INFO", ["interval", "lags", "width", "bins", "records"],
     "van_hove_info: the van Hove function needs the fused engine"),
    ("van_hove_distinct_info", "VAN_HOVE_DISTINCT_INFO", ["interval", "lags", "width", "bins", "records"],
     "van_hove_distinct_info: the distinct van Hove function needs the fused engine"),
]


@pytest.fixture(scope="module")
def placement_only():
    from particlerobotsimulations_amd import host
    h = host.HostSim(os.path.join(ROOT, "examples", "example.cfg"), engine="host")
    yield h
    h.close()


@pytest.mark.parametrize("method,spec,keys,refused", INFO, ids=[i[0] for i in INFO])
def test_info_reader_returns_its_specs_keys_and_a_refusal_keeps_its_text(placement_only, method, spec, keys, refused):
    from particlerobotsimulations_amd import _analysis
    fields = getattr(_analysis, spec)
    assert [name for name, _ in fields] == keys
    want = {name: (k + 1.5 if ctype is C.c_float else k + 1) for k, (name, ctype) in enumerate(fields)}

    def call(*pointers):  # what a C info call does: one value through every pointer
        assert len(pointers) == len(fields)
        for p, value in zip(pointers, want.values()):
            p._obj.value = value

    d = _analysis.read_info(fields, call)
    assert d == want and list(d) == keys
    assert all(type(d[name]) is (float if ctype is C.c_float else int) for name, ctype in fields)
    with pytest.raises(RuntimeError) as caught:
        getattr(placement_only, method)()
    assert str(caught.value) == refused
