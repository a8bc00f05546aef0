"""The inputs of the analysis-session tests (tests/test_analysis_session_cases_ref.py on the CPU,
tests/test_gpu_analysis_sessions.py on the device): the states, a catalogue of named analysis calls with the expectation
of each from the restatements the suite already has, six call orders per state, and the preconditions that make the
orders exercise what they are there for.  Nothing here touches a device: the states come from the CPU oracle, the
expectations from tests/*_ref.py, and bring() takes the package as an argument.

The states.  `batch3x300` is an Ensemble of three members of 300 bots (neither a multiple of 64 nor of 256; the analysis
grid is 32 x 16 cells per member): a jittered blob per member, member 1 with a tenth of its bots dead, stepped 120 steps
at sort_interval 0.5.  The mark at gap 0.0019 is taken after 90 of them.  After the last step six bots of member 1 are
made unmeasured (NaN x, inf y, x = -2048, vy = 2048, a NaN radius, a radius of 2048): planted before the steps they would
not survive them (the integrator clamps, the pair law spreads NaN), and the member would hold no measured bot at all.
set_state writes through the slot layout, so the slots stay out of original order and the engine's cell lists stale.
`single17` is one Sim of 17 bots (grid 8 x 4) brought to its state with set_state alone: marked at the blob, then moved.
The front end sizes the link rule's grid by the largest finite radius of the whole batch, so the radius of 2048 puts all
of batch3x300 into the four cells around the origin whenever a cluster, contact, hexatic or rearrangement call files it:
a sweep that walked a stale or foreign grid there would still meet every pair.  `batch3x300_small_radii` is the same
recipe without that one bot (five unmeasured bots): its link grids have edges of a bot's diameter, 32 x 16 cells that
fold, and differ from call to call with the gap.

Pair correlations take at most 1024 bins (PB_CORR_MAX_BINS), radial counts 4096: "the largest bin count the call takes"
is 1024 for the one and 4096 for the other.

A result is compared with its expectation the way the owning test file compares it (Entry.check), and with the result
of the same call on a fresh session bit for bit (same_bits)."""
import collections
import functools
import struct

import numpy as np

import cluster_ref as CR
import contacts_ref as NR
import correlation_ref as KR
import display_ref as DR
import dynamics_ref as YR
import field_ref as FR
import render_ref as RR
import series_ref as MR
import sfactor_ref as QR
import structure_ref as SR
from helpers import jittered_blob, simparams_from_orc

f32 = np.float32
DT = 0.01
SORT_INTERVAL = 0.5
STEPS, STEPS_AFTER_MARK = 120, 30
GAPS = (0.0, 0.0019, 0.05)
RADIAL = ((0.4, 7), (3.0, 4096), (0.25, 1))
CORRELATION = ((0.4, 7), (3.0, 1024), (0.25, 1))
FIELD_SHAPES = ((8, 8), (64, 48), (1, 1))
RENDER_SHAPES = ((8, 8), (64, 48), (5, 3))
SK_MOST = 4096                      # _capi.SK_MAX_VECTORS, asserted by the CPU test
SK_BOX = 4
# the marks: A the recipe's, on the earlier state; B and C taken by an entry of the catalogue, on the state itself
MARKS = {"A": 0.0019, "B": 0.05, "C": 0.0}
STATES = ("batch3x300", "single17")         # the two every test runs on
ALL_STATES = STATES + ("batch3x300_small_radii",)   # and the one more the call orders run on
ORDERS = ("catalogue", "reversed", "shuffle0", "shuffle1", "shuffle2", "shuffle3")
FILING = ("clusters", "contacts", "hexatic", "radial", "correlation")  # the families that re-file the bots, the mark aside
UNMEASURED = {10: "nan x", 40: "inf y", 77: "x -2048", 123: "vy 2048", 200: "nan radius", 290: "radius 2048"}

State = collections.namedtuple("State", "name nsims n params wall_half start at_mark mark_time final time view")
Entry = collections.namedtuple("Entry", "name family call expected check norm reads_mark sets_mark")


# ---- the states ------------------------------------------------------------------------------------------------------

def plant_unmeasured(st, radius_2048=True):
    """One member's state dict with the six unmeasured bots of UNMEASURED (five without the radius of 2048) written into
    copies of its arrays."""
    pos, vel, rad = st["pos"].copy(), st["vel"].copy(), st["rad"].copy()
    pos[10, 0] = np.nan
    pos[40, 1] = np.inf
    pos[77, 0] = -2048.0
    vel[123, 1] = 2048.0
    rad[200] = np.nan
    if radius_2048:
        rad[290] = 2048.0
    return dict(st, pos=pos, vel=vel, rad=rad)


def _batch_params(orc, k):
    # discs 0.15 apart overlap (two radii are 0.155 ... 0.235): under the default spring of 1000 the blob flies apart within
    # the 120 steps and leaves some forty links per member; a spring of 100 with a damping of 0.5 keeps it in contact
    return orc.default_params(nCells=300, nDead=0, seed=900 + k, max_time=1e9, phase_update_interval=0.3, spring=100.0,
                              damping=0.5, display_shadow=0, centroid_steps=16, centroid_int=0.1)


def _batch_start(k):
    rng = np.random.default_rng(5000 + k)
    pos, vel, rad = jittered_blob(300, 0.15, rng, center=(0.4 * k, -0.3 * k), jitter=0.3)
    phase = rng.uniform(0.0, 6.28, 300).astype(f32)
    dead = (rng.random(300) < 0.1).astype(np.int32) if k == 1 else np.zeros(300, np.int32)
    return dict(pos=pos, vel=vel, rad=rad, phase=phase, dead=dead)


def _oracle_run(orc, P, start):
    """The oracle's member after 90 and after 120 steps: (state at the mark, its fp32 time, final state, final time)."""
    osim = orc.Sim(P, reset=False)
    for key in ("pos", "vel", "rad", "phase", "dead"):
        osim.set(key, start[key])
    keys = ("pos", "vel", "rad", "phase", "dead")
    assert osim.run(STEPS - STEPS_AFTER_MARK, dt=DT, sort_interval=SORT_INTERVAL)
    at_mark, mark_time = {k: osim.get(k) for k in keys}, float(osim.time)
    assert osim.run(STEPS_AFTER_MARK, dt=DT, sort_interval=SORT_INTERVAL)
    final, time = {k: osim.get(k) for k in keys}, float(osim.time)
    osim.close()
    return at_mark, mark_time, final, time


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def state(name):
    """The named state, computed once on the CPU and shared read-only."""
    from oracle import orclib as orc
    if name in ("batch3x300", "batch3x300_small_radii"):
        params = [_batch_params(orc, k) for k in range(3)]
        start = [_batch_start(k) for k in range(3)]
        runs = [_oracle_run(orc, P, s) for P, s in zip(params, start)]
        assert len({r[1] for r in runs}) == 1 and len({r[3] for r in runs}) == 1
        final = [r[2] for r in runs]
        final[1] = plant_unmeasured(final[1], name == "batch3x300")
        return State(name, 3, 300, params, 0.0, [_frozen(s) for s in start], [_frozen(r[0]) for r in runs], runs[0][1],
                     [_frozen(s) for s in final], runs[0][3], dict(center=(0.4, -0.3), half=(1.5, 1.2), render_half=2.5))
    if name == "single17":
        rng = np.random.default_rng(2017)
        pos, vel, rad = jittered_blob(17, 0.15, rng, jitter=0.3)
        P = orc.default_params(nCells=17, nDead=0, seed=3, max_time=1e9, display_shadow=0, centroid_steps=16,
                               centroid_int=0.1)
        rest = dict(vel=vel, rad=rad, phase=np.zeros(17, f32), dead=np.zeros(17, np.int32))
        at_mark = dict(rest, pos=pos)
        final = dict(rest, pos=YR.perturbed(pos, rng, shift=0.05))
        return State(name, 1, 17, [P], 4.0e6, [_frozen(dict(at_mark))], [_frozen(at_mark)], 0.0, [_frozen(final)], 0.0,
                     dict(center=(0.05, 0.05), half=(0.3, 0.25), render_half=0.5))
    raise KeyError(name)


def state_of(sim, member):
    return sim.get_state_of(member) if hasattr(sim, "nsims") else sim.get_state()


def bring(pb, st, mark=True):
    """A fresh session on the device brought to the state by its recipe (pb: the package)."""
    sps = [simparams_from_orc(P) for P in st.params]
    if st.nsims == 3:
        sim = pb.Ensemble([sp for sp, _ in sps], wall_half=st.wall_half, keepalive=[k for _, k in sps])
        for k, s in enumerate(st.start):
            sim.set_state_of(k, **s)
        assert sim.step(STEPS - STEPS_AFTER_MARK, dt=DT, sort_interval=SORT_INTERVAL) == STEPS - STEPS_AFTER_MARK
        if mark:
            sim.mark_reference(MARKS["A"])
        assert sim.step(STEPS_AFTER_MARK, dt=DT, sort_interval=SORT_INTERVAL) == STEPS_AFTER_MARK
        planted = plant_unmeasured(sim.get_state_of(1), st.name == "batch3x300")
        sim.set_state_of(1, pos=planted["pos"], vel=planted["vel"], rad=planted["rad"])
        return sim
    sim = pb.Sim(sps[0][0], wall_half=st.wall_half, keepalive=sps[0][1])
    sim.set_state(**st.at_mark[0])
    if mark:
        sim.mark_reference(MARKS["A"])
    sim.set_state(pos=st.final[0]["pos"])
    return sim


def mark_of(st, key):
    """(positions, radii per member, gap, fp32 time) of the mark `key` of MARKS."""
    src, t = (st.at_mark, st.mark_time) if key == "A" else (st.final, st.time)
    return [s["pos"] for s in src], [s["rad"] for s in src], MARKS[key], t


def members_of(st):
    """(first, last, the member with the dead and the unmeasured bots)"""
    return (0, 2, 1) if st.nsims == 3 else (0, 0, 0)


# ---- comparisons -----------------------------------------------------------------------------------------------------

def same_bits(a, b):
    """a and b are the same result: arrays byte for byte with dtype and shape, floats by their bits, the rest by =="""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and a.tobytes() == b.tobytes())
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return isinstance(b, float) and struct.pack("<d", a) == struct.pack("<d", b)
    if isinstance(a, complex):
        return isinstance(b, complex) and same_bits(a.real, b.real) and same_bits(a.imag, b.imag)
    return type(a) is type(b) and a == b


def same_floats(got, want):
    """test_gpu_contacts.assert_same_floats: bit for bit where the reference is finite, non-finite where it is not."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    fin = np.isfinite(want)
    assert not np.isfinite(got[~fin]).any(), "finite where the reference is not"
    as_int = np.uint32 if got.dtype == np.float32 else np.uint64
    a, b = got[fin].view(as_int), want[fin].view(as_int)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (bad.size, a.size, got[fin][bad[:3]], want[fin][bad[:3]])


def nan_aware_bits(got, want):
    """fp32 arrays: bit for bit where the reference is no NaN, NaN where it is (test_gpu_dynamics.check's rule)."""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def psi_bits(psi):
    return np.ascontiguousarray(psi).view(np.float64).reshape(-1, 2).view(np.uint64)


def ints_equal(got, want):
    assert np.array_equal(np.asarray(got), np.asarray(want)), np.flatnonzero(np.asarray(got) != np.asarray(want))[:8]


def equal(got, want):
    assert got == want, (got, want)


# ---- restatements this file adds --------------------------------------------------------------------------------------

def centroid_restated(pos):
    """pbSimCentroids' float64 mean of one member, addition for addition: workgroups of 256 lanes reduce their bots by
    halving (lane t += lane t + w for w = 128 ... 1, zeros past the end), lane k of one wave adds the workgroups' sums
    k, k + 64, ... in order, the 64 lanes combine by the butterfly v[i] += v[i ^ d] for d = 32 ... 1, and lane 0's sum
    is divided by n."""
    pos = np.asarray(pos, f32).reshape(-1, 2)
    n = pos.shape[0]
    blocks = -(-n // 256)
    v = np.zeros((blocks * 256, 2), np.float64)
    v[:n] = pos.astype(np.float64)
    v = v.reshape(blocks, 256, 2)
    w = 128
    with np.errstate(all="ignore"):
        while w >= 1:
            v[:, :w] = v[:, :w] + v[:, w:2 * w]
            w //= 2
        lanes = np.zeros((64, 2), np.float64)
        for b in range(blocks):
            lanes[b % 64] = lanes[b % 64] + v[b, 0]
        d = 32
        while d >= 1:
            lanes = lanes + lanes[np.arange(64) ^ d]
            d //= 2
        out = lanes[0] / np.float64(n)
    return float(out[0]), float(out[1])


def sk_vectors(count):
    """`count` wavevectors as test_gpu_sfactor draws them; the last one has work of its own."""
    v = np.random.default_rng(5200 + count).integers(-70, 71, (count, 2)).tolist()
    v[-1] = [-3, 2]
    return v


def render_view(st, shape):
    return (shape[0], shape[1], st.view["center"], st.view["render_half"])


# ---- the catalogue ---------------------------------------------------------------------------------------------------

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _clusters(st, gap):
    return _cached((st.name, "clusters", gap), lambda: [CR.analyse(s["pos"], s["rad"], gap) for s in st.final])


def _network(st, gap, m):
    s = st.final[m]
    from oracle import orclib as orc
    return _cached((st.name, "network", gap, m),
                   lambda: NR.network(orc, st.params[m], s["pos"], s["vel"], s["rad"], gap))


def _hexatic(st, gap):
    return _cached((st.name, "hexatic", gap), lambda: [SR.analyse(s["pos"], s["rad"], gap) for s in st.final])


def _rearrangement(st, key):
    pos0, rad0, gap, _ = mark_of(st, key)
    return _cached((st.name, "rearrangement", key),
                   lambda: [YR.analyse(pos0[m], rad0[m], s["pos"], s["rad"], gap) for m, s in enumerate(st.final)])


def catalogue(st):
    """The named calls, in the order `catalogue` runs them.  call(sim) makes the call; expected(mark) is what the
    restatement gives for the state under the mark named (only entries with reads_mark look at it); check(got, want)
    compares the two the way the owning test file does; norm(got) drops what is no part of the answer."""
    from particlerobotsimulations_amd import _capi
    first, last, odd = members_of(st)
    view = dict(center=st.view["center"], half=st.view["half"])
    E = []

    def add(name, family, call, expected, check, norm=None, reads_mark=False, sets_mark=None):
        E.append(Entry(name, family, call, expected, check, norm or (lambda got: got), reads_mark, sets_mark))

    def strip_rounds(rows):  # the rounds the forest took to settle are no part of the answer
        return [{k: r[k] for k in CR.FIELDS} for r in rows]

    def check_contacts(got, want):
        assert got["offsets"].dtype == np.uint32 and got["other"].dtype == np.uint32
        ints_equal(got["offsets"], want["offsets"])
        ints_equal(got["other"], want["other"])
        same_floats(got["gap"], want["gap"])
        assert np.array_equal(got["gap"].view(np.uint32), want["gap"].view(np.uint32))
        same_floats(got["force"], want["force"])

    def check_structure(got, want):
        keys = ("bonds", "psi6_re", "psi6_im", "coordination")
        assert [{k: r[k] for k in keys} for r in got] == want, (got, want)

    def check_hexatic(got, want):
        assert got[0].dtype == np.complex128 and got[1].dtype == np.uint32
        ints_equal(got[1], want[1])
        assert np.array_equal(psi_bits(got[0]), psi_bits(want[0]))

    def check_labels(got, want):
        ints_equal(got[0], want[0])
        ints_equal(got[1], want[1])

    for gap in GAPS:
        add(f"clusters({gap})", "clusters", lambda sim, gap=gap: sim.clusters(gap),
            lambda mark, gap=gap: [c[0] for c in _clusters(st, gap)], equal, norm=strip_rounds)
    for gap, m in ((GAPS[0], first), (GAPS[1], last), (GAPS[2], first), (GAPS[2], last)):
        add(f"cluster_labels({gap}, member {m})", "clusters", lambda sim, gap=gap, m=m: sim.cluster_labels(gap, member=m),
            lambda mark, gap=gap, m=m: _clusters(st, gap)[m][1:], check_labels)
    for gap in GAPS:
        add(f"contacts({gap}, member {odd})", "contacts", lambda sim, gap=gap: sim.contacts(gap, member=odd),
            lambda mark, gap=gap: _network(st, gap, odd), check_contacts)
    for gap in GAPS:
        add(f"contact_virial({gap}, member {odd})", "contacts", lambda sim, gap=gap: sim.contact_virial(gap, member=odd),
            lambda mark, gap=gap: _network(st, gap, odd)["virial"], same_floats)
    for gap in GAPS:
        add(f"structure({gap})", "hexatic", lambda sim, gap=gap: sim.structure(gap),
            lambda mark, gap=gap: [h[0] for h in _hexatic(st, gap)], check_structure)
    for gap in GAPS:
        add(f"hexatic({gap}, member {last})", "hexatic", lambda sim, gap=gap: sim.hexatic(gap, member=last),
            lambda mark, gap=gap: _hexatic(st, gap)[last][1:], check_hexatic)

    def want_radial(r_max, bins):
        return np.stack([SR.radial_counts(s["pos"], s["rad"], r_max, bins) for s in st.final])

    def check_radial(got, want):
        assert got.dtype == np.uint64 and got.shape == want.shape
        ints_equal(got, want)
        assert not (got & np.uint64(1)).any()

    for r_max, bins in RADIAL:
        add(f"radial_counts({r_max}, {bins})", "radial", lambda sim, r=r_max, b=bins: sim.radial_counts(r, b),
            lambda mark, r=r_max, b=bins: want_radial(r, b), check_radial)

    def want_correlation(kind, r_max, bins, mark):
        pos0 = mark_of(st, mark)[0] if kind == "displacement" else [None] * st.nsims
        refs = [KR.pair_correlation(kind, s["pos"], s["vel"], s["rad"], r_max, bins, pos0[m])
                for m, s in enumerate(st.final)]
        return [KR.rows_of(r, _capi.CORRELATION_BIN_DTYPE) for r in refs], [r["totals"] for r in refs]

    def check_correlation(got, want):
        rows, totals = got
        assert rows.dtype == _capi.CORRELATION_BIN_DTYPE and rows.shape == (st.nsims, len(want[0][0]))
        for m in range(st.nsims):
            assert rows[m].tobytes() == want[0][m].tobytes(), (m, np.flatnonzero(rows[m] != want[0][m])[:8])
            assert totals[m] == want[1][m], (m, totals[m], want[1][m])
        assert not (rows["pairs"] & np.uint64(1)).any()

    for kind in ("velocity", "radius", "displacement"):
        for r_max, bins in CORRELATION:
            add(f"pair_correlation({kind}, {r_max}, {bins})", "correlation",
                lambda sim, k=kind, r=r_max, b=bins: sim.pair_correlation(k, r, b),
                lambda mark, k=kind, r=r_max, b=bins: want_correlation(k, r, b, mark), check_correlation,
                reads_mark=kind == "displacement")

    def want_field(nx, ny, members):
        return [FR.field_map(st.final[m]["pos"], st.final[m]["vel"], st.final[m]["rad"], st.final[m]["dead"], nx=nx, ny=ny,
                             **view) for m in members]

    def check_field_batch(got, want):
        cells, totals = got
        assert cells.dtype.itemsize == 64 and cells.shape[0] == len(want) == len(totals)
        for m, (want_cells, want_tot) in enumerate(want):
            assert totals[m] == want_tot, (m, totals[m], want_tot)
            assert FR.from_device(cells[m]) == want_cells, m

    def check_field_of(got, want):
        check_field_batch((got[0][None], [got[1]]), want)

    for nx, ny in FIELD_SHAPES:
        add(f"field_map({nx}x{ny})", "field",
            lambda sim, nx=nx, ny=ny: sim.field_map(nx, ny, view["center"], view["half"]),
            lambda mark, nx=nx, ny=ny: want_field(nx, ny, range(st.nsims)), check_field_batch)
        add(f"field_map({nx}x{ny}, member {odd})", "field",
            lambda sim, nx=nx, ny=ny: sim.field_map(nx, ny, view["center"], view["half"], member=odd),
            lambda mark, nx=nx, ny=ny: want_field(nx, ny, [odd]), check_field_of)

    def want_sk(count, kind, members):
        vectors = sk_vectors(count)
        return [QR.structure_factor(st.final[m]["pos"], st.final[m]["vel"], st.final[m]["rad"], vectors, SK_BOX, kind)
                for m in members]

    def check_sk(got, want):
        rows = got if got.ndim == 2 else got[None]
        assert rows.dtype.itemsize == 80 and rows.shape == (len(want), len(want[0])) and not rows["reserved"].any()
        for m, w in enumerate(want):
            assert QR.from_device(rows[m]) == w, m

    for count, kind, one in ((1, "density", False), (SK_MOST, "velocity", False), (3, "density", True),
                             (SK_MOST, "density", True), (3, "velocity", False), (1, "velocity", True)):
        if one:
            add(f"structure_factor({count} vectors, {kind}, member {last})", "sfactor",
                lambda sim, c=count, k=kind: sim.structure_factor(sk_vectors(c), SK_BOX, kind=k, member=last),
                lambda mark, c=count, k=kind: want_sk(c, k, [last]), check_sk)
        else:
            add(f"structure_factor({count} vectors, {kind})", "sfactor",
                lambda sim, c=count, k=kind: sim.structure_factor(sk_vectors(c), SK_BOX, kind=k),
                lambda mark, c=count, k=kind: want_sk(c, k, range(st.nsims)), check_sk)

    def check_moments(got, want):
        assert [{k: row[k] for k in MR.FIELDS} for row in got] == want

    add("moments()", "moments", lambda sim: sim.moments(),
        lambda mark: [MR.moments(s["pos"], s["vel"], s["rad"]) for s in st.final], check_moments)

    def want_colours():
        s, P = st.final[odd], st.params[odd]
        with np.errstate(all="ignore"):
            return DR.colours(s["rad"], s["dead"], np.zeros(st.n, bool), P.min_radius, P.max_radius, 0)

    add(f"colors(member {odd})", "display", lambda sim: sim.colors(odd), lambda mark: want_colours(), nan_aware_bits)

    def check_centroid(got, want):
        assert same_bits(tuple(got), tuple(want)), (got, want)

    add("centroid()", "display", lambda sim: sim.centroid(), lambda mark: centroid_restated(st.final[0]["pos"]),
        check_centroid)

    def want_frame(shape):
        s = st.final[odd]
        with np.errstate(all="ignore"):
            return RR.render(RR.scene_from(st.params[odd], light_radius=0.25), RR.View(*render_view(st, shape)), s["pos"],
                             s["rad"], s["dead"])

    def check_frame(got, want):
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:8]

    for shape in RENDER_SHAPES:
        add(f"render({shape[0]}x{shape[1]}, member {odd})", "render",
            lambda sim, shape=shape: sim.render(*render_view(st, shape), light_radius=0.25, member=odd),
            lambda mark, shape=shape: want_frame(shape), check_frame)

    # the mark: three reads of whichever mark the order has put in place, and two compound entries that replace it
    def check_rearrangement_of(got, want):
        assert got["disp"].dtype == f32
        for k in ("marked", "now", "kept"):
            assert got[k].dtype == np.uint32
            ints_equal(got[k], want[k])
        fin = np.isfinite(want["disp"])
        assert np.array_equal(got["disp"].view(np.uint32)[fin], want["disp"].view(np.uint32)[fin])
        assert np.array_equal(np.isnan(got["disp"])[~fin], np.isnan(want["disp"])[~fin])
        assert np.array_equal(np.isfinite(got["disp"]), fin)

    def want_info(mark):
        _, _, gap, t = mark_of(st, mark)
        return {"marked": True, "gap": float(f32(gap)), "time": float(f32(t)),
                "entries": sum(r[0]["bonds_marked"] for r in _rearrangement(st, mark))}

    add("rearrangement()", "mark", lambda sim: sim.rearrangement(),
        lambda mark: [r[0] for r in _rearrangement(st, mark)], equal, reads_mark=True)
    add(f"rearrangement_of(member {odd})", "mark", lambda sim: sim.rearrangement_of(odd),
        lambda mark: _rearrangement(st, mark)[odd][1], check_rearrangement_of, reads_mark=True)
    add("reference_info()", "mark", lambda sim: sim.reference_info(), want_info, equal, reads_mark=True)

    def mark_then_compare(sim, key):
        sim.mark_reference(MARKS[key])
        return sim.rearrangement()

    for key in ("B", "C"):
        add(f"mark_reference({MARKS[key]}) + rearrangement()", "mark", lambda sim, key=key: mark_then_compare(sim, key),
            lambda mark: [r[0] for r in _rearrangement(st, mark)], equal, reads_mark=True, sets_mark=key)
    names = [e.name for e in E]
    return E if len(set(names)) == len(names) else _renamed(E)


def _renamed(entries):
    """On a batch of one, two entries may name the same call: tell them apart by their place."""
    seen, out = collections.Counter(), []
    for e in entries:
        seen[e.name] += 1
        out.append(e if seen[e.name] == 1 else e._replace(name=f"{e.name} #{seen[e.name]}"))
    return out


# ---- the orders ------------------------------------------------------------------------------------------------------

def orders(st):
    """name -> list of catalogue indices: the catalogue as written, reversed, and four shuffles in each of which every
    entry appears twice."""
    count = len(catalogue(st))
    out = {"catalogue": list(range(count)), "reversed": list(range(count))[::-1]}
    for k in range(4):
        out[f"shuffle{k}"] = [int(i) for i in np.random.default_rng(7000 + k).permutation(list(range(count)) * 2)]
    assert tuple(out) == ORDERS
    return out


def walk(st, order, mark="A"):
    """(entry, the mark its result is expected under) along an order that starts with `mark` in place."""
    entries = catalogue(st)
    for i in order:
        e = entries[i]
        if e.sets_mark:
            mark = e.sets_mark
        yield e, mark


def expected(st, entry, mark):
    """The entry's expectation, computed once per (state, entry, mark it reads)."""
    return _cached((st.name, "expected", entry.name, mark if entry.reads_mark else None), lambda: entry.expected(mark))


def needed(st):
    """Every (catalogue index, mark) that occurs in one of the orders: what the fresh sessions have to answer."""
    entries = catalogue(st)
    index = {e.name: i for i, e in enumerate(entries)}
    out = set()
    for order in orders(st).values():
        for e, mark in walk(st, order):
            out.add((index[e.name], mark if e.reads_mark else None))
    for key in MARKS:  # a session that lost its mark and took a new one (the refused-call test)
        for i, e in enumerate(entries):
            if e.reads_mark and not e.sets_mark and key != "A":
                out.add((i, key))
    return sorted(out, key=lambda p: (p[0], p[1] or ""))


# ---- preconditions ---------------------------------------------------------------------------------------------------

# every buffer that ensure() only grows, with the catalogue's call that needs the most of it and the one that needs the
# least: the links of member `odd` grow with the gap, the histograms with the bins, the marked network with the mark's
# gap, the private buffers of the field maps, structure factors and frames with the cells, vectors and pixels
def growing_buffers(st):
    _, last, odd = members_of(st)
    return {
        "cLinks": (f"contacts({GAPS[2]}, member {odd})", f"contacts({GAPS[0]}, member {odd})"),
        "sCounts": ("radial_counts(3.0, 4096)", "radial_counts(0.25, 1)"),
        "kAcc": ("pair_correlation(velocity, 3.0, 1024)", "pair_correlation(radius, 0.25, 1)"),
        "dOther": (f"mark_reference({MARKS['B']}) + rearrangement()", f"mark_reference({MARKS['C']}) + rearrangement()"),
        "field cells": ("field_map(64x48)", f"field_map(1x1, member {odd})"),
        "structure factor rows": (f"structure_factor({SK_MOST} vectors, velocity)",
                                  f"structure_factor(1 vectors, velocity, member {last})"),
        "frame": (f"render(64x48, member {odd})", f"render(5x3, member {odd})"),
    }


def check_orders(st):
    """From the orders alone: every grow-then-shrink, both switches of the filing kind and the long-lived mark occur."""
    entries = catalogue(st)
    names = [e.name for e in entries]
    assert len(set(names)) == len(names)
    all_orders = orders(st)
    assert all_orders["reversed"] == all_orders["catalogue"][::-1]
    for k in range(4):
        assert sorted(all_orders[f"shuffle{k}"]) == sorted(all_orders["catalogue"] * 2)
    assert len({tuple(o) for o in all_orders.values()}) == len(ORDERS)
    placed = [[names[i] for i in order] for order in all_orders.values()]
    for buffer, (largest, smallest) in growing_buffers(st).items():
        assert largest in names and smallest in names, buffer
        assert any(max(k for k, nm in enumerate(p) if nm == smallest) > min(k for k, nm in enumerate(p) if nm == largest)
                   for p in placed), f"{buffer}: its smallest call never runs after its largest"
    # the filing kind: radial counts and pair correlations file with perRmax = 0, the link rule's callers with 2
    plain, linked = {"radial", "correlation"}, {"clusters", "contacts", "hexatic", "mark"}
    family = {e.name: e.family for e in entries}
    pairs = {(family[a], family[b]) for p in placed for a, b in zip(p, p[1:])}
    assert any(a in plain and b in linked for a, b in pairs), "no link-rule call directly behind a plain filing"
    assert any(a in linked and b in plain for a, b in pairs), "no plain filing directly behind a link-rule call"
    # a read of the mark behind five other families' re-filings since the mark was put in place
    best = 0
    for order in all_orders.values():
        since = set()
        for e, _ in walk(st, order):
            if e.sets_mark:
                since = set()
            elif e.reads_mark:
                best = max(best, len(since))
            if e.family in FILING:
                since.add(e.family)
    assert best >= 5, f"the mark is never read behind more than {best} other families"
    return len(entries)


def check_not_trivial(st):
    """The expectations say something on these states."""
    _, _, odd = members_of(st)
    for m, c in enumerate(_clusters(st, GAPS[2])):
        assert c[0]["links"] >= st.n, (m, c[0])
    for m, s in enumerate(st.final):
        counts = SR.radial_counts(s["pos"], s["rad"], *RADIAL[0])
        assert (counts > 0).sum() >= 3, (m, counts)
    for m, (row, _) in enumerate(_rearrangement(st, "A")):
        assert row["bots_lost"] + row["bots_gained"] > 0 and row["measured"] > 0, (m, row)
    s = st.final[odd]
    for nx, ny in FIELD_SHAPES:
        _, tot = FR.field_map(s["pos"], s["vel"], s["rad"], s["dead"], nx=nx, ny=ny, center=st.view["center"],
                              half=st.view["half"])
        assert tot["inside"] > 0 and tot["outside"] > 0, (nx, ny, tot)
    if st.nsims == 3:
        assert tot["unmeasured"] == len(UNMEASURED) - (st.name != "batch3x300") and int(s["dead"].sum()) >= 20
        # the link rule's grid edge, (2 rmax + gap) (1 + 2^-10): one cell for everything, or cells of a bot's diameter
        rmax = max(float(np.nanmax(np.where(np.isfinite(f["rad"]), f["rad"], 0.0))) for f in st.final)
        assert rmax == 2048.0 if st.name == "batch3x300" else rmax < 0.12
