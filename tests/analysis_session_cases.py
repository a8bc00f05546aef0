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

The strain family (strain() at three thresholds, strain_of() per member) files nothing: it reads the CSR and the
positions of whichever mark is in place, shares pbDynamicsScatter with the rearrangement compare and keeps its rows in
the shared scratch.  Its expectations come from tests/strain_ref.py on the marked network restated once per mark; the
mark is the earlier state for A and the state itself for B and C, where every fitted bot's gradient is the identity and
its d2min exactly 0 (check_strain_not_trivial says what the rows hold there).  check_orders asks for a strain call
directly behind every family that re-files, behind an entry that replaces the mark, behind a compare and behind a
displacement correlation, and for a compare directly behind a strain call.

The recorders' shapes are here as well: RECORD_BETWEEN, the distinct van Hove records the GPU file takes between every
two calls (a filing at rMax = 1 with no radius term: check_record_grid shows that no call of the catalogue files on that
grid), and the two van Hove functions of the interleaving test, the self part's width chosen from the oracle's
displacements over one lag (van_hove_self_width, check_van_hove_self_width).

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
import strain_ref as ER
import structure_ref as SR
import vanhove_distinct_ref as GR
import vanhove_ref as VR
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
SHUFFLES = 4
ORDERS = ("catalogue", "reversed") + tuple(f"shuffle{k}" for k in range(SHUFFLES))
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


def _marked_network(st, key, m):
    pos0, rad0, gap, _ = mark_of(st, key)
    return _cached((st.name, "marked network", key, m), lambda: NR.topology(pos0[m], rad0[m], gap))


def _strain(st, key, threshold):
    """strain_ref's (row, per-bot arrays) of every member: the mark `key` against the state as it is."""
    pos0 = mark_of(st, key)[0]

    def one(m):
        off, _, oth = _marked_network(st, key, m)
        return ER.analyse_csr(off, oth, pos0[m], st.final[m]["pos"], threshold)

    return _cached((st.name, "strain", key, threshold), lambda: [one(m) for m in range(st.nsims)])


@functools.lru_cache(maxsize=None)
def strain_thresholds():
    """(0, the median of the reference's d2min over the fitted bots of batch3x300 under mark A in world units, rounded to
    fp32 as the call takes it, 1e30 that no bot exceeds): the same three on every state."""
    bots = [b for _, b in _strain(state("batch3x300"), "A", 0.0)]
    d2 = np.concatenate([b["d2min"][b["fitted"]] for b in bots])
    return 0.0, float(f32(np.median(d2) / 2.0 ** 40)), 1.0e30


def nan_aware_bits64(got, want):
    """float64 arrays as test_gpu_strain compares them, by their bits; a NaN of the reference asks for a NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = np.flatnonzero(got.view(np.uint64)[~nan] != want.view(np.uint64)[~nan])
    assert bad.size == 0, (bad.size, bad[:8])


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

    # the strain analysis files nothing: it reads the CSR and the positions of whichever mark the order has put in place
    def check_strain(got, want):
        assert len(got) == st.nsims and all(tuple(row) == ER.FIELDS for row in got)
        assert got == want, [{k: (g[k], w[k]) for k in g if g[k] != w[k]} for g, w in zip(got, want)]

    def check_strain_of(got, want):
        assert got["moments"].dtype == np.int64 and got["moments"].shape == (st.n, 9)
        assert got["gradient"].shape == (st.n, 2, 2) and got["d2min"].shape == (st.n,)
        ints_equal(got["moments"], want["moments"])
        nan_aware_bits64(got["d2min"], want["d2min"])
        nan_aware_bits64(got["gradient"], want["gradient"])
        _, grad, d2 = ER.fit_all(got["moments"])  # the device's d2min is the fit of the device's own moments
        nan_aware_bits64(got["d2min"], d2)
        nan_aware_bits64(got["gradient"], grad)

    for threshold in strain_thresholds():
        add(f"strain({threshold!r})", "strain", lambda sim, t=threshold: sim.strain(t),
            lambda mark, t=threshold: [r[0] for r in _strain(st, mark, t)], check_strain, reads_mark=True)
    for m in (first, last, odd):
        add(f"strain_of(member {m})", "strain", lambda sim, m=m: sim.strain_of(m),
            lambda mark, m=m: _strain(st, mark, 0.0)[m][1], check_strain_of, reads_mark=True)

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
    """name -> list of catalogue indices: the catalogue as written, reversed, and SHUFFLES shuffles in each of which
    every entry appears twice."""
    count = len(catalogue(st))
    out = {"catalogue": list(range(count)), "reversed": list(range(count))[::-1]}
    for k in range(SHUFFLES):
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
    for k in range(SHUFFLES):
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
    # (by the link rule's readers and the displacement correlation, and by the strain analysis, each on its own)
    best = {False: 0, True: 0}
    for order in all_orders.values():
        since = set()
        for e, _ in walk(st, order):
            if e.sets_mark:
                since = set()
            elif e.reads_mark:
                best[e.family == "strain"] = max(best[e.family == "strain"], len(since))
            if e.family in FILING:
                since.add(e.family)
    assert best[False] >= 5, f"the mark is never read behind more than {best[False]} other families"
    assert best[True] >= 5, f"no strain call reads the mark behind more than {best[True]} other families"
    # the strain analysis reads the mark's buffers and shares a kernel and the scratch with the rest: a strain call
    # directly behind every family that re-files, behind an entry that replaces the mark (and may move dOther), behind a
    # rearrangement compare and behind a correlation that reads the marked positions; and a compare behind a strain call
    by_name = {e.name: e for e in entries}
    behind = {(by_name[a], by_name[b]) for p in placed for a, b in zip(p, p[1:])}
    strain_behind = [a for a, b in behind if b.family == "strain"]
    for fam in FILING:
        assert any(a.family == fam for a in strain_behind), f"no strain call directly behind a call of {fam}"
    assert any(a.sets_mark for a in strain_behind), "no strain call directly behind an entry that replaces the mark"
    assert any(is_compare(a) for a in strain_behind), "no strain call directly behind a rearrangement read"
    assert any(a.family == "correlation" and a.reads_mark for a in strain_behind), \
        "no strain call directly behind a correlation that reads the mark"
    assert any(a.family == "strain" and is_compare(b) for a, b in behind), "no rearrangement read directly behind a strain call"
    return len(entries)


def is_compare(entry):
    """rearrangement() or rearrangement_of() on the mark in place (not reference_info(), which asks the host alone)."""
    return entry.family == "mark" and not entry.sets_mark and entry.name.startswith("rearrangement")


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
        check_strain_not_trivial(st)


def check_strain_not_trivial(st):
    """The strain rows of a batch state, from strain_ref alone.  Under mark A (90 steps against 120) bots are fitted and
    their d2min is positive; under marks B and C the marked state IS the present one, so every fitted bot has the
    identity for a gradient and a d2min of exactly 0 (test_gpu_strain asserts the same of a state against itself): there
    the moments, the fitted bots and the bonds are what the rows say.  single17 (17 bots moved by noise of 0.03, no pure
    translation) has 13 fitted bots under mark A; nothing is asserted of it here."""
    _, middle, huge = strain_thresholds()
    for key in MARKS:
        for m, (row, bots) in enumerate(_strain(st, key, 0.0)):
            assert row["fitted"] > 0 and row["unfitted"] > 0 and row["bonds_used"] > 0 and row["w"] > 0, (key, m, row)
            assert (row["max_d2"] > 0 and row["sum_d2"] > row["max_d2"]) if key == "A" else row["max_d2"] == 0, (key, m, row)
            assert (bots["gradient"][bots["fitted"]] == np.eye(2)).all() == (key != "A"), (key, m)
    for m, (row, _) in enumerate(_strain(st, "A", middle)):
        assert 0 < row["above"] < row["fitted"], (m, row)
    assert all(row["above"] == 0 for row, _ in _strain(st, "A", huge))
    # the planted bots had bonds at step 90; a NaN, an infinite or a far-away component now fails pbStrainInReach
    odd = _strain(st, "A", 0.0)[1]
    assert odd[0]["unfitted"] > 0 and odd[0]["bonds_dropped"] > 0
    length = np.diff(np.asarray(_marked_network(st, "A", 1)[0]).astype(np.int64))
    # (bot 10 had no bond at step 90; the bots at inf y and at x = -2048 had five and four, dropped at both ends)
    gone = (10, 40, 77)
    for bot in gone:
        assert odd[1]["dropped"][bot] == length[bot] and not odd[1]["fitted"][bot], bot
    assert length[40] > 0 and length[77] > 0 and odd[0]["bonds_dropped"] == 2 * sum(int(length[b]) for b in gone)


# ---- the recorders that run between and beside the calls -------------------------------------------------------------

RECORD_BETWEEN = (2, 1.0 / 32, 32)  # (lags, width, bins) of the distinct van Hove records taken between two calls
VAN_HOVE_LAGS, VAN_HOVE_INTERVAL, VAN_HOVE_BINS = 4, 0.05, 16  # the two recorders of the interleaving test
VAN_HOVE_DISTINCT = (1.0 / 32, 32)


def filing_edges(st):
    """The edge of every grid a call of the catalogue files the state on (pbClusterFile): (2 rmax + gap) (1 + 2^-10)
    for the link rule's callers, rmax the largest finite radius of the batch as it is; rMax (1 + 2^-10) for the radial
    counts and the pair correlations."""
    rmax = max(float(np.max(np.where(np.isfinite(s["rad"]), s["rad"], f32(0.0)))) for s in st.final)
    grow = 1.0 + 1.0 / 1024.0
    gaps = sorted(set(GAPS) | set(MARKS.values()))
    return ([(2.0 * rmax + float(f32(gap))) * grow for gap in gaps]
            + [max(float(f32(r)) * grow, 1.0 / 256.0) for r, _ in RADIAL + CORRELATION])


def check_record_grid(st):
    """The records between the calls file on a grid no call of the catalogue files on: rMax = 1, an edge a tenth away
    from every other at the least, so that a sweep which kept the grid of the record in front of it walks other cells."""
    lags, width, bins = RECORD_BETWEEN
    edge, gx, gy = GR.grid_of(st.n, width, bins)
    assert VR.qw_of(width) * bins == 1 << 20 and edge == 1.0 + 1.0 / 1024.0
    assert (gx, gy) == ((32, 16) if st.n == 300 else (8, 4))
    others = filing_edges(st)
    assert len(others) == len(set(GAPS) | set(MARKS.values())) + len(RADIAL) + len(CORRELATION)
    assert all(abs(e / edge - 1.0) > 0.1 for e in others), (edge, others)
    return edge, others


@functools.lru_cache(maxsize=None)
def oracle_lagged_positions():
    """batch3x300's members run on by the oracle (nothing planted), their positions at 0, 5, 10 and 15 steps behind the
    state: records 0.05 s apart as the interleaving test's gate takes them."""
    from oracle import orclib as orc
    st = state("batch3x300")
    out = []
    for P, start in zip(st.params, st.start):
        osim = orc.Sim(P, reset=False)
        for key in ("pos", "vel", "rad", "phase", "dead"):
            osim.set(key, start[key])
        assert osim.run(STEPS, dt=DT, sort_interval=SORT_INTERVAL)
        pos = [osim.get("pos")]
        for _ in range(VAN_HOVE_LAGS - 1):
            assert osim.run(5, dt=DT, sort_interval=SORT_INTERVAL)
            pos.append(osim.get("pos"))
        osim.close()
        out.append(pos)
    return out


@functools.lru_cache(maxsize=None)
def van_hove_self_width():
    """The self part's bin width in the interleaving test: static friction holds most bots where they are, so the width
    comes from those that move: the largest power of two not above the 90th percentile of the displacement over one
    lag of 0.05 s, all members of batch3x300 together."""
    moved = np.concatenate([np.linalg.norm((p[1] - p[0]).astype(np.float64), axis=1) for p in oracle_lagged_positions()])
    return float(2.0 ** np.floor(np.log2(np.percentile(moved, 90))))


def check_van_hove_self_width():
    """With that width lag 1 fills more than one bin and lag 3 does not fall beyond the last edge as a whole."""
    width = van_hove_self_width()
    assert 2.0 ** -12 <= width <= 2.0 ** -8, width
    for m, pos in enumerate(oracle_lagged_positions()):
        rows = VR.table(pos, [0, 5, 10, 15], VAN_HOVE_LAGS, width, VAN_HOVE_BINS)
        assert all(VR.identities_hold(r) for r in rows)
        assert sum(1 for c in rows[1]["radial"] if c) > 1 and sum(rows[1]["radial"][1:]) > 0, (m, rows[1])
        assert 0 < sum(rows[3]["radial"][1:]) and rows[3]["beyond_r"] < rows[3]["samples"], (m, rows[3])
    return width
