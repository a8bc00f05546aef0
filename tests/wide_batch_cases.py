"""The inputs of the wide-batch tests (tests/test_wide_batch_cases_ref.py on the CPU, tests/test_gpu_wide_batches.py and
tests/test_gpu_wide_recorders.py on the device): batches of hundreds of members, the expectation of every member from
the restatements the suite already has, and the preconditions that make a member mix-up change the answer.  Nothing here
touches a device: the states are built on the host and the expectations come from tests/*_ref.py.

The shapes.  `wide257x40` is 257 members of 40 bots: one member past the 256 lanes of the per-member row kernels'
workgroup, 8 x 8 analysis cells per member.  `wide1025x7` is 1025 members of 7 bots: one past 1024, the 4 x 4 minimum
grid, whose `start` array has 16 400 + 1 entries.  `<shape>_huge` is the same batch with one radius of 2048 in the last
member: the link grid is sized by the batch-wide largest finite radius, so every member folds into one cell.
`<shape>_finite` is the batch without plants, dead bots and empty members, for the recorders (what is planted would not
survive a step).

A member.  Member k is a jittered_blob from the seed SEED0 + k around its own centre (uniform in +-CENTRE_HALF, so that
the one shared field-map view has members inside, straddling and outside), its radii scaled towards min_radius by its
own factor, its own spring (SPRING0 + 3 k: the contact forces read the member's parameters), velocities and phases from
its seed.  Bot 4 is moved next to bot 3 (0.1 apart: below any two radii) and the last bot 0.6 away from the blob, so that
the member has a link and a bot without one whatever its seed drew.  The marked state is that one; the present state is
dynamics_ref.perturbed of it with the member's own shift, the pair and the outlier put in place again.

What is planted (the main states only).  Every third member has dead bots.  The members PLANTED_AT get the unmeasured
bots of analysis_session_cases.UNMEASURED without the radius of 2048, their indices scaled to n.  The members 128 and
the last hold no measured bot at all: every present position is NaN (the last one's marked positions too).

`chosen(shape)` is the eight members the per-member getters and the lone-Sim comparison run at."""
import collections
import functools

import numpy as np

import analysis_session_cases as AC
import cluster_ref as CR
import contacts_ref as NR
import correlation_ref as KR
import display_ref as DR
import dynamics_ref as YR
import field_ref as FR
import render_ref as RR
import series_ref as MR
import sfactor_ref as QR
import strain_ref as TR
import structure_ref as SR
from helpers import jittered_blob

f32 = np.float32
SHAPES = {"wide257x40": (257, 40), "wide1025x7": (1025, 7)}
MAIN = tuple(SHAPES)
HUGE = tuple(f"{name}_huge" for name in SHAPES)
ALL = MAIN + HUGE
FINITE = "wide257x40_finite"
SEED0, SPRING0 = 31000, 100.0
SPACING, JITTER = 0.19, 0.3
CENTRE_HALF = 3.5
PAIR, PAIR_OFFSET = (3, 4), (0.1, 0.02)
OUTLIER_OFFSET = (0.6, 0.45)
HUGE_BOT = 4                        # in the last member; no plant sits there
GAPS = (0.0, 0.0019, 0.05)
MARK_GAP = GAPS[1]
STRAIN_THRESHOLD = 0.0001
RADIAL = ((0.4, 7), (3.0, 4096))
CORRELATION = (0.4, 7)
KINDS = ("velocity", "radius", "displacement")
FIELD_SHAPES = ((8, 8), (1, 1))
VIEW = dict(center=(0.0, 0.0), half=(2.0, 1.8))
RENDER = (8, 8, (0.0, 0.0), 4.0)    # width, height, centre, half extent
SK_COUNT, SK_BOX, SK_KINDS = 3, AC.SK_BOX, ("density", "velocity")
SHUFFLE_SEED = 8128
SHIFTS = (1, 64, 256, 1024)         # the member strides a wrong offset would most likely be off by

Shape = collections.namedtuple("Shape", "name nsims n params wall_half marked final view")


def plants(n):
    """UNMEASURED's five plants without the radius of 2048, at indices scaled from 300 bots to n: bot -> what."""
    out = {int(round(i * n / 300.0)): what for i, what in AC.UNMEASURED.items() if what != "radius 2048"}
    # the linked pair and the outlier keep their positions and radii (a planted velocity does not touch the link rule)
    assert len(out) == 5 and all(what == "vy 2048" for bot, what in out.items() if bot in (PAIR[0], PAIR[1], n - 1)), out
    assert HUGE_BOT not in out
    return out


def planted_at(nsims):
    return tuple(m for m in (0, 63, 64, 255, 256, nsims - 1))


def empty_members(nsims):
    return (128, nsims - 1)


def chosen(st):
    """The eight members of the per-member calls: 0, both sides of the first wave's last lane, the empty member 128
    with both its neighbours, and the last two (255 and 256, or 1023 and 1024; the last one is empty too)."""
    return (0, 63, 64, 127, 128, 129, st.nsims - 2, st.nsims - 1)


def _plant(s, n):
    pos, vel, rad = s["pos"].copy(), s["vel"].copy(), s["rad"].copy()
    for bot, what in plants(n).items():
        if what == "nan x":
            pos[bot, 0] = np.nan
        elif what == "inf y":
            pos[bot, 1] = np.inf
        elif what == "x -2048":
            pos[bot, 0] = -2048.0
        elif what == "vy 2048":
            vel[bot, 1] = 2048.0
        else:
            assert what == "nan radius"
            rad[bot] = np.nan
    return dict(s, pos=pos, vel=vel, rad=rad)


def _in_place(pos):
    """The pair that is always linked and the bot that never is."""
    pos = pos.copy()
    pos[PAIR[1]] = pos[PAIR[0]] + np.asarray(PAIR_OFFSET, f32)
    pos[-1] = pos[:-1].max(axis=0) + np.asarray(OUTLIER_OFFSET, f32)
    return pos


def member_states(orc_params, k, n, nsims, kind):
    """(marked, present) of member k; kind: "main", "huge" or "finite"."""
    P = orc_params
    rng = np.random.default_rng(SEED0 + k)
    centre = rng.uniform(-CENTRE_HALF, CENTRE_HALF, 2)
    pos, vel, rad = jittered_blob(n, SPACING, rng, center=tuple(centre), jitter=JITTER, rmin=P.min_radius,
                                  rmax=P.max_radius)
    scale = f32(0.25 + 0.75 * rng.random())
    rad = (f32(P.min_radius) + (rad - f32(P.min_radius)) * scale).astype(f32)
    assert (rad >= f32(P.min_radius)).all() and (rad <= f32(P.max_radius)).all()
    phase = rng.uniform(0.0, 6.28, n).astype(f32)
    dead = np.zeros(n, np.int32)
    shift = 0.02 + 0.3 * rng.random()
    pos = _in_place(pos)
    now = _in_place(YR.perturbed(pos, rng, shift=shift))
    if kind != "finite" and k % 3 == 0:
        dead = (rng.random(n) < 0.3).astype(np.int32)
        dead[int(rng.integers(n))] = 1
    marked = dict(pos=pos, vel=vel, rad=rad, phase=phase, dead=dead)
    final = dict(marked, pos=now)
    if kind != "finite":
        if k in planted_at(nsims):
            final = _plant(final, n)
        if k in empty_members(nsims):
            final = dict(final, pos=np.full((n, 2), np.nan, f32))
            if k == nsims - 1:
                marked = dict(marked, pos=np.full((n, 2), np.nan, f32))
        if kind == "huge" and k == nsims - 1:
            rad = final["rad"].copy()
            rad[HUGE_BOT] = 2048.0
            marked, final = dict(marked, rad=rad), dict(final, rad=rad)
    return AC._frozen(marked), AC._frozen(final)


def member_params(orc, k, n):
    return orc.default_params(nCells=n, nDead=0, seed=900 + k, max_time=1e9, phase_update_interval=0.3,
                              spring=SPRING0 + 3.0 * k, damping=0.5, display_shadow=0, centroid_steps=16, centroid_int=0.1)


@functools.lru_cache(maxsize=None)
def state(name):
    """The named batch, built once on the host and shared read-only."""
    from oracle import orclib as orc
    base = name.replace("_huge", "").replace("_finite", "")
    nsims, n = SHAPES[base]
    kind = "huge" if name.endswith("_huge") else "finite" if name.endswith("_finite") else "main"
    params = [member_params(orc, k, n) for k in range(nsims)]
    both = [member_states(params[k], k, n, nsims, kind) for k in range(nsims)]
    return Shape(name, nsims, n, params, 4.0e6, [b[0] for b in both], [b[1] for b in both], VIEW)


def shuffle(st):
    """The fixed order of the second batch: member j of it is member shuffle(st)[j] of the first."""
    return np.random.default_rng(SHUFFLE_SEED + st.nsims).permutation(st.nsims)


def permuted(st, perm):
    return st._replace(name=f"{st.name}_shuffled", params=[st.params[p] for p in perm],
                       marked=[st.marked[p] for p in perm], final=[st.final[p] for p in perm])


# ---- the references: every member, one list per call ------------------------------------------------------------------

LINK_FAMILIES = ("clusters", "structure", "rearrangement", "strain", "entries")


def references(st, link_only=False):
    """call name -> the expectation of the whole batch, member by member, from tests/*_ref.py alone."""
    from particlerobotsimulations_amd import _capi
    out = {}
    final, marked = st.final, st.marked
    for gap in GAPS:
        out[f"clusters({gap})"] = [CR.analyse(s["pos"], s["rad"], gap) for s in final]
    out["structure"] = [SR.analyse(s["pos"], s["rad"], MARK_GAP) for s in final]
    out["rearrangement"] = [YR.analyse(a["pos"], a["rad"], s["pos"], s["rad"], MARK_GAP) for a, s in zip(marked, final)]
    out["strain"] = [TR.analyse(a["pos"], a["rad"], s["pos"], MARK_GAP, STRAIN_THRESHOLD) for a, s in zip(marked, final)]
    out["entries"] = sum(r[0]["bonds_marked"] for r in out["rearrangement"])
    if link_only:
        return out
    for r_max, bins in RADIAL:
        out[f"radial({r_max}, {bins})"] = np.stack([SR.radial_counts(s["pos"], s["rad"], r_max, bins) for s in final])
    out["moments"] = [MR.moments(s["pos"], s["vel"], s["rad"]) for s in final]
    out["centroids"] = np.array([AC.centroid_restated(s["pos"]) for s in final], np.float64)
    for nx, ny in FIELD_SHAPES:
        out[f"field({nx}x{ny})"] = [FR.field_map(s["pos"], s["vel"], s["rad"], s["dead"], nx=nx, ny=ny, **VIEW)
                                    for s in final]
    vectors = AC.sk_vectors(SK_COUNT)
    for kind in SK_KINDS:
        out[f"sfactor({kind})"] = [QR.structure_factor(s["pos"], s["vel"], s["rad"], vectors, SK_BOX, kind) for s in final]
    for kind in KINDS:
        refs = [KR.pair_correlation(kind, s["pos"], s["vel"], s["rad"], *CORRELATION,
                                    a["pos"] if kind == "displacement" else None) for a, s in zip(marked, final)]
        out[f"correlation({kind})"] = ([KR.rows_of(r, _capi.CORRELATION_BIN_DTYPE) for r in refs],
                                       [r["totals"] for r in refs])
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    st = state(name)
    return references(st, link_only=name.endswith("_huge"))


def member_references(st, m):
    """What the per-member getters of member m are compared with (the whole-batch lists hold the rest)."""
    from oracle import orclib as orc
    s, P = st.final[m], st.params[m]
    out = {"network": NR.network(orc, P, s["pos"], s["vel"], s["rad"], MARK_GAP)}
    with np.errstate(all="ignore"):
        out["colours"] = DR.colours(s["rad"], s["dead"], np.zeros(st.n, bool), P.min_radius, P.max_radius, 0)
        out["frame"] = RR.render(RR.scene_from(P, light_radius=0.25), RR.View(*RENDER), s["pos"], s["rad"], s["dead"])
    return out


# ---- the comparisons: one member's answer against its reference, the way the family's own test file compares ----------

def strip_rounds(row):
    return {k: row[k] for k in CR.FIELDS}


def check_cluster_row(got, want):
    assert strip_rounds(got) == want[0], (got, want[0])


def check_labels(got, want):
    AC.ints_equal(got[0], want[1])
    AC.ints_equal(got[1], want[2])


def check_structure_row(got, want):
    keys = ("bonds", "psi6_re", "psi6_im", "coordination")
    assert {k: got[k] for k in keys} == want[0], (got, want[0])


def check_hexatic(got, want):
    assert got[0].dtype == np.complex128 and got[1].dtype == np.uint32
    AC.ints_equal(got[1], want[2])
    assert np.array_equal(AC.psi_bits(got[0]), AC.psi_bits(want[1]))


def check_radial_row(got, want):
    assert got.dtype == np.uint64 and got.shape == want.shape
    AC.ints_equal(got, want)
    assert not (got & np.uint64(1)).any()


def check_moments_row(got, want):
    assert {k: got[k] for k in MR.FIELDS} == want, (got, want)


def check_centroid(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (got, want)
    assert np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]), (got, want)


def check_field(cells, totals, want):
    assert cells.dtype.itemsize == 64
    assert totals == want[1], (totals, want[1])
    assert FR.from_device(cells) == want[0]


def check_sfactor(rows, want):
    assert rows.dtype.itemsize == 80 and rows.shape == (len(want),) and not rows["reserved"].any()
    assert QR.from_device(rows) == want


def check_correlation(rows, totals, want_rows, want_totals):
    assert rows.tobytes() == want_rows.tobytes(), np.flatnonzero(rows != want_rows)[:8]
    assert totals == want_totals, (totals, want_totals)
    assert not (rows["pairs"] & np.uint64(1)).any()


def check_rearrangement_row(got, want):
    assert got == want[0], (got, want[0])


def check_rearrangement_of(got, want):
    want = want[1]
    assert got["disp"].dtype == f32
    for k in ("marked", "now", "kept"):
        assert got[k].dtype == np.uint32
        AC.ints_equal(got[k], want[k])
    fin = np.isfinite(want["disp"])
    assert np.array_equal(got["disp"].view(np.uint32)[fin], want["disp"].view(np.uint32)[fin])
    assert np.array_equal(np.isnan(got["disp"])[~fin], np.isnan(want["disp"])[~fin])
    assert np.array_equal(np.isfinite(got["disp"]), fin)


def check_strain_row(got, want):
    assert tuple(got) == TR.FIELDS and got == want[0], {k: (got[k], want[0][k]) for k in got if got[k] != want[0][k]}


def check_strain_of(got, want):
    want = want[1]
    u64 = np.uint64
    assert got["moments"].dtype == np.int64 and got["gradient"].dtype == np.float64 and got["d2min"].dtype == np.float64
    assert np.array_equal(got["moments"], want["moments"])
    assert np.array_equal(got["d2min"].view(u64), want["d2min"].view(u64))
    assert np.array_equal(got["gradient"].view(u64), want["gradient"].view(u64))


def check_contacts(got, want):
    assert got["offsets"].dtype == np.uint32 and got["other"].dtype == np.uint32
    AC.ints_equal(got["offsets"], want["offsets"])
    AC.ints_equal(got["other"], want["other"])
    AC.same_floats(got["gap"], want["gap"])
    assert np.array_equal(got["gap"].view(np.uint32), want["gap"].view(np.uint32))
    AC.same_floats(got["force"], want["force"])


def check_frame(got, want):
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere((got != want).any(axis=2))[:8]


def every_member(st, what, check):
    """check(m) for every member; fails with the list of ALL members that failed.  Returns the members compared."""
    bad = []
    for m in range(st.nsims):
        try:
            check(m)
        except AssertionError as e:
            bad.append((m, str(e)[:200]))
    assert not bad, f"{st.name} {what}: members {[m for m, _ in bad]} differ; first: {bad[0]}"
    return st.nsims


# ---- preconditions ---------------------------------------------------------------------------------------------------

def link_cells(st, gap=MARK_GAP):
    """(cx, cy, measured) of every member's bots on the link grid as pbClusterFile states it: edge = (2 rmax + gap)
    (1 + 2^-10) with rmax the largest finite positive radius of the batch, cell = floor(coordinate * (1 / edge)) masked
    to the grid's columns and rows; cells = max(16, n rounded up to a power of two), gxLog2 = (bits + 1) / 2."""
    bits = 4
    while (1 << bits) < st.n:
        bits += 1
    gx, gy = 1 << ((bits + 1) // 2), 1 << (bits // 2)
    rad = np.stack([s["rad"] for s in st.final])
    pos = np.stack([s["pos"] for s in st.final])
    with np.errstate(all="ignore"):
        ok = (rad > 0) & (rad < np.inf)
        rmax = float(rad[ok].max())
        edge = (2.0 * rmax + float(f32(gap))) * (1.0 + 1.0 / 1024.0)
        inv = 1.0 / edge
        measured = np.isfinite(pos).all(axis=2) & np.isfinite(rad)
        safe = np.where(measured[..., None], pos, f32(0.0)).astype(np.float64)
        cx = np.floor(safe[..., 0] * inv).astype(np.int64) & (gx - 1)
        cy = np.floor(safe[..., 1] * inv).astype(np.int64) & (gy - 1)
    return cx, cy, measured, gx, gy


def check_preconditions(name):
    """Asserted from the references alone.  Returns a dict of the figures, for the summary."""
    assert name in ALL, name
    st, E = state(name), expected(name)
    nsims, n = st.nsims, st.n
    empties = empty_members(nsims)
    full = [m for m in range(nsims) if m not in empties]
    figures = {}
    # the link rule at the middle gap: a link and a bot without one in every member that has measured bots
    if not name.endswith("_huge"):
        for m in full:
            row, _, degree = E[f"clusters({MARK_GAP})"][m]
            assert row["links"] >= 1 and row["isolated"] >= 1 and (degree == 0).any(), (m, row)
    # members differ: moments and fine radial counts pairwise, cluster rows under every likely stride
    cluster_key = [tuple(tuple(E[f"clusters({gap})"][m][0].values()) for gap in GAPS) for m in range(nsims)]
    figures["distinct cluster rows"] = len(set(cluster_key))
    if "moments" in E:
        assert len({tuple(E["moments"][m].values()) for m in full}) == len(full)
        fine = E[f"radial({RADIAL[1][0]}, {RADIAL[1][1]})"]
        assert len({fine[m].tobytes() for m in full}) == len(full)
        assert all(fine[m].any() for m in full)
        if nsims * 3 < 7 ** 4:  # (more members than rows of 7 bots can tell apart: see the strides below)
            assert len({cluster_key[m] for m in full}) == len(full)
        # seven bots have fewer cluster rows than there are members, so equal rows are certain somewhere; what a test
        # needs is that a member read at a wrong stride shows: under each stride more than half of the members change
        for d in SHIFTS:
            if d < nsims:
                same = sum(cluster_key[m] == cluster_key[(m + d) % nsims] for m in range(nsims))
                assert 2 * same < nsims, (d, same)
                figures[f"equal cluster rows at stride {d}"] = same
    # the mark: bonds are lost and gained
    rows = [E["rearrangement"][m][0] for m in full]
    if not name.endswith("_huge"):
        lost, gained = sum(r["bots_lost"] > 0 for r in rows), sum(r["bots_gained"] > 0 for r in rows)
        assert 4 * lost > len(full) and 4 * gained > len(full), (lost, gained)
        figures["members that lost / gained bonds"] = (lost, gained)
        assert sum(r[0]["fitted"] > 0 for r in E["strain"]) * 2 > nsims or n < 16
        assert sum(r[0]["fitted"] for r in E["strain"]) > 0 and sum(r[0]["sum_d2"] for r in E["strain"]) > 0
    # the grid: bots in the wrap columns and rows, linked pairs across the wrap in x and in y
    cx, cy, measured, gx, gy = link_cells(st)
    if name.endswith("_huge"):
        assert gx * gy == max(16, 1 << (n - 1).bit_length())
        assert (cx[measured] == cx[measured][0]).all() or set(np.unique(cx[measured])) <= {0, gx - 1}
        assert len(set(zip(cx[measured].tolist(), cy[measured].tolist()))) <= 4  # the cells around the origin
    else:
        edge_x = measured & ((cx == 0) | (cx == gx - 1))
        edge_y = measured & ((cy == 0) | (cy == gy - 1))
        figures["share in a wrap column"] = edge_x.sum() / measured.sum()
        figures["share in a wrap row"] = edge_y.sum() / measured.sum()
        if n <= 16:
            assert (gx, gy) == (4, 4) and 4 * edge_x.sum() >= measured.sum() and 4 * edge_y.sum() >= measured.sum()
        wrap_x = wrap_y = 0
        for m in full:
            off, own, oth = NR.topology(st.final[m]["pos"], st.final[m]["rad"], MARK_GAP)
            wrap_x += int((np.abs(cx[m][own] - cx[m][oth]) == gx - 1).sum())
            wrap_y += int((np.abs(cy[m][own] - cy[m][oth]) == gy - 1).sum())
        assert wrap_x > 0 and wrap_y > 0, (wrap_x, wrap_y)
        figures["links across the wrap (x, y)"] = (wrap_x, wrap_y)
    # the field-map view: members inside, straddling and outside
    if "field(8x8)" in E:
        tot = [E["field(8x8)"][m][1] for m in full]
        kinds = collections.Counter("inside" if t["outside"] == 0 else "outside" if t["inside"] == 0 else "straddling"
                                    for t in tot if t["measured"])
        assert all(kinds[k] >= 3 for k in ("inside", "straddling", "outside")), kinds
        figures["field view"] = dict(kinds)
    # dead and unmeasured bots where the recipe puts them
    assert all((st.final[m]["dead"].sum() > 0) == (m % 3 == 0) for m in range(nsims))
    for m in planted_at(nsims):
        if "field(8x8)" in E and m not in empties:
            assert E["field(8x8)"][m][1]["unmeasured"] == 5, (m, E["field(8x8)"][m][1])
    # the empty members: what each reference calls empty
    for m in empties:
        for gap in GAPS:
            row = E[f"clusters({gap})"][m][0]
            assert row["links"] == 0 and row["max_degree"] == 0 and row["largest"] <= 1, (m, row)
        assert E["structure"][m][0]["bonds"] == 0 and E["structure"][m][0]["psi6_re"] == 0
        r = E["rearrangement"][m][0]
        assert r["bonds_now"] == r["bonds_kept"] == r["measured"] == r["sum_q2"] == r["max_q2"] == 0, (m, r)
        t = E["strain"][m][0]
        assert t["fitted"] == t["bonds_used"] == t["sum_d2"] == 0 and t["unfitted"] == n, (m, t)
        if "moments" in E:
            assert E["moments"][m]["measured"] == 0 and not any(E["moments"][m][k] for k in MR.SUMS + MR.SQUARES)
            assert np.isnan(E["centroids"][m]).all()
            assert all(not E[f"radial({r_max}, {bins})"][m].any() for r_max, bins in RADIAL)
            for nx, ny in FIELD_SHAPES:
                cells, tot = E[f"field({nx}x{ny})"][m]
                assert tot["measured"] == tot["inside"] == tot["outside"] == 0 and tot["unmeasured"] == n
                assert not _any_value(cells)
            for kind in SK_KINDS:
                assert all(row["measured"] == 0 and not any(row[k] for k in QR.SUMS) for row in E[f"sfactor({kind})"][m])
            for kind in KINDS:
                rows_k, totals_k = E[f"correlation({kind})"]
                assert totals_k[m]["measured"] == 0 and totals_k[m]["pairs"] == 0 and not rows_k[m]["pairs"].any()
    return figures


def _any_value(cells):
    """Whether a nest of lists and dicts holds anything but zeros."""
    if isinstance(cells, dict):
        return any(_any_value(v) for v in cells.values())
    if isinstance(cells, (list, tuple)):
        return any(_any_value(v) for v in cells)
    return bool(cells)
