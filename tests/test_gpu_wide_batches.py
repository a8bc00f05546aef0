"""GPU: the on-demand analyses on batches of 257 and 1025 members (tests/wide_batch_cases.py), EVERY member against the
restatement of its family in tests/*_ref.py, exactly as the family's own test file compares (integers equal, floats bit
for bit, NaN where the reference is NaN).  The member count is the point: 257 is one past the 256 lanes of the row
kernels' workgroup, 1025 one past 1024 with the 4 x 4 minimum grid per member, and every member differs from the others
(check_preconditions, asserted here before the first device call).

A comparison over all members collects every member that fails and names them all (every_member), so an answer that is
right for members 0 to 2 and shifted behind them shows where it starts.  Each test prints its wall time and the number
of members it compared.

Three tests need less than the references: the huge-radius variants run the link-rule families with every member folded
into one cell, a lone Sim must give the bits of the member inside the batch, and a batch built in a shuffled member
order must give the first batch's results, permuted, bit for bit."""
import time

import numpy as np
import pytest

import analysis_session_cases as AC
import wide_batch_cases as W
from helpers import simparams_from_orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def bring(pb, st, members=None):
    """A fresh session on the device: the marked state written with set_state_of, the mark taken at MARK_GAP, then the
    present state written.  members: a batch of those members only (None: all)."""
    members = range(st.nsims) if members is None else members
    sps = [simparams_from_orc(st.params[m]) for m in members]
    sim = pb.Ensemble([sp for sp, _ in sps], wall_half=st.wall_half, keepalive=[k for _, k in sps])
    for k, m in enumerate(members):
        sim.set_state_of(k, **st.marked[m])
    sim.mark_reference(W.MARK_GAP)
    for k, m in enumerate(members):
        sim.set_state_of(k, **st.final[m])
    return sim


def bring_alone(pb, st, m):
    sp, keep = simparams_from_orc(st.params[m])
    sim = pb.Sim(sp, wall_half=st.wall_half, keepalive=keep)
    sim.set_state(**st.marked[m])
    sim.mark_reference(W.MARK_GAP)
    sim.set_state(**st.final[m])
    return sim


def link_calls(sim):
    """The whole-batch calls of the link-rule families: name -> result, one entry per member."""
    out = {f"clusters({gap})": [W.strip_rounds(r) for r in sim.clusters(gap)] for gap in W.GAPS}
    out["structure"] = sim.structure(W.MARK_GAP)
    out["rearrangement"] = sim.rearrangement()
    out["strain"] = sim.strain(W.STRAIN_THRESHOLD)
    return out


def counting_calls(sim):
    """The whole-batch calls of the other families."""
    out = {f"radial({r}, {b})": sim.radial_counts(r, b) for r, b in W.RADIAL}
    out["moments"] = sim.moments()
    out["centroids"] = sim.centroids()
    for nx, ny in W.FIELD_SHAPES:
        out[f"field({nx}x{ny})"] = sim.field_map(nx, ny, W.VIEW["center"], W.VIEW["half"])
    for kind in W.SK_KINDS:
        out[f"sfactor({kind})"] = sim.structure_factor(AC.sk_vectors(W.SK_COUNT), W.SK_BOX, kind=kind)
    for kind in W.KINDS:
        out[f"correlation({kind})"] = sim.pair_correlation(kind, *W.CORRELATION)
    return out


def member_calls(sim, m):
    """The per-member getters of member m: name -> result."""
    nx, ny = W.FIELD_SHAPES[0]
    return {
        "cluster_labels": sim.cluster_labels(W.MARK_GAP, member=m),
        "contacts": sim.contacts(W.MARK_GAP, member=m),
        "contact_virial": sim.contact_virial(W.MARK_GAP, member=m),
        "hexatic": sim.hexatic(W.MARK_GAP, member=m),
        "rearrangement_of": sim.rearrangement_of(m),
        "strain_of": sim.strain_of(m),
        "colors": sim.colors(m),
        "field_map": sim.field_map(nx, ny, W.VIEW["center"], W.VIEW["half"], member=m),
        "structure_factor": sim.structure_factor(AC.sk_vectors(W.SK_COUNT), W.SK_BOX, kind="velocity", member=m),
        "radial_counts": sim.radial_counts(*W.RADIAL[0], member=m),
        "pair_correlation": sim.pair_correlation("displacement", *W.CORRELATION, member=m),
        "render": sim.render(*W.RENDER, light_radius=0.25, member=m),
    }


def check_link_calls(st, E, got):
    """Every member of every link-rule call against the references; returns the members compared per call."""
    counts = {}
    for gap in W.GAPS:
        key = f"clusters({gap})"
        counts[key] = W.every_member(st, key, lambda m: W.check_cluster_row(got[key][m], E[key][m]))
    counts["structure"] = W.every_member(st, "structure", lambda m: W.check_structure_row(got["structure"][m],
                                                                                           E["structure"][m]))
    counts["rearrangement"] = W.every_member(st, "rearrangement", lambda m: W.check_rearrangement_row(
        got["rearrangement"][m], E["rearrangement"][m]))
    counts["strain"] = W.every_member(st, "strain", lambda m: W.check_strain_row(got["strain"][m], E["strain"][m]))
    for key, rows in got.items():
        assert len(rows) == st.nsims, key
    return counts


def check_counting_calls(st, E, got):
    counts = {}
    for r, b in W.RADIAL:
        key = f"radial({r}, {b})"
        assert got[key].shape == (st.nsims, b)
        counts[key] = W.every_member(st, key, lambda m: W.check_radial_row(got[key][m], E[key][m]))
    assert len(got["moments"]) == st.nsims and got["centroids"].shape == (st.nsims, 2)
    counts["moments"] = W.every_member(st, "moments", lambda m: W.check_moments_row(got["moments"][m], E["moments"][m]))
    counts["centroids"] = W.every_member(st, "centroids", lambda m: W.check_centroid(got["centroids"][m],
                                                                                      E["centroids"][m]))
    for nx, ny in W.FIELD_SHAPES:
        key = f"field({nx}x{ny})"
        cells, totals = got[key]
        assert cells.shape == (st.nsims, ny, nx) and len(totals) == st.nsims
        counts[key] = W.every_member(st, key, lambda m: W.check_field(cells[m], totals[m], E[key][m]))
    for kind in W.SK_KINDS:
        key = f"sfactor({kind})"
        assert got[key].shape == (st.nsims, W.SK_COUNT)
        counts[key] = W.every_member(st, key, lambda m: W.check_sfactor(got[key][m], E[key][m]))
    for kind in W.KINDS:
        key = f"correlation({kind})"
        rows, totals = got[key]
        assert rows.shape == (st.nsims, W.CORRELATION[1]) and len(totals) == st.nsims
        counts[key] = W.every_member(st, key, lambda m: W.check_correlation(rows[m], totals[m], E[key][0][m],
                                                                            E[key][1][m]))
    return counts


def check_member_calls(st, E, m, got):
    ref = W.member_references(st, m)
    W.check_labels(got["cluster_labels"], E[f"clusters({W.MARK_GAP})"][m])
    W.check_contacts(got["contacts"], ref["network"])
    AC.same_floats(got["contact_virial"], ref["network"]["virial"])
    W.check_hexatic(got["hexatic"], E["structure"][m])
    W.check_rearrangement_of(got["rearrangement_of"], E["rearrangement"][m])
    W.check_strain_of(got["strain_of"], E["strain"][m])
    AC.nan_aware_bits(got["colors"], ref["colours"])
    nx, ny = W.FIELD_SHAPES[0]
    W.check_field(got["field_map"][0], got["field_map"][1], E[f"field({nx}x{ny})"][m])
    W.check_sfactor(got["structure_factor"], E["sfactor(velocity)"][m])
    r, b = W.RADIAL[0]
    W.check_radial_row(got["radial_counts"], E[f"radial({r}, {b})"][m])
    rows, totals = E["correlation(displacement)"]
    W.check_correlation(got["pair_correlation"][0], got["pair_correlation"][1], rows[m], totals[m])
    W.check_frame(got["render"], ref["frame"])


def report(what, t0, counts):
    print(f"{what}: {time.perf_counter() - t0:.2f} s on the device side; members compared {counts}")


# ---- every member against its reference -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", W.MAIN)
def test_link_rule_families_every_member(pb, orc, name):
    """clusters at three gaps, hexatic order, and the mark with its readers: rearrangement, strain, entries."""
    W.check_preconditions(name)
    st, E = W.state(name), W.expected(name)
    t0 = time.perf_counter()
    sim = bring(pb, st)
    got = link_calls(sim)
    info = sim.reference_info()
    counts = check_link_calls(st, E, got)
    assert info["marked"] and info["gap"] == float(np.float32(W.MARK_GAP)) and info["entries"] == E["entries"], info
    assert set(counts.values()) == {st.nsims}
    report(f"{name} link-rule families", t0, counts)


@pytest.mark.parametrize("name", W.MAIN)
def test_counting_families_every_member(pb, orc, name):
    """radial counts, moments, centroids, field maps, structure factors and the three pair correlations."""
    W.check_preconditions(name)
    st, E = W.state(name), W.expected(name)
    t0 = time.perf_counter()
    sim = bring(pb, st)
    counts = check_counting_calls(st, E, counting_calls(sim))
    assert set(counts.values()) == {st.nsims}
    report(f"{name} counting families", t0, counts)


@pytest.mark.parametrize("name", W.MAIN)
def test_per_member_getters_at_the_chosen_members(pb, orc, name):
    W.check_preconditions(name)
    st, E = W.state(name), W.expected(name)
    t0 = time.perf_counter()
    sim = bring(pb, st)
    for m in W.chosen(st):
        try:
            check_member_calls(st, E, m, member_calls(sim, m))
        except AssertionError as e:
            raise AssertionError(f"{name} member {m}: {e}") from e
    report(f"{name} getters", t0, len(W.chosen(st)))


# ---- the huge radius ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", W.HUGE)
def test_one_radius_of_2048_folds_every_member_into_one_cell(pb, orc, name):
    W.check_preconditions(name)
    st, E = W.state(name), W.expected(name)
    t0 = time.perf_counter()
    sim = bring(pb, st)
    got = link_calls(sim)
    counts = check_link_calls(st, E, got)
    assert sim.reference_info()["entries"] == E["entries"]
    assert set(counts.values()) == {st.nsims}
    # the radius changes no link outside its own member (whose positions are NaN): the rows are the main batch's
    main = W.expected(name.replace("_huge", ""))
    for key in counts:
        assert [r[0] for r in E[key]] == [r[0] for r in main[key]], key
    report(f"{name} link-rule families", t0, counts)


# ---- a member alone -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", W.MAIN)
def test_a_lone_sim_gives_the_bits_of_the_member_inside_the_batch(pb, orc, name):
    st = W.state(name)
    t0 = time.perf_counter()
    sim = bring(pb, st)
    for m in W.chosen(st):
        inside = member_calls(sim, m)
        alone = member_calls(bring_alone(pb, st, m), 0)
        for key in inside:
            assert AC.same_bits(inside[key], alone[key]), (name, m, key)
    report(f"{name} lone Sim", t0, len(W.chosen(st)))


# ---- the members in another order ----------------------------------------------------------------------------------------

def permute(result, perm):
    """A whole-batch result with its members in the order `perm` reads them."""
    if isinstance(result, np.ndarray):
        return result[perm]
    if isinstance(result, tuple):
        return tuple(permute(r, perm) for r in result)
    return [result[p] for p in perm]


@pytest.mark.parametrize("name", W.MAIN)
def test_shuffled_members_give_the_same_results_permuted(pb, orc, name):
    """No reference at all: the second batch holds the same members in another order."""
    st = W.state(name)
    perm = W.shuffle(st)
    t0 = time.perf_counter()
    first = bring(pb, st)
    second = bring(pb, W.permuted(st, perm))
    a = dict(link_calls(first), **counting_calls(first))
    b = dict(link_calls(second), **counting_calls(second))
    assert first.reference_info() == second.reference_info()
    counts = {}
    for key in a:
        want = permute(a[key], perm)
        assert AC.same_bits(b[key], want), (name, key, _differing(b[key], want))
        counts[key] = st.nsims
    report(f"{name} shuffled", t0, counts)


def _differing(got, want):
    """The members (positions in the second batch) at which two whole-batch results differ."""
    if isinstance(got, tuple):
        return sorted(set(sum((_differing(g, w) for g, w in zip(got, want)), [])))[:16]
    return [m for m in range(len(got)) if not AC.same_bits(got[m], want[m])][:16]
