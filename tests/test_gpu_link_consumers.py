"""GPU: the three consumers of the link rule agree.  The cluster analysis (degrees of pbSimClusterLabelsOf), the contact
export (list lengths of pbSimContactsOf) and the hexatic order (neighbour counts of pbSimHexaticOf) walk the same nine
cells (pbWalkNine) and apply the same rule (pbWhenLinked, both csrc/pb_cluster.hpp): per bot the three counts are equal
to each other and to tests/cluster_ref.py on the state read back from the device, exactly.  The states are the smallest
on which the walk's cases all occur: a 4 x 4 grid (half of all columns are wrap columns), the first non-square grid
(8 x 4), several workgroups, negative and wrapped cell coordinates, and two copies of a blob that fold into the same
cells of the grid and must not link to each other."""
import numpy as np
import pytest

import cluster_ref as CR
from helpers import jittered_blob, simparams_from_orc

pytestmark = pytest.mark.gpu

f32 = np.float32
GAPS = [0.0019, 0.05]


def blob(n):
    pos, _, rad = jittered_blob(n, 0.15, np.random.default_rng(2000 + n), jitter=0.3)
    return pos, rad


def shifted_300():
    pos, rad = blob(300)
    return (pos + np.array([-37.3, 1021.7], f32)).astype(f32), rad


def twins(gap):
    """The 8-bot blob and a copy 8 cell edges further in x: 16 bots file on the 4-wide grid, whose edge is
    (2 rmax + gap) (1 + 2^-10), so a bot and its copy share a cell."""
    pos, rad = blob(8)
    edge = (2.0 * float(rad.max()) + float(f32(gap))) * (1.0 + 2.0 ** -10)
    copy = (pos.astype(np.float64) + np.array([8.0 * edge, 0.0])).astype(f32)
    return np.concatenate([pos, copy]), np.concatenate([rad, rad])


STATES = {"n16": lambda gap: blob(16), "n17": lambda gap: blob(17), "n300": lambda gap: blob(300),
          "n300_shifted": lambda gap: shifted_300(), "twins": twins}


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def sim_with(pb, orc, pos, rad):
    n = rad.size
    P = orc.default_params(nCells=n, nDead=0, seed=3, max_time=1e9)
    sp, keep = simparams_from_orc(P)
    sim = pb.Sim(sp, wall_half=4.0e6, keepalive=keep)
    sim.set_state(pos=pos, vel=np.zeros((n, 2), f32), rad=rad, phase=np.zeros(n, f32), dead=np.zeros(n, np.int32))
    return sim


@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("state", sorted(STATES))
def test_degrees_list_lengths_and_neighbour_counts_are_equal(pb, orc, state, gap):
    pos, rad = STATES[state](gap)
    n = rad.size
    sim = sim_with(pb, orc, pos, rad)
    try:
        st = sim.get_state()
        stats, _, want = CR.analyse(st["pos"], st["rad"], gap)
        print(state, gap, "links", stats["links"], "max degree", stats["max_degree"])
        assert stats["links"] >= n, (state, gap, stats)  # (no trivial case: at least one link per bot on average)
        if state == "twins":
            assert stats["links"] == {0.0019: 22, 0.05: 26}[gap]
            assert np.array_equal(want[:8], want[8:]), "the copy has the blob's degrees: no link between the two"
        degree = sim.cluster_labels(gap)[1]
        lengths = np.diff(sim.contacts(gap)["offsets"].astype(np.int64))
        neighbours = sim.hexatic(gap)[1]
        assert np.array_equal(degree, want), (state, gap, "cluster degrees")
        assert np.array_equal(lengths, want), (state, gap, "contact list lengths")
        assert np.array_equal(neighbours, want), (state, gap, "hexatic neighbour counts")
    finally:
        sim.close()


@pytest.mark.parametrize("n", [16, 17])
def test_radial_counts_hold_every_ordered_pair(pb, orc, n):
    """rMax 3.0 is wider than the blob, and its grid (4 x 4, 8 x 4) folds the blob onto itself: every ordered pair is
    counted once."""
    pos, rad = blob(n)
    sim = sim_with(pb, orc, pos, rad)
    try:
        counts = sim.radial_counts(3.0, 7, member=0)
        assert int(counts.sum()) == n * (n - 1), counts
    finally:
        sim.close()
