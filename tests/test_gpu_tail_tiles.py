"""The throughput form's split-lane tail (pbSimSetTailTiles, csrc/pb_force.hip): the last tiles of every XCD's share
of the grid run with two lanes per bot.  Results must not depend on it, bit for bit: the bench arena with the tail
on and off, through re-sorts, and arenas large enough to have a tail (>= 64 tiles) against the CPU oracle -- a blob
across the grid's x-wrap, payload mode, a batch of two members, tail counts that do not divide the tile count."""
import os
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal, jittered_blob, simparams_from_orc

pytestmark = pytest.mark.gpu
KEYS = ("pos", "vel", "rad", "phase", "absForce_a", "absForce_r")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def _throughput_row(pb, attraction_sums):
    for i, f in enumerate(pb.force_forms()):
        if f["flat"] and f["lanes_per_bot"] == 1 and not f["offsets64"] and f["attraction_sums"] == attraction_sums:
            return i
    raise AssertionError("no throughput row in the forms table")


@pytest.mark.parametrize("sums", [1, 0])
def test_bench_arena_tail_on_and_off_bit_identical(pb, sums):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import benchkit as K
    states = []
    for tail in (-1, 0):
        sim = K.make_sim(pb, 1_000_000, K.LATTICE_PITCH, seed=1, force_sums=sums)
        sim.set_tail_tiles(tail)
        cfg = sim.config()
        assert cfg["lanes_per_bot"] == 1 and cfg["attraction_sums"] == sums, cfg
        assert (cfg["tail_tiles"] > 0) == (tail != 0) and (cfg["tail_lanes"] > 0) == (tail != 0), cfg
        assert sim.step(40, sort_interval=0.12) == 40   # re-sorts every 12 steps
        states.append(sim.get_state())
        sim.close()
    for k in KEYS:
        if states[0][k] is None:
            assert states[1][k] is None
            continue
        assert_bit_equal(states[0][k], states[1][k], f"{k} (tail on vs off, sums {sums})")


def _blob(orc, n, seed, center, **over):
    P = orc.default_params(nCells=n, nDead=over.pop("nDead", 0), seed=seed, phase_std=0.0, max_time=1e9,
                           phase_update_interval=0.5, **over)
    osim = orc.Sim(P, reset=True)
    pos, vel, rad = jittered_blob(n, 0.158, np.random.default_rng(seed), center=center, jitter=0.12)
    osim.set("pos", pos), osim.set("vel", vel), osim.set("rad", rad)
    return P, osim


# n >= 64 tiles of 256 bots (the XCD order and the tail need them); tail counts per XCD that cut the XCD's share
# at various points, all of it included (the share of an XCD here is 9 or 10 tiles)
@pytest.mark.parametrize("sums", [1, 0])
@pytest.mark.parametrize("case,tail", [("wrap", 3), ("wrap", 9), ("payload", 5), ("plain", 1)])
def test_tail_tiles_match_the_oracle(pb, orc, case, tail, sums):
    if case == "payload":
        P, osim = _blob(orc, 17000, 31, (0.0, 0.0), nDead=-1, attractionFactor=0.5, massFactor=2.0, radFactor=2.0)
    elif case == "wrap":   # across the grid's x-wrap (x = -64 + 512 * 0.235)
        P, osim = _blob(orc, 20000, 32, (56.0, -50.0))
    else:
        P, osim = _blob(orc, 16500, 33, (-10.0, 20.0))
    sp, keep = simparams_from_orc(P)
    gsim = pb.Sim(sp, keepalive=keep)
    gsim.set_state(pos=osim.get("pos"), vel=osim.get("vel"), rad=osim.get("rad"), phase=osim.get("phase"),
                   dead=osim.get("dead"))
    gsim.select_force_form(_throughput_row(pb, sums))
    gsim.set_tail_tiles(tail)
    cfg = gsim.config()
    assert cfg["tail_tiles"] == tail and cfg["payload"] == (case == "payload"), cfg
    step = 0
    for k in (1, 2, 30):   # un-fused first step, fused steps, a re-sort at 20
        osim.run(k - step, sort_interval=0.2)
        assert gsim.step(k - step, sort_interval=0.2) == k - step
        step = k
        st = gsim.get_state()
        for key in KEYS:
            if st[key] is None:
                continue
            assert_bit_equal(st[key], osim.get(key), f"{case} tail {tail} sums {sums}: {key} after {k} steps")


def test_tail_tiles_in_a_batch_of_two_members(pb, orc):
    members = [_blob(orc, 17500, 40 + m, (5.0 * m, -3.0)) for m in range(2)]
    sps = [simparams_from_orc(P) for P, _ in members]
    ens = pb.Ensemble([sp for sp, _ in sps], keepalive=[keep for _, keep in sps])
    for m, (_, osim) in enumerate(members):
        ens.set_state_of(m, pos=osim.get("pos"), vel=osim.get("vel"), rad=osim.get("rad"), phase=osim.get("phase"),
                         dead=osim.get("dead"))
    ens.select_force_form(_throughput_row(pb, 1))
    ens.set_tail_tiles(7)
    assert ens.config()["tail_tiles"] == 7
    for _, osim in members:
        osim.run(25, sort_interval=0.2)
    assert ens.step(25, sort_interval=0.2) == 25
    for m, (_, osim) in enumerate(members):
        st = ens.get_state_of(m)
        for key in KEYS:
            if st.get(key) is not None:
                assert_bit_equal(st[key], osim.get(key), f"member {m}: {key}")
