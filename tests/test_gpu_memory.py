"""GPU: nothing the engine allocates outlives its owner.  pbDeviceMemoryLive counts the device and pinned blocks the
library holds, process-wide; free device memory as the runtime reports it moves with other processes and is no measure.
Shapes are chosen so that every allocation path runs, not for size: 3 members x 300 bots (one resident workgroup per
member) and 1 member x 5000 bots (the per-step kernels), both under light-wave control, so the phase update runs.
tests/test_memory_owner.py checks the owner itself on the CPU."""
import ctypes as C
import gc

import pytest

from test_gpu_series import DT, make_batch

pytestmark = pytest.mark.gpu

BATCHES = [(3, 300), (1, 5000)]
GAP, RMAX = 0.02, 0.5
ROW_BYTES, CELL_BYTES, SNAPSHOT_BYTES = 152, 72, 16  # a moments row, a table cell of nine words, one bot's snapshot


@pytest.fixture(scope="module")
def pb():
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    return pb


def live():
    """(blocks, bytes) held right now, after Python has let go of whatever batches earlier tests left behind."""
    from particlerobotsimulations_amd import _capi
    gc.collect()
    buffers, nbytes = C.c_ulonglong(0), C.c_ulonglong(0)
    _capi.check(_capi.lib().pbDeviceMemoryLive(C.byref(buffers), C.byref(nbytes)), "pbDeviceMemoryLive")
    return int(buffers.value), int(nbytes.value)


def light_wave_batch(pb, orc, members, n):
    return make_batch(pb, orc, members, n, control=0, phase_update_interval=0.1, centroid_int=0.05, centroid_steps=4)


@pytest.mark.parametrize("members,n", BATCHES)
def test_everything_switched_on_is_given_back_by_destroy(pb, orc, members, n):
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    before = live()
    ens = light_wave_batch(pb, orc, members, n)
    created = live()
    assert created[0] > before[0] and created[1] > before[1] + 2 * 16 * members * n  # (both copies of posrad at least)

    ens.set_centroid_trail(True)
    ens.set_series(0.0, 8)
    ens.set_time_correlation(0.0, 4, 0.015625)
    _capi.check(L.pbSimSetMinDistanceMode(ens._h, 0))
    assert ens.step(25, dt=DT, sort_interval=0.2) == 25
    updates = ens.stats()["phase_updates"]
    assert updates >= 1
    _capi.check(L.pbSimSetMinDistanceMode(ens._h, 1))
    _capi.check(L.pbSimSetRng(ens._h, 1))  # XORWOW: a state per bot
    assert ens.step(25, dt=DT, sort_interval=0.2) == 25
    assert ens.stats()["phase_updates"] >= updates + 1  # (the host loop ran, on XORWOW noise)
    assert ens.series_info()["records"] == 50 and ens.time_correlation_info()["records"] == 50
    assert ens.centroid_trail()[2] >= 5
    ens.set_force_variant(3)  # the batch has its cell lists: the walk counter is allocated and read now
    assert ens.stream_walk_trips()[0] > 0

    assert len(ens.clusters(GAP)) == members
    links = ens.contacts(GAP, member=0)  # sized, then filled
    assert links["offsets"][-1] == links["other"].size
    assert ens.radial_counts(RMAX, 8).shape == (members, 8) and ens.radial_counts(RMAX, 64).shape == (members, 64)
    assert len(ens.structure(GAP)) == members
    ens.mark_reference(GAP)
    assert len(ens.rearrangement()) == members
    for bins in (8, 32):
        rows, totals = ens.pair_correlation("velocity", RMAX, bins)
        assert rows.shape == (members, bins) and len(totals) == members
    assert len(ens.moments()) == members
    assert ens.colors().shape == (n, 4)
    assert ens.render(32, 32, style="reference").shape == (32, 32, 3)
    assert ens.render(64, 64, style="reference").shape == (64, 64, 3)

    most = live()
    assert most[0] >= created[0] + 40 and most[1] > created[1]  # (the layers above hold some forty blocks of their own)
    print(members, n, "before", before, "created", created, "everything on", most)
    ens.close()
    assert live() == before


@pytest.mark.parametrize("members,n", BATCHES)
def test_time_correlation_and_series_hold_exactly_their_rings(pb, orc, members, n):
    ens = light_wave_batch(pb, orc, members, n)
    base = live()
    total = members * n
    for lags in (4, 16, 0):
        ens.set_time_correlation(0.0, lags, 0.015625)
        now = live()
        assert now[1] - base[1] == lags * total * SNAPSHOT_BYTES + members * lags * CELL_BYTES, (lags, now, base)
        assert now[0] - base[0] == (2 if lags else 0)
        if lags:
            assert ens.step(3, dt=DT, sort_interval=0.2) == 3  # (records in flight when the next Set lets the ring go)
    assert live() == base
    for capacity in (8, 32, 0):
        ens.set_series(0.0, capacity)
        now = live()
        assert now[1] - base[1] == capacity * members * ROW_BYTES, (capacity, now, base)
        assert now[0] - base[0] == (1 if capacity else 0)
    assert live() == base
    ens.close()


def test_self_tests_give_back_what_they_take(pb):
    before = live()
    assert pb.self_test(1 << 20)["sqrt_mismatches"] == 0
    assert pb.self_test_hold_threshold(1e-6)["mismatches"] == 0
    assert pb.self_test_pair_geometry(0, 1)["mismatches"] == 0
    assert pb.self_test_division(0, 1)["mismatches"] == 0
    assert pb.self_test_magnitude_root()["mismatches"] == 0
    assert pb.self_test_term_root()["mismatches"] == 0
    sampler = pb.ClockSample(0.01)
    assert live() == (before[0] + 1, before[1] + 16)
    assert sampler.end() > 0
    assert live() == before
