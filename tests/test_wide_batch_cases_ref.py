"""The wide-batch tests without a GPU: the batches of tests/wide_batch_cases.py hold what their description says
(check_preconditions, from the references alone), the shuffle is a real permutation that moves every chosen member, the
every-member comparison names exactly the members that differ, and the whole reference side of a shape runs in seconds
(printed; the GPU tests compute it once per process)."""
import time

import numpy as np
import pytest

import wide_batch_cases as W

f32 = np.float32


@pytest.mark.parametrize("name", W.ALL)
def test_preconditions(orc, name):
    t0 = time.perf_counter()
    st = W.state(name)
    W.expected(name)
    seconds = time.perf_counter() - t0
    figures = W.check_preconditions(name)
    print(f"{name}: {st.nsims} x {st.n}, the reference side in {seconds:.1f} s; {figures}")
    assert (st.nsims, st.n) == W.SHAPES[name.replace("_huge", "")]
    assert seconds < 60.0  # (about five on one core: anything near a minute means a reference went quadratic in members)


@pytest.mark.parametrize("name", W.MAIN)
def test_shape_marks_the_edges_it_is_there_for(orc, name):
    st = W.state(name)
    assert st.nsims % 256 == 1 and st.n < 64 and st.n & (st.n - 1)
    cells = max(16, 1 << (st.n - 1).bit_length())
    assert cells == {40: 64, 7: 16}[st.n] and st.nsims * cells + 1 == {257: 16449, 1025: 16401}[st.nsims]
    chosen = W.chosen(st)
    assert len(set(chosen)) == 8 and set(W.empty_members(st.nsims)) <= set(chosen) and {0, 63, 64} <= set(chosen)
    assert st.nsims - 1 in chosen and st.nsims - 2 in chosen
    assert len({P.spring for P in st.params}) == st.nsims
    # the plants: five distinct bots, none of them the pair's partner, the outlier or the huge radius' bot
    planted = st.final[0]
    bots = W.plants(st.n)
    assert len(bots) == 5
    assert np.isnan(planted["pos"][:, 0]).sum() == 1 and np.isinf(planted["pos"][:, 1]).sum() == 1
    assert (planted["pos"][:, 0] == -2048.0).sum() == 1 and (planted["vel"][:, 1] == 2048.0).sum() == 1
    assert np.isnan(planted["rad"]).sum() == 1 and not (planted["rad"] == 2048.0).any()
    for m in W.empty_members(st.nsims):
        assert np.isnan(st.final[m]["pos"]).all()
    assert np.isfinite(st.marked[128]["pos"]).all() and np.isnan(st.marked[st.nsims - 1]["pos"]).all()
    # the variant differs in one radius of the last member and nowhere else
    huge = W.state(name + "_huge")
    for m in range(st.nsims):
        for key in ("pos", "vel", "rad", "phase", "dead"):
            a, b = st.final[m][key], huge.final[m][key]
            if m == st.nsims - 1 and key == "rad":
                assert b[W.HUGE_BOT] == 2048.0 and np.flatnonzero(a.view(np.uint32) != b.view(np.uint32)).tolist() == [4]
            else:
                assert a.tobytes() == b.tobytes(), (m, key)


def test_the_recorders_batch_is_finite(orc):
    st = W.state(W.FINITE)
    assert (st.nsims, st.n) == (257, 40)
    for s in st.marked + st.final:
        assert all(np.isfinite(s[k]).all() for k in ("pos", "vel", "rad", "phase")) and not s["dead"].any()


@pytest.mark.parametrize("name", W.MAIN)
def test_shuffle_is_a_permutation_that_moves_every_chosen_member(orc, name):
    st = W.state(name)
    perm = W.shuffle(st)
    assert sorted(perm.tolist()) == list(range(st.nsims))
    assert np.array_equal(perm, W.shuffle(st))
    for m in W.chosen(st):
        assert perm[m] != m, m
    assert (perm != np.arange(st.nsims)).sum() > st.nsims - 8
    shuffled = W.permuted(st, perm)
    assert shuffled.final[0] is st.final[perm[0]] and shuffled.params[5] is st.params[perm[5]]


@pytest.mark.parametrize("name", W.MAIN)
def test_every_member_comparison_names_exactly_the_members_that_differ(orc, name):
    """The reference rows stand in for the device's; two members of the expectation are swapped."""
    st, E = W.state(name), W.expected(name)
    got = E["moments"]
    assert W.every_member(st, "moments", lambda m: W.check_moments_row(got[m], E["moments"][m])) == st.nsims
    a, b = 2, st.nsims - 2
    swapped = list(E["moments"])
    swapped[a], swapped[b] = swapped[b], swapped[a]
    with pytest.raises(AssertionError, match=rf"members \[{a}, {b}\] differ"):
        W.every_member(st, "moments", lambda m: W.check_moments_row(got[m], swapped[m]))
