"""CPU side of the rasteriser's shape-and-edge tests (tests/render_cases.py; the device side is
tests/test_gpu_render_edges.py).

1. Every case exercises what it is there for (render_cases.check_preconditions).
2. tests/render_ref.py, which the device is compared against, equals the host writer's bytes on every finite case: a
   host-engine Particlebot of the case's configuration (HostSim(engine="host"), write_frame; the route of hand_made in
   tests/test_render_api.py), plain style -- a host-engine instance has no device colours.
3. A bot whose position or radius is not finite paints nothing: stated once by _paint_disc and _paint_many of render_ref,
   and recorded here for the host writer, whose (int)floorf(NaN) the language leaves open."""
import warnings

import numpy as np
import pytest

import render_cases as RC
import render_ref as RR
from helpers import assert_bit_equal
from test_render_api import assert_same_frame

f32 = np.float32


def ids(cases):
    return [c.name for c in cases]


# ---- 1. the cases ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", RC.all_cases(), ids=ids(RC.all_cases()))
def test_case_exercises_what_it_is_there_for(case):
    RC.check_preconditions(case)


def test_the_shapes_cover_every_remainder():
    assert {w * h % 4 for (w, h) in RC.SMALL_SHAPES} == {1, 2, 3} and any(w * h < 4 for (w, h) in RC.SMALL_SHAPES)
    assert all(w % 4 for (w, h) in RC.ODD_WIDTH_SHAPES)
    assert {w % 4 for (w, h) in RC.SHAPES if RC.straddles_a_row(w, h)} == {1, 2, 3}   # (2 from the 2 x 3 frame)
    assert {w for (w, h) in RC.SMALL_SHAPES if w < 4} == {1, 2, 3}
    assert set(RC.SMALL_SHAPES) | set(RC.ODD_WIDTH_SHAPES) | {(4, 4)} == set(RC.SHAPES)
    assert not RC.straddles_a_row(4, 4) and not RC.straddles_a_row(7, 1) and RC.straddles_a_row(5, 4)


def test_lane_thresholds_are_those_of_the_kernel_launch():
    """lanes_for restates lanesFor of pb_render.hip: its text has these thresholds and these lane counts."""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "particlerobotsimulations_amd",
                            "csrc", "pb_render.hip")).read()
    body = src[src.index("inline int lanesFor("):src.index("}  // namespace")]
    assert "if (!(radiusPixels > 2.0f)) return 1;" in body and "return radiusPixels > 16.0f ? 64 : 8;" in body
    above = lambda v: np.nextafter(f32(v), f32(np.inf))
    assert [RC.lanes_for(v) for v in (0.4, 2.0, above(2.0), 16.0, above(16.0), 300.0)] == [1, 1, 8, 8, 64, 64]
    assert RC.lanes_for(float("nan")) == 1


# ---- 2. the restatement equals the host writer --------------------------------------------------------------------------

def host_instance(case):
    """A host-engine Particlebot with the case's scene, bots and dead flags."""
    from particlerobotsimulations_amd import host
    over = RC.host_overrides(case)
    h = host.HostSim(None, engine="host", **over)
    assert h.n == case.n
    if case.params["nDead"] > 0:
        h.draw_dead()
    h.set("pos", case.pos)
    h.set("rad", case.rad)
    assert_bit_equal(h.get("pos"), case.pos, "pos")
    assert_bit_equal(h.get("rad"), case.rad, "rad")
    assert np.array_equal(h.get("dead"), case.dead)
    # the scene the loader resolves is the scene the restatement is given
    cfg, mine = RR.scene_from(host.load_config(None, **over)), RC.scene(case)
    assert sorted(cfg) == sorted(mine)
    for k in mine:
        assert cfg[k] == mine[k], (case.name, k, cfg[k], mine[k])
    return h


def host_frame(h, case, tmp_path):
    w, hh, c, half = case.view
    p = tmp_path / "host.ppm"
    h.write_frame(str(p), size=(w, hh), center=c, half_extent=half)
    img, head = RR.read_ppm(str(p))
    assert head == b"P6\n%d %d\n255\n" % (w, hh) and img.shape == (hh, w, 3)
    return img


@pytest.mark.parametrize("case", RC.finite_cases(), ids=ids(RC.finite_cases()))
def test_restatement_equals_host_writer(case, tmp_path):
    want = host_frame(host_instance(case), case, tmp_path)
    assert_same_frame(RC.reference(case), want, case.name)


@pytest.mark.parametrize("view", RC.shape_state_views(), ids=lambda v: "%dx%d" % v[:2])
def test_restatement_equals_host_writer_on_the_growth_views(view, tmp_path):
    """The frames of the growth sequence and the largest guarded frame: the state of the shape cases at other views."""
    case = RC.replaced(RC.shape_case(4, 4, "covered"), view=view)
    want = host_frame(host_instance(case), case, tmp_path)
    assert (want != 245).any()
    assert_same_frame(RC.render(case), want, "%dx%d" % view[:2])


@pytest.mark.parametrize("member", range(3))
def test_restatement_equals_host_writer_on_the_ensemble_members(member, tmp_path):
    for view in RC.ENSEMBLE_VIEWS:
        case = RC.replaced(RC.ensemble_cases()[member], view=view)
        want = host_frame(host_instance(case), case, tmp_path)
        assert (want != 245).any()
        assert_same_frame(RC.render(case), want, f"{case.name} {view[0]}x{view[1]}")


# ---- 3. a disc that is not finite paints nothing ------------------------------------------------------------------------

@pytest.mark.parametrize("case", RC.nonfinite_cases(), ids=ids(RC.nonfinite_cases()))
def test_host_writer_paints_nothing_for_a_bot_that_is_not_finite(case, tmp_path):
    """What this build's host writer does with (int)floorf of a NaN or an infinity: its picture is the picture of the
    state without those bots, which is the rule pixDisc and render_ref state."""
    want = host_frame(host_instance(case), case, tmp_path)
    assert_same_frame(RC.render(case, keep=RC.finite_bots(case)), want, f"{case.name}: the finite bots alone")
    assert_same_frame(RC.reference(case), want, case.name)


@pytest.mark.parametrize("case", RC.nonfinite_cases(), ids=ids(RC.nonfinite_cases()))
def test_both_painters_of_the_restatement_state_the_same_rule(case):
    """_paint_disc (n <= 4096) and _paint_many (above) on the same state: neither paints a disc that is not finite, and
    neither converts a NaN or an infinity to an integer on the way (numpy warns where it does)."""
    V = RC.view_of(case)
    rgb = RR.plain_colours(case.rad, case.dead, case.params["min_radius"], case.params["max_radius"])
    one, many = (np.full((V.h, V.w, 3), 245, np.uint8) for _ in range(2))
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*cast.*", category=RuntimeWarning)
        for i in range(case.n):
            RR._paint_disc(one, V, case.pos[i, 0], case.pos[i, 1], case.rad[i], rgb[i])
        RR._paint_many(many, V, case.pos, case.rad, rgb)
    assert np.array_equal(one, many) and np.array_equal(one, RC.reference(case))
    for i in RC.NONFINITE:
        assert not RC.painted_alone(case, i, V).any(), i
    # the same bots with the offending value made finite do paint: the rule is what keeps them out
    keep = RC.finite_bots(case)
    pos, rad = case.pos.copy(), case.rad.copy()
    pos[~np.isfinite(pos)] = 0.0
    rad[~np.isfinite(rad)] = RC.MAX_R
    mended = RC.replaced(case, pos=pos, rad=rad)
    assert not np.array_equal(RC.render(mended), RC.render(case, keep=keep))
