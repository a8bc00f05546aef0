"""CPU side of the device rasteriser (pbSimRenderOf, csrc/pb_render.hip).

1. tests/render_ref.py, the numpy restatement of the frame's per-pixel rule that the GPU tests compare against where
   no host writer exists, is pinned here to the bytes of the host writer (Particlebot::writeFramePPM through
   HostSim(engine="host"), which places the bots and paints without a GPU): the five examples at four views and a
   non-square size, million_bots.cfg, and hand-made cases for the rule itself.
2. The C-ABI entry is declared, exported and rejects bad arguments before it touches the device; the runner knows
   --frame-render.
3. The code objects of pb_render.hip use no scratch, and the force kernels' registers are what profiles/ records."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = ["example.cfg", "example_dead_cells.cfg", "example_gap.cfg", "example_object_transport.cfg",
            "example_obstacle.cfg"]
f32 = np.float32


def cfg_path(name):
    return os.path.join(ROOT, "examples", name)


def views_of(cfg, pos, rad, size=512):
    """(name, width, height, center, half_extent): the reference camera, one bot's radius above 64 pixels, the whole
    arena, an off-centre window inside the blob (discs clipped on all four edges), and a non-square frame."""
    ref_half = float(f32(cfg.camera_y) * f32(0.57735027))
    ref_c = (float(cfg.camera_x), 0.0)
    i = int(np.argmax(rad))
    zoom_half = 0.5 * size * float(rad[i]) / 80.0
    j = int(np.argmin(((pos - np.median(pos, axis=0)) ** 2).sum(axis=1)))  # a bot in the middle of the blob
    inner = (float(pos[j, 0]) + 0.03, float(pos[j, 1]) - 0.02)
    return [("reference", size, size, ref_c, ref_half),
            ("zoom", size, size, (float(pos[i, 0]) + 0.05, float(pos[i, 1])), zoom_half),
            ("arena", size, size, (0.0, 0.0), float(cfg.wallHalf)),
            ("clipped", size, size, inner, 3.0 * float(cfg.max_radius)),
            ("nonsquare", 320, 200, ref_c, ref_half)]


def clipped_edges(V, pos, rad):
    """Which of the four frame edges cut through some bot's disc (left, right, top, bottom)."""
    cx, cy, pr = V.px(pos[:, 0]), V.py(pos[:, 1]), (rad * V.scale).astype(f32)
    inside = (cx + pr > 0) & (cx - pr < V.w) & (cy + pr > 0) & (cy - pr < V.h)
    return [bool((inside & (cx - pr < 0)).any()), bool((inside & (cx + pr > V.w)).any()),
            bool((inside & (cy - pr < 0)).any()), bool((inside & (cy + pr > V.h)).any())]


def host_frame(h, tmp_path, width, height, center, half, name="f.ppm"):
    p = tmp_path / name
    h.write_frame(str(p), size=(width, height), center=center, half_extent=half)
    img, head = RR.read_ppm(str(p))
    assert head == b"P6\n%d %d\n255\n" % (width, height) and img.shape == (height, width, 3)
    return img


def assert_same_frame(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=2))
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at (x {x}, y {y}): {got[y, x]} vs {want[y, x]}")


@pytest.mark.parametrize("example", EXAMPLES)
def test_restatement_equals_host_writer_on_examples(example, tmp_path):
    from particlerobotsimulations_amd import host
    cfg = host.load_config(cfg_path(example))
    h = host.HostSim(cfg_path(example), engine="host")
    pos, rad, dead = h.get("pos"), h.get("rad"), h.get("dead")
    scene = RR.scene_from(cfg)
    for (name, w, hh, c, half) in views_of(cfg, pos, rad):
        V = RR.View(w, hh, c, half)
        want = host_frame(h, tmp_path, w, hh, c, half)
        assert (want != 245).any(), f"{example} {name}: empty picture"
        if name == "zoom":
            assert float(rad.max()) * float(V.scale) > 64.0
        if name == "clipped":
            assert clipped_edges(V, pos, rad) == [True] * 4
        assert_same_frame(RR.render(scene, V, pos, rad, dead), want, f"{example} {name}")


def test_reference_camera_is_the_default_view(tmp_path):
    """half_extent <= 0 selects the camera the runner uses; the views above spell it out."""
    from particlerobotsimulations_amd import host
    cfg = host.load_config(cfg_path("example.cfg"))
    h = host.HostSim(cfg_path("example.cfg"), engine="host")
    a = host_frame(h, tmp_path, 256, 256, (0.0, 0.0), 0.0, "a.ppm")
    b = host_frame(h, tmp_path, 256, 256, (float(cfg.camera_x), 0.0), float(f32(cfg.camera_y) * f32(0.57735027)), "b.ppm")
    assert np.array_equal(a, b)


def test_restatement_equals_host_writer_on_a_million_bots(tmp_path):
    from particlerobotsimulations_amd import host
    path = cfg_path("million_bots.cfg")
    cfg = host.load_config(path)
    h = host.HostSim(path, engine="host")
    pos, rad, dead = h.get("pos"), h.get("rad"), h.get("dead")
    assert pos.shape[0] >= 1000000
    scene = RR.scene_from(cfg)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    c = (float((lo[0] + hi[0]) / 2), float((lo[1] + hi[1]) / 2))
    half = float(max(hi[0] - lo[0], hi[1] - lo[1]) / 2) * 1.02
    for (w, hh, cc, hf) in ((512, 512, c, half), (384, 256, (c[0] + half / 3, c[1]), half / 8)):
        want = host_frame(h, tmp_path, w, hh, cc, hf)
        assert (want != 245).any()
        assert_same_frame(RR.render(scene, RR.View(w, hh, cc, hf), pos, rad, dead), want, f"million bots {w}x{hh}")


def hand_made(tmp_path, edit, width=64, height=64, center=(0.0, 0.0), half=2.0):
    """A host-engine example_dead_cells.cfg whose first bots are moved by `edit(pos, rad, dead)`; every other bot is
    parked far outside the view.  Returns (host frame, restatement, pos, rad, dead, View)."""
    from particlerobotsimulations_amd import host
    path = cfg_path("example_dead_cells.cfg")
    cfg = host.load_config(path)
    h = host.HostSim(path, engine="host")
    h.draw_dead()  # the example's 20 dead bots, now rather than at time_to_dead
    pos, rad, dead = h.get("pos"), h.get("rad"), h.get("dead")
    pos[:] = (500.0, 500.0)
    edit(pos, rad, dead)
    h.set("pos", pos)
    h.set("rad", rad)
    assert np.array_equal(h.get("pos"), pos) and np.array_equal(h.get("rad"), rad)
    V = RR.View(width, height, center, half)
    want = host_frame(h, tmp_path, width, height, center, half)
    got = RR.render(RR.scene_from(cfg), V, pos, rad, dead)
    assert_same_frame(got, want, "hand-made")
    return want, got, pos, rad, dead, V


def dead_flags():
    from particlerobotsimulations_amd import host
    return host.HostSim(cfg_path("example_dead_cells.cfg"), engine="host").draw_dead()  # a function of the seed


def test_overlap_stack_highest_original_index_wins(tmp_path):
    live = np.flatnonzero(dead_flags() == 0)[:3]

    def edit(pos, rad, dead):
        for k, i in enumerate(live):
            pos[i] = (0.02 * k, 0.01 * k)
        rad[live] = [0.0775, 0.0975, 0.1175]  # three different colours

    img, _, pos, rad, dead, V = hand_made(tmp_path, edit, half=0.5)
    cols = RR.plain_colours(rad, dead, f32(0.0775), f32(0.1175))
    assert len({tuple(cols[i]) for i in live}) == 3
    # the pixel under the last bot's centre is covered by all three discs and shows the last one
    x, y = int(V.px(pos[live[2], 0])), int(V.py(pos[live[2], 1]))
    for i in live:
        dx, dy = f32(x) + f32(0.5) - V.px(pos[i, 0]), f32(y) + f32(0.5) - V.py(pos[i, 1])
        assert dx * dx + dy * dy <= (rad[i] * V.scale) ** 2
    assert tuple(img[y, x]) == tuple(cols[live[2]])


def test_dead_bot_is_black_and_covers_live_ones_below_it(tmp_path):
    dead0 = dead_flags()
    d = int(np.flatnonzero(dead0 != 0)[-1])
    below = int(np.flatnonzero(dead0[:d] == 0)[0])

    def edit(pos, rad, dead):
        pos[d] = (0.0, 0.0)
        pos[below] = (0.05, 0.0)

    img, _, pos, rad, dead, V = hand_made(tmp_path, edit, half=0.5)
    x, y = int(V.px(0.0)), int(V.py(0.0))
    assert tuple(img[y, x]) == (0, 0, 0)
    assert (img == (0, 0, 0)).all(axis=2).sum() > 60  # a disc of at least 4.96 pixels radius


def test_disc_tangent_to_a_pixel_centre(tmp_path):
    """scale 16: the bot at x = 0 with radius 0.09375 has pixel centre 32.0 and pixel radius 1.5 exactly; the pixel
    centres 30.5 and 33.5 of its row lie ON the circle and are covered (<=), 29.5 and 34.5 are not."""
    def edit(pos, rad, dead):
        i = int(np.flatnonzero(dead == 0)[0])
        pos[i] = (0.0, -0.03125)  # py = 32.5: row 32's centre
        rad[i] = 0.09375

    img, _, pos, rad, dead, V = hand_made(tmp_path, edit, half=2.0)
    assert V.scale == 16.0
    row = (img[32] != 245).any(axis=1)
    assert list(np.flatnonzero(row)) == [30, 31, 32, 33]


def test_width_differs_from_height(tmp_path):
    def edit(pos, rad, dead):
        live = np.flatnonzero(dead == 0)[:40]
        pos[live, 0] = np.linspace(-3.0, 3.0, 40)
        pos[live, 1] = np.linspace(-1.0, 1.0, 40)

    img, _, _, _, _, V = hand_made(tmp_path, edit, width=96, height=40, center=(0.2, 0.1), half=1.25)
    assert img.shape == (40, 96, 3) and (img != 245).any()


# ---- 2. the entry points -------------------------------------------------------------------------------------------

def test_symbol_is_declared_and_exported():
    from particlerobotsimulations_amd import _capi
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in ("pbSimRenderOf", "pbSimGetRenderStats"):
        assert name in _capi.SYMBOLS and name + "(" in header
        assert hasattr(_capi.lib(), name)
    assert C.sizeof(_capi.pbRenderView) == 28


def test_render_rejects_null_arguments_before_touching_the_device():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    view = _capi.pbRenderView(16, 16, 0.0, 0.0, 1.0, 0.25, 0)
    buf = np.zeros(16 * 16 * 3, np.uint8)
    fake = C.c_void_p(1)  # never dereferenced: the NULL checks come first
    assert L.pbSimRenderOf(None, 0, C.byref(view), _capi.np_ptr(buf)) == 2  # PB_ERR_ARG
    assert b"pbSimRenderOf" in L.pbGetLastErrorString()
    assert L.pbSimRenderOf(fake, 0, None, _capi.np_ptr(buf)) == 2
    assert L.pbSimRenderOf(fake, 0, C.byref(view), None) == 2
    assert L.pbSimGetRenderStats(None, None, None) == 2
    assert not buf.any()


def test_runner_knows_frame_render(tmp_path):
    exe = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert "--frame-render host|device" in r.stdout + r.stderr
    r = subprocess.run([exe, cfg_path("example.cfg"), "--frame-render", "gpu"], capture_output=True, text=True,
                       timeout=60, cwd=tmp_path)
    assert r.returncode != 0 and "usage" in r.stderr


def test_host_engine_has_no_device_frame(tmp_path):
    from particlerobotsimulations_amd import host
    h = host.HostSim(cfg_path("example.cfg"), engine="host")
    with pytest.raises(OSError):
        h.write_frame(str(tmp_path / "x.ppm"), size=32, renderer="device")
    with pytest.raises(RuntimeError):
        h.render(32, 32)
    with pytest.raises(ValueError):
        h.write_frame(str(tmp_path / "x.ppm"), size=32, renderer="gpu")


# ---- 3. the code objects ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def regs():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import summarize_profile
    r = summarize_profile.code_object_registers()
    if not r:
        pytest.skip("no csrc/build/*.o (libraries came prebuilt without their objects)")
    return {k: tuple(int(x) if str(x).isdigit() else x for x in v) for k, v in r.items()}


def recorded_registers():
    """kernel -> (vgpr, sgpr, lds, scratch) from the table in profiles/frame_render.txt."""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "frame_render.txt")):
        parts = line.split()
        if parts[:1] == ["reg"]:
            rows[" ".join(parts[1:-4])] = tuple(int(v) for v in parts[-4:])
    return rows


def test_render_kernels_have_no_scratch(regs):
    mine = {k: v for k, v in regs.items() if k.startswith("k_render_")}
    assert sorted(mine) == ["k_render_bots<1>", "k_render_bots<64>", "k_render_bots<8>", "k_render_resolve",
                            "k_render_trail<1>", "k_render_trail<64>", "k_render_trail<8>"]
    for k, (vgpr, sgpr, lds, scratch) in mine.items():
        assert scratch == 0 and lds == 0, (k, vgpr, sgpr, lds, scratch)
    rec = recorded_registers()
    for k, v in mine.items():
        assert rec[k] == v, (k, rec[k], v)  # the counts the profile file records are those of this build


def test_force_kernel_registers_are_unchanged(regs):
    """The force kernels' sources did not change, so neither do the rows recorded with the parent's build."""
    rec = {k: v for k, v in recorded_registers().items() if not k.startswith("k_render_")}
    assert len(rec) >= 4
    for k, v in rec.items():
        assert regs[k] == v, (k, regs[k], v)
