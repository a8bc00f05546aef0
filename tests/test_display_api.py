"""The display surface (updateCol / calcCOG, the engine's colours and centroid trail) without a GPU: the symbols are
exported and declared, the runner documents its flags, and the numpy restatements of tests/display_ref.py reproduce
hand-computed values."""
import os
import re
import subprocess

import numpy as np

import display_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pbSimGetColorsOf", "pbSimSetCentroidTrail", "pbSimGetCentroidTrailOf")


def test_symbols_exported_and_declared():
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "particlebot_hip.h")).read()
    for name in NEW + ("updateCol", "calcCOG"):
        assert hasattr(L, name), name
        assert re.search(r"\b%s\(" % name, header), name
    assert "does nothing" not in header


def test_runner_help_lists_display_flags():
    exe = os.path.join(ROOT, "particlerobotsimulations_amd", "bin", "particlebot_run")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "--frame-style plain|reference" in text and "--trail FILE" in text


def test_centroid_tree_by_hand():
    # n = 1: (x / 1, y / 1 + 2000)
    assert np.array_equal(R.centroid(np.array([[1.5, -2.0]], np.float32)), np.array([1.5, 1998.0], np.float32))
    # +0.0f + -0.0f is +0.0f: the centroid of one bot at (-0, -0) has x = +0
    c = R.centroid(np.array([[-0.0, -0.0]], np.float32))
    assert c.view(np.uint32)[0] == 0 and c[1] == np.float32(2000.0)
    # n = 65: two levels; block 0 holds 64 ones, block 1 one 2**24: (64 + 2**24) / 65 in fp32 after the tree
    pos = np.zeros((65, 2), np.float32)
    pos[:64, 0] = 1.0
    pos[64, 0] = 2.0 ** 24
    want = np.float32(np.float32(64.0) + np.float32(2.0 ** 24)) * np.float32(np.float32(1) / np.float32(65))
    assert R.centroid(pos)[0] == want
    # the order is the tree's, not a serial sum: 1 + 2**24 + 1 + ... loses what the pairwise tree keeps
    pos = np.zeros((64, 2), np.float32)
    pos[0, 0] = 2.0 ** 24
    pos[1:, 0] = 1.0
    tree = R.centroid(pos)[0] * np.float32(64)
    assert tree != np.float32(2.0 ** 24)  # a serial fp32 sum would stay at 2**24


def test_ring_slot():
    assert R.ring_slot(0.0, 10.0, 5) == 0
    assert R.ring_slot(25.0, 10.0, 5) == 2
    assert R.ring_slot(49.99, 10.0, 5) == 4
    assert R.ring_slot(50.0, 10.0, 5) == 0


def test_colour_by_hand():
    f = np.float32
    # radius at min_radius: g = 200/255, b = 30/255
    c = R.bot_colour(f(0.0775), 0, False, f(0.0775), f(0.1175), 0)
    assert c[0] == f(f(30) / f(255)) and c[1] == f(f(200) / f(255)) and c[2] == f(f(30) / f(255)) and c[3] == 1
    # radius at max_radius: g = 20/255, b = 210/255
    c = R.bot_colour(f(0.1175), 0, False, f(0.0775), f(0.1175), 0)
    assert c[1] == f(f(20) / f(255)) and c[2] == f(f(210) / f(255))
    # dead: black, alpha kept
    assert np.array_equal(R.bot_colour(f(0.1), 1, True, f(0.0775), f(0.1175), 1, f(0.25)), np.array([0, 0, 0, 0.25], f))
    # shadow tint halves the HSL lightness: (30, 200, 30)/255 -> l = 115/255 -> 57.5/255, hue and saturation kept
    c = R.bot_colour(f(0.0775), 0, True, f(0.0775), f(0.1175), 1)
    assert abs(float(c[1]) - 100 / 255) < 1e-6 and abs(float(c[0]) - 15 / 255) < 1e-6 and abs(float(c[2]) - 15 / 255) < 1e-6
    # without display_shadow the flag is ignored
    assert np.array_equal(R.bot_colour(f(0.09), 0, True, f(0.0775), f(0.1175), 0),
                          R.bot_colour(f(0.09), 0, False, f(0.0775), f(0.1175), 0))
