"""The float64 reference of one collide step (tests/stream_ref.py) pinned against the oracle on the CPU, and the
yardstick the GPU tests of the streamlined kernel use (tests/golden/stream_step/yardstick.json): how far the
oracle's own fp32 builds are from float64 on every input of tests/test_gpu_stream_step.py.  No GPU here."""
import ctypes as C
import json

import numpy as np
import pytest

import stream_ref as sr

YARDSTICK = sr.YARDSTICK


def test_pair_law_against_collideSpheres(orc):
    """Per pair: contact or not as the oracle decides wherever the gap is further than DELTA_GAP from 0, and the
    same term.  Tolerance: the fp32 gap is off by at most an ulp of the distance (3e-8 at 0.4) plus half an ulp of the
    reach (1.5e-8); the steepest the law gets is 2 A / gap^3 = 1.4e4 N per unit at 0.0019 (the ramp has 1.1e4, the
    spring 1e3), hence 7e-4 N, plus 2e-6 relative for the fp32 operations themselves."""
    P = sr.make_params(orc, 2)
    rng = np.random.default_rng(11)
    m = 3000
    gaps = np.concatenate([sr.ladder_gaps(2000), rng.uniform(0.002, 0.4, m - 2000)])
    ra, rb = rng.uniform(0.0775, 0.1175, m).astype(np.float32), rng.uniform(0.0775, 0.1175, m).astype(np.float32)
    th = rng.uniform(0, 2 * np.pi, m)
    pa = rng.uniform(-1, 1, (m, 2)).astype(np.float32)
    pb = (pa + ((ra + rb + gaps)[:, None] * np.stack([np.cos(th), np.sin(th)], 1))).astype(np.float32)
    va, vb = rng.uniform(-1, 1, (m, 2)).astype(np.float32), rng.uniform(-1, 1, (m, 2)).astype(np.float32)
    att = np.where(rng.random(m) < 0.5, P.attraction, P.attraction * 0.3).astype(np.float32)
    ref = sr.pair_terms(P, pa, pb, va, vb, ra, rb, att)
    assert all((ref["regime"] == k).sum() > 100 for k in range(4))
    L = orc.lib()
    checked = 0
    for k in range(m):
        f, fa, fr = np.zeros(2, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32)
        L.orc_collideSpheres(C.byref(P), pa[k], pb[k], va[k], vb[k], ra[k], rb[k], att[k], f, fa, fr)
        if ref["margin"][k] <= sr.DELTA_GAP:
            continue
        checked += 1
        assert (fr[0] > 0) == (ref["regime"][k] == 0), k
        mag = fr[0] if ref["regime"][k] == 0 else fa[0]
        tol = 7e-4 + 2e-6 * ref["mag"][k]
        assert abs(f[0] - ref["tx"][k]) <= tol and abs(f[1] - ref["ty"][k]) <= tol and abs(mag - ref["mag"][k]) <= tol, k
    assert checked >= m - 30


def test_stage_calls_are_one_step_of_the_oracle(orc):
    """integrate_fp32 + collide_fp32 (the stage functions the yardstick is measured with) are exactly one
    orc.Sim.update from the same state, payload and wrap included."""
    for name in ("blob_payload", "wrap", "ladder_payload2"):
        inp = sr.step_input(name)
        sim = orc.Sim(inp["P"], reset=False)
        n = inp["n"]
        for key, a in (("pos", inp["pos0"]), ("vel", inp["vel0"]), ("rad", inp["rad"]),
                       ("phase", np.full(n, sr.FROZEN)), ("dead", np.zeros(n, np.int32))):
            sim.set(key, a)
        sim.time = sr.T0
        sim.force_sort_once()
        assert sim.update(np.float32(sr.DT)) == 0
        v, fa, fr = sr.collide_fp32(orc, inp["P"], inp["pos1"], inp["vel1"], inp["rad"])
        assert np.array_equal(sim.get("pos"), inp["pos1"]) and np.array_equal(sim.get("rad"), inp["rad"])
        assert np.array_equal(sim.get("vel"), v)
        assert np.array_equal(sim.get("absForce_a"), fa) and np.array_equal(sim.get("absForce_r"), fr)


@pytest.mark.parametrize("name", sr.STEP_INPUTS)
def test_builds_against_float64(orc, name):
    """Every fp32 build of the oracle against the float64 step: the same held / stopped bots wherever the margin
    exceeds DELTA, a held or stopped bot exactly at rest, errors of the size fp32 can have (the yardstick holds the
    figures), excluded bots within one jump.  And the cap on exclusions: at most 1 % of an input, none on a ladder."""
    inp = sr.step_input(name)
    ref = inp["ref"]
    keep = ~ref["excluded"]
    assert ref["excluded"].sum() <= 0.01 * inp["n"]
    if name.startswith("ladder"):
        assert not ref["excluded"].any()
    if name.startswith("blob") or name in ("pile", "wrap", "alias") or name.startswith("batch"):
        assert not ref["held"].any() and ref["stopped"].sum() <= 0.001 * inp["n"] + 1  # moving: vel shows every net force
    if name.startswith("rest"):
        assert ref["held"].sum() >= 3 and ref["stopped"].sum() >= 3
    # what fp32 can be off by: the gap by 4.5e-8 (pair-law test above) where the law is steepest, relative to the
    # smallest single term there is, the 2.5 N floor (sums only dilute it); a contact's term is at least the dashpot
    # on the ladder's slowest approach (0.3)
    P = inp["P"]
    steep = max(2 * P.attraction / sr.INT2 ** 3, abs(P.attraction / sr.INT2 ** 2 - sr.FMIN) / (sr.INT2 - sr.INT1), P.spring)
    lim = {"vel": 1.2 * steep * 4.5e-8 / sr.FMIN + 1e-5, "fa": 1.2 * steep * 4.5e-8 / sr.FMIN + 1e-5,
           "fr": 2 * P.spring * 4.5e-8 / (P.damping * 0.3) + 2e-6}
    if name == "ladder_noattr":
        lim["vel"] = lim["fa"] = 1e-2   # the ramp falls to A / 0.0019^2 = 0 here: near 0.0019 its own value is no scale
    for b in sr.BUILDS:
        v, fa, fr = sr.collide_fp32(orc, inp["P"], inp["pos1"], inp["vel1"], inp["rad"], b)
        rest = (v == 0).all(1)
        assert np.array_equal(rest[keep], ref["stopped"][keep]), (name, b)
        err = sr.step_errors(ref, v, fa, fr)
        for k in sr.OUTPUTS:
            assert sr.stats(err[k], keep)[0] <= lim[k], (name, b, k, sr.stats(err[k], keep)[0])
        dv = np.linalg.norm(v.astype(np.float64) - ref["vel"], axis=1)
        assert np.isfinite(v).all() and (dv[~keep] <= sr.jump_bound(ref)[~keep] + 1e-5).all(), (name, b)


def test_actuation_against_updateRad(orc):
    """The float64 actuation takes every branch on the two inputs together, and the oracle's fp32 actuation on the
    same sums lands within 2e-5 of max_radius wherever the branch margin exceeds DELTA_REL (fp32's share: t1 is
    rounded at 100 periods = 1200 s for a negative time, 6e-5 s, times the slope 0.02 per second over 0.1175)."""
    seen = set()
    for cc in (0, 1):
        inp = sr.actuation_input(cc)
        seen |= set(np.unique(inp["branch"]).tolist())
        keep = inp["margin"] > sr.DELTA_REL
        assert (~keep).sum() <= 0.01 * inp["n"] and not inp["ref1"]["excluded"].sum() > 0.01 * inp["n"]
        t1w = np.float64(inp["t1"]) + inp["phase"].astype(np.float64)
        assert (t1w[inp["phase"] < 1e7] < 0).any()     # the wrap of a negative time is reached
        fa, fr = inp["ref1"]["fa"].astype(np.float32), inp["ref1"]["fr"].astype(np.float32)
        rad2 = sr.actuate_fp32(orc, inp["P"], inp["rad1"], inp["phase"], inp["dead"], fa, fr, inp["t1"])
        e = np.abs(rad2.astype(np.float64) - inp["rad2"]) / float(inp["P"].max_radius)
        assert e[keep].max() <= 2e-5, (cc, e[keep].max())
        still = np.isin(inp["branch"], (0, 1, 2))
        assert np.array_equal(rad2[still], inp["rad1"][still])
    assert seen == set(range(len(sr.ACT_BRANCHES)))


def test_yardstick_file_is_reproducible(orc):
    """tests/golden/stream_step/yardstick.json is what tests/golden/make_stream_step.py measures now: the GPU tests
    read the file and need neither the bracket builds nor anything outside the tree."""
    want = json.load(open(YARDSTICK))
    got = sr.measure_yardstick(orc)
    for section in ("step", "actuation"):
        assert set(want[section]) == set(got[section])
        for name, rec in got[section].items():
            for key, val in rec.items():
                if isinstance(val, dict):
                    for stat in ("max", "p99"):
                        assert val[stat] == pytest.approx(want[section][name][key][stat], rel=1e-6, abs=0), (name, key)
                else:
                    assert val == want[section][name][key], (name, key)
