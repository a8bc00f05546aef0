#!/usr/bin/env python3
"""What a record of the distinct van Hove function costs (pbSimSetVanHoveDistinct, csrc/pb_vanhove_distinct.hip): the
device time of its launches (pbSimGetVanHoveDistinctTimes) with the ring full, so that a record pairs with every lag,
against its yardsticks timed in the same process on one GPU: one pbSimRadialCounts at the same rMax (the floor for a
single lag: the same filing and the same walk, each pair met from one end), one force step, one time-correlation record
and one self van Hove record at the same lags, and the bare pos copy that a host route would start with.

  python tools/vanhove_distinct_cost.py [--reps 20] [--out profiles/van_hove_distinct.txt]
  python tools/vanhove_distinct_cost.py --forms-only --libdir particlerobotsimulations_amd/lib_<tag> --tag <tag>

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps; and a batch of 256 members of 1000 bots.  16 and 64
lags; rMax of 5 and 10 min_radius in 64 bins.  One step runs between two records.  Every figure is the median of --reps
records after the ring has filled and two more untimed ones, with the spread (max - min).  The `vd` rows end with the
record's time over lags x the radial count's: how close a lag comes to its floor.

The `form` rows compare the builds of the kernel on the arena at 16 lags, both rMax: the radial bin by an fp32 guess
corrected against the LDS edges (PB_VHD_BIN_RULE 1, tag `guess`: what ships), by the self part's binary search in the
edges (0, `rule0`) or by the integer square root and one division (2, `rule2`), and equal counters of a wave combined by
ballot (PB_VHD_COMBINE 1, `combine`) against plain LDS atomics, each a library built with EXTRA_DEVFLAGS=-D... into
--libdir.  --forms-only measures only these and appends them under --tag.

The file starts with the commit, the build stamp and the register counts of the code objects
(tests/test_vanhove_distinct_code_objects.py compares those).  --registers-only writes the register table with the cost
rows marked as not measured and needs no GPU; everything else needs one: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from vanhove_cost import kept_rows, med, time_records, yardsticks  # noqa: E402  (the same medians and yardsticks)

LAGS = (16, 64)
RADII = (5.0, 10.0)
BINS = 64


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_vhd_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--forms-only", action="store_true")
    ap.add_argument("--libdir", default=None)
    ap.add_argument("--tag", default="guess")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "van_hove_distinct.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = ("# Distinct van Hove function (csrc/pb_vanhove_distinct.hip): code-object registers and cost "
            "(tools/vanhove_distinct_cost.py).")
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_vanhove_distinct_code_objects.py compares)")
    notes = kept_rows(args.out, "# note ") + kept_rows(args.out, "bench ")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/vanhove_distinct_cost.py (which rewrites this file on a GPU, "
                 "with the commit and the build stamp) are not here yet.", regs_head] + register_rows(args.out) + notes
        open(args.out, "w").write("\n".join(lines) + "\n")
        return
    if args.libdir:
        from particlerobotsimulations_amd import _capi
        _capi.LIB_DIR = os.path.abspath(args.libdir)
        _capi.HIP_SO = os.path.join(_capi.LIB_DIR, "libparticlebot_hip.so")
        _capi.HOST_SO = os.path.join(_capi.LIB_DIR, "libparticlebot_host.so")
    import particlerobotsimulations_amd as pb
    import benchkit
    from helpers import jittered_blob
    pb.legacy.cudaInit(0, None)
    stamp = benchkit.loaded_build_stamp() or {}
    lines = [head, "# commit %s (parent of the change when the tree is not committed yet); build stamp %s" %
             (commit, json.dumps(stamp, sort_keys=True)), regs_head]
    lines += register_rows(args.out) + notes
    lines += ["", "# tools/vanhove_distinct_cost.py --reps %d: milliseconds, median (max - min) of %d repetitions after two "
              "untimed ones" % (args.reps, args.reps),
              "# yard <case> <members> <bots> | force_step_device_ms spread | pos_copy_wall_ms spread",
              "# rdf <case> <members> <bots> rmax <r> bins <bins> | radial_counts_device_ms spread   (one pbSimRadialCounts)",
              "# tc <case> <members> <bots> lags <lags> | record_device_ms spread   (a time-correlation record, ring full)",
              "# vh <case> <members> <bots> lags <lags> bins <bins> width <w> | record_device_ms spread   (a self van Hove "
              "record, ring full)",
              "# vd <case> <members> <bots> lags <lags> bins <bins> rmax <r> | record_device_ms spread | over lags x rdf   "
              "(filing + snapshot + all lags, ring full, one step between records)",
              "# form <tag> <case> lags <lags> bins <bins> rmax <r> | record_device_ms spread   (a build of the kernel)"]
    if args.forms_only:
        lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def one_step(sim):
        return lambda: sim.step(1)

    def distinct(sim, lags, rmax):
        """Median and spread of a record at `lags` lags and BINS bins up to rmax, ring full; checks the table."""
        sim.set_van_hove_distinct(-1.0, lags, rmax / BINS, BINS)
        dev = time_records(sim.van_hove_distinct_record, sim.van_hove_distinct_times, lags, args.reps, one_step(sim))
        rows = sim.van_hove_distinct()[0]
        assert all(r["centres"] > 0 and r["pairs"] == sum(r["counts"]) and r["pairs"] > 0 for r in rows)
        assert all(c % 2 == 0 for c in rows[0]["counts"])
        sim.set_van_hove_distinct(-1.0, 0, 0.0, 0)
        return med(dev)

    def forms(name, sim, radius):
        for rmax in RADII:
            say("form %s %s lags 16 bins %d rmax %.6g | %.4f %.4f" % ((args.tag, name, BINS, rmax * radius)
                                                                       + distinct(sim, 16, rmax * radius)))

    def case(name, sim, members, radius):
        (s, ss), (c, cs) = yardsticks(sim, members, args.reps)
        say("yard %s %d %d | %.4f %.4f | %.4f %.4f" % (name, members, sim.n, s, ss, c, cs))
        floor = {}
        for rmax in RADII:
            ms = []
            for r in range(args.reps + 2):
                sim.radial_counts(rmax * radius, BINS)
                if r >= 2:
                    ms.append(sim.structure_times()[1])
            floor[rmax] = med(ms)
            say("rdf %s %d %d rmax %.6g bins %d | %.4f %.4f" % ((name, members, sim.n, rmax * radius, BINS) + floor[rmax]))
        for lags in LAGS:
            sim.set_time_correlation(-1.0, lags, 0.1)
            dev = time_records(sim.time_correlation_record, sim.time_correlation_times, lags, args.reps, one_step(sim))
            sim.set_time_correlation(-1.0, 0, 0.0)
            say("tc %s %d %d lags %d | %.4f %.4f" % ((name, members, sim.n, lags) + med(dev)))
            sim.set_van_hove(-1.0, lags, 0.125 * radius, BINS)
            dev = time_records(sim.van_hove_record, sim.van_hove_times, lags, args.reps, one_step(sim))
            sim.set_van_hove(-1.0, 0, 0.0, 0)
            say("vh %s %d %d lags %d bins %d width %.6g | %.4f %.4f" % ((name, members, sim.n, lags, BINS, 0.125 * radius)
                                                                        + med(dev)))
            for rmax in RADII:
                m, spread = distinct(sim, lags, rmax * radius)
                say("vd %s %d %d lags %d bins %d rmax %.6g | %.4f %.4f | %.3f"
                    % (name, members, sim.n, lags, BINS, rmax * radius, m, spread, m / (lags * floor[rmax][0])))

    sim = benchkit.make_sim(pb, 1000000, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    radius = float(sim.params.min_radius)
    if not args.forms_only:
        case("million_arena", sim, 1, radius)
    forms("million_arena", sim, radius)
    sim.close()

    if not args.forms_only:
        members, n = 256, 1000
        rng = np.random.default_rng(1)
        plist, keeps = [], []
        for k in range(members):
            p, keep = benchkit.workload_params(n, seed=k + 1)
            plist.append(p)
            keeps.append(keep)
        ens = pb.Ensemble(plist, wall_half=240.0, keepalive=keeps)
        for k in range(members):
            pos, vel, rad = jittered_blob(n, 0.2, rng, jitter=0.3)
            ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=np.zeros(n, np.float32), dead=np.zeros(n, np.int32))
        assert ens.step(32) == 32
        case("ensemble_256x1000", ens, members, float(plist[0].min_radius))
        ens.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.forms_only:
        open(args.out, "a").write("\n".join(lines) + "\n")
    else:
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
