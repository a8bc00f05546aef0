#!/usr/bin/env python3
"""What a record of the self van Hove function costs (pbSimSetVanHove, csrc/pb_vanhove.hip): the device time of its
launches (pbSimGetVanHoveTimes) with the ring full, so that a record pairs with every lag, against one force step, a
time-correlation record at the same lags (pbSimGetTimeCorrelationTimes) and the bare pos copy that a host route would
start with at every sample (pbSimGetStateOf per member), all in one process on one GPU.

  python tools/vanhove_cost.py [--reps 20] [--out profiles/van_hove.txt]
  python tools/vanhove_cost.py --forms-only --libdir particlerobotsimulations_amd/lib_<tag> --tag <tag>

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps; and a batch of 256 members of 1000 bots.  16 and 64
lags; 64 and 1024 bins an eighth of min_radius wide.  One step runs between two records, so the short lags fall into one
or two bins.  Every figure is the median of --reps records after the ring has filled and two more untimed ones, with
the spread (max - min).

The `form` rows compare how a wave adds to the LDS histogram (vhCount: plain LDS atomics, or PB_VH_COMBINE_ROUNDS rounds
of a ballot leader loop in a library built with EXTRA_DEVFLAGS=-DPB_VH_COMBINE_ROUNDS=<k> into --libdir) on the arena at
16 lags and 64 bins, on three states: `still` (no step between records: every pair adds to the same counter of each
histogram, the worst contention there is), `stepped` (one step between records) and `broad` (every bot moved by a step
of its own, uniform in [-3, 3] per axis, between records: tests/test_vanhove_api.py's recipe).  --forms-only measures
only these and appends them to the file under --tag.

The file starts with the commit, the build stamp and the register counts of the code objects
(tests/test_vanhove_code_objects.py compares those).  --registers-only writes the register table with the cost rows
marked as not measured and needs no GPU; everything else needs one: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAGS = (16, 64)
BINS = (64, 1024)
f32 = np.float32


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_vh_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def kept_rows(out, prefix):
    """Rows of the file as it is that another tool or a person wrote (the `bench` rows): kept when the file is rewritten."""
    if not os.path.exists(out):
        return []
    return [l.rstrip("\n") for l in open(out) if l.startswith(prefix)]


def med(a):
    a = np.asarray(a, float)
    return float(np.median(a)), float(a.max() - a.min())


def time_records(record, times, lags, reps, between=None):
    """Device ms of `reps` records taken once the ring holds `lags` snapshots (so that each pairs with every lag);
    between() runs in front of every record."""
    out = []
    for r in range(lags + 2 + reps):
        if between:
            between()
        record()
        if r >= lags + 2:
            out.append(times()[1])
    return out


def yardsticks(sim, members, reps):
    """Medians of one force step and of the copy of pos of every member."""
    from particlerobotsimulations_amd import _capi
    pos = np.empty((sim.n, 2), np.float32)
    step, copy = [], []
    for r in range(reps + 2):
        sim.synchronize()
        done, ms = sim.step_timed(64, dt=0.01, sort_interval=180.0)
        assert done == 64
        sim.synchronize()
        t0 = time.perf_counter()
        for k in range(members):
            _capi.check(_capi.lib().pbSimGetStateOf(sim._h, k, _capi.np_ptr(pos), None, None, None, None, None, None),
                        "pbSimGetStateOf")
        t1 = time.perf_counter()
        if r >= 2:
            step.append(ms / 64), copy.append((t1 - t0) * 1e3)
    return med(step), med(copy)


def identities_hold(row):
    return all(sum(row[k]) + row["beyond_" + b] == row["samples"] for k, b in (("radial", "r"), ("x", "x"), ("y", "y")))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--forms-only", action="store_true")
    ap.add_argument("--libdir", default=None)
    ap.add_argument("--tag", default="plain")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "van_hove.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = "# Self van Hove function (csrc/pb_vanhove.hip): code-object registers and cost (tools/vanhove_cost.py)."
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_vanhove_code_objects.py compares)")
    notes = kept_rows(args.out, "# note ") + kept_rows(args.out, "bench ")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/vanhove_cost.py (which rewrites this file on a GPU, with the "
                 "commit and the build stamp) are not here yet.", regs_head] + register_rows(args.out) + notes
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
    lines += ["", "# tools/vanhove_cost.py --reps %d: milliseconds, median (max - min) of %d repetitions after two untimed ones"
              % (args.reps, args.reps),
              "# yard <case> <members> <bots> | force_step_device_ms spread | pos_copy_wall_ms spread",
              "# tc <case> <members> <bots> lags <lags> | record_device_ms spread   (a time-correlation record, ring full)",
              "# vh <case> <members> <bots> lags <lags> bins <bins> width <w> | record_device_ms spread   "
              "(snapshot + all lags, ring full, one step between records)",
              "# form <tag> <case> <state> lags <lags> bins <bins> | record_device_ms spread   (vhCount: plain, or "
              "PB_VH_COMBINE_ROUNDS rounds of a ballot leader loop)"]
    if args.forms_only:
        lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def one_step(sim):
        return lambda: sim.step(1)

    def forms(name, sim, width):
        """The three states at 16 lags and 64 bins."""
        lags, bins = 16, 64
        st = sim.get_state()
        rng = np.random.default_rng(7)
        pos = [st["pos"].copy()]

        def walk():
            pos[0] = (pos[0] + rng.integers(-3072, 3073, size=pos[0].shape).astype(f32) / f32(1024.0)).astype(f32)
            sim.set_state(pos=pos[0], vel=st["vel"], rad=st["rad"], phase=st["phase"], dead=st["dead"])

        for state, between, w in (("still", None, width), ("stepped", one_step(sim), width), ("broad", walk, 0.125)):
            sim.set_van_hove(-1.0, lags, w, bins)
            dev = time_records(sim.van_hove_record, sim.van_hove_times, lags, args.reps, between)
            rows = sim.van_hove()[0]
            assert all(r["samples"] > 0 and identities_hold(r) for r in rows)
            used = sum(1 for c in rows[1]["radial"] if c)
            sim.set_van_hove(-1.0, 0, 0.0, 0)
            say("form %s %s %s lags %d bins %d | %.4f %.4f   (lag 1 fills %d radial bins)"
                % ((args.tag, name, state, lags, bins) + med(dev) + (used,)))
        sim.set_state(pos=st["pos"], vel=st["vel"], rad=st["rad"], phase=st["phase"], dead=st["dead"])

    def case(name, sim, members, width):
        (s, ss), (c, cs) = yardsticks(sim, members, args.reps)
        say("yard %s %d %d | %.4f %.4f | %.4f %.4f" % (name, members, sim.n, s, ss, c, cs))
        for lags in LAGS:
            sim.set_time_correlation(-1.0, lags, 0.1)
            dev = time_records(sim.time_correlation_record, sim.time_correlation_times, lags, args.reps, one_step(sim))
            sim.set_time_correlation(-1.0, 0, 0.0)
            say("tc %s %d %d lags %d | %.4f %.4f" % ((name, members, sim.n, lags) + med(dev)))
            for bins in BINS:
                sim.set_van_hove(-1.0, lags, width, bins)
                dev = time_records(sim.van_hove_record, sim.van_hove_times, lags, args.reps, one_step(sim))
                rows = sim.van_hove()
                assert all(r["samples"] > 0 and identities_hold(r) for r in rows[0])
                sim.set_van_hove(-1.0, 0, 0.0, 0)
                say("vh %s %d %d lags %d bins %d width %.6g | %.4f %.4f"
                    % ((name, members, sim.n, lags, bins, width) + med(dev)))

    sim = benchkit.make_sim(pb, 1000000, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    width = 0.125 * float(sim.params.min_radius)
    if not args.forms_only:
        case("million_arena", sim, 1, width)
    forms("million_arena", sim, width)
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
        case("ensemble_256x1000", ens, members, 0.125 * float(plist[0].min_radius))
        ens.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.forms_only:
        open(args.out, "a").write("\n".join(lines) + "\n")
    else:
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
