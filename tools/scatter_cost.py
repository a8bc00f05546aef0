#!/usr/bin/env python3
"""What a record of the self-intermediate scattering function costs (pbSimSetScattering, csrc/pb_scatter.hip): the device
time of its launches (pbSimGetScatteringTimes) with the ring full, so that a record pairs with every lag, against one
force step, a time-correlation record at the same lags (pbSimGetTimeCorrelationTimes) and the bare pos copy that a host
route would start with at every sample (pbSimGetStateOf per member), all in one process on one GPU.

  python tools/scatter_cost.py [--reps 20] [--out profiles/intermediate_scattering.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps, box 2^9; and a batch of 256 members of 1000 bots, box
2^3.  16 and 64 lags; 8, 24 and 256 wavevectors (the first 8 and all 24 of half_plane_vectors(3), and 256 random ones).
Every figure is the median of --reps records after the ring has filled and two more untimed ones, with the spread
(max - min).

The file starts with the commit, the build stamp and the register counts of the code objects
(tests/test_scatter_code_objects.py compares those).  --registers-only writes the register table with the cost rows
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


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_scat_")]
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


def time_records(record, times, lags, reps):
    """Device ms of `reps` records taken once the ring holds `lags` snapshots (so that each pairs with every lag)."""
    out = []
    for r in range(lags + 2 + reps):
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intermediate_scattering.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = ("# Self-intermediate scattering (csrc/pb_scatter.hip): code-object registers and cost "
            "(tools/scatter_cost.py).")
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_scatter_code_objects.py compares)")
    notes = kept_rows(args.out, "# note ") + kept_rows(args.out, "bench ")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/scatter_cost.py (which rewrites this file on a GPU, with the "
                 "commit and the build stamp) are not here yet.", regs_head] + register_rows(args.out) + notes
        open(args.out, "w").write("\n".join(lines) + "\n")
        return
    import particlerobotsimulations_amd as pb
    import benchkit
    from helpers import jittered_blob
    pb.legacy.cudaInit(0, None)
    stamp = benchkit.loaded_build_stamp() or {}
    lines = [head, "# commit %s (parent of the change when the tree is not committed yet); build stamp %s" %
             (commit, json.dumps(stamp, sort_keys=True)), regs_head]
    lines += register_rows(args.out) + notes
    lines += ["", "# tools/scatter_cost.py --reps %d: milliseconds, median (max - min) of %d repetitions after two untimed ones"
              % (args.reps, args.reps),
              "# yard <case> <members> <bots> | force_step_device_ms spread | pos_copy_wall_ms spread",
              "# tc <case> <members> <bots> lags <lags> | record_device_ms spread   (a time-correlation record, ring full)",
              "# scat <case> <members> <bots> lags <lags> vectors <nvec> box_log2 <e> | record_device_ms spread   "
              "(snapshot + all lags, ring full)"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    half = pb.half_plane_vectors(3)
    many = np.random.default_rng(1).integers(-64, 65, (256, 2)).astype(np.int32)
    lists = (half[:8], half, many)

    def case(name, sim, members, box_log2):
        (s, ss), (c, cs) = yardsticks(sim, members, args.reps)
        say("yard %s %d %d | %.4f %.4f | %.4f %.4f" % (name, members, sim.n, s, ss, c, cs))
        for lags in LAGS:
            sim.set_time_correlation(-1.0, lags, 0.1)
            dev = time_records(sim.time_correlation_record, sim.time_correlation_times, lags, args.reps)
            sim.set_time_correlation(-1.0, 0, 0.0)
            say("tc %s %d %d lags %d | %.4f %.4f" % ((name, members, sim.n, lags) + med(dev)))
            for vectors in lists:
                sim.set_scattering(-1.0, lags, box_log2, vectors)
                dev = time_records(sim.scattering_record, sim.scattering_times, lags, args.reps)
                rows = sim.scattering()
                assert all(r["samples"] > 0 for r in rows[0][lags - 1])
                sim.set_scattering(-1.0, 0, 0, None)
                say("scat %s %d %d lags %d vectors %d box_log2 %d | %.4f %.4f"
                    % ((name, members, sim.n, lags, len(vectors), box_log2) + med(dev)))

    sim = benchkit.make_sim(pb, 1000000, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    case("million_arena", sim, 1, 9)
    sim.close()

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
    case("ensemble_256x1000", ens, members, 3)
    ens.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
