#!/usr/bin/env python3
"""What a structure factor costs (pbSimStructureFactor, csrc/pb_sfactor.hip): the device time of its launches
(pbSimGetStructureFactorTimes) and the time of the whole call, read-back included, against one force step and the bare
pos copy that a host route would start with (pbSimGetStateOf per member), all in one process on one GPU.

  python tools/sfactor_cost.py [--reps 20] [--out profiles/structure_factor.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps, with the 544 wavevectors of half_plane_vectors(16) and
with 4096 wavevectors, box 2^9; and a batch of 256 members of 1000 bots with the 544 wavevectors, box 2^3.  Every kind
(density, radius, velocity).  Every figure is the median of --reps repetitions after two untimed ones, with the spread
(max - min).

The file starts with the commit, the build stamp and the register counts of the code objects
(tests/test_sfactor_code_objects.py compares those).  --registers-only writes the register table with the cost rows
marked as not measured and needs no GPU; everything else needs one: there is no fallback."""
import argparse
import ctypes as C
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

KINDS = ("density", "radius", "velocity")


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_sk_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def med(a):
    a = np.asarray(a, float)
    return float(np.median(a)), float(a.max() - a.min())


def time_analyses(sim, members, vectors, box_log2, kind, reps):
    """(device ms, call ms) lists of one analysis of every member into a buffer made once."""
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    vec = _capi.sk_vectors(vectors)
    rows = np.zeros((members, len(vec)), _capi.SK_ROW_DTYPE)
    dev, call = [], []
    for r in range(reps + 2):
        sim.synchronize()
        t0 = time.perf_counter()
        _capi.check(L.pbSimStructureFactor(sim._h, _capi.sk_kind(kind), box_log2, _capi.np_ptr(vec), len(vec),
                                           _capi.np_ptr(rows)), "pbSimStructureFactor")
        t1 = time.perf_counter()
        if r >= 2:
            dev.append(sim.structure_factor_times()[1])
            call.append((t1 - t0) * 1e3)
    return dev, call, int(rows["measured"][:, 0].sum())


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_factor.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = "# Structure factor (csrc/pb_sfactor.hip): code-object registers and cost (tools/sfactor_cost.py)."
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_sfactor_code_objects.py compares)")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/sfactor_cost.py (which rewrites this file on a GPU, with the "
                 "commit and the build stamp) are not here yet.", regs_head] + register_rows(args.out)
        open(args.out, "w").write("\n".join(lines) + "\n")
        return
    import particlerobotsimulations_amd as pb
    import benchkit
    from helpers import jittered_blob
    pb.legacy.cudaInit(0, None)
    stamp = benchkit.loaded_build_stamp() or {}
    lines = [head, "# commit %s (parent of the change when the tree is not committed yet); build stamp %s" %
             (commit, json.dumps(stamp, sort_keys=True)), regs_head]
    lines += register_rows(args.out)
    lines += ["", "# tools/sfactor_cost.py --reps %d: milliseconds, median (max - min) of %d repetitions after two untimed ones"
              % (args.reps, args.reps),
              "# yard <case> <members> <bots> | force_step_device_ms spread | pos_copy_wall_ms spread",
              "# sk <case> <members> <bots> <kind> <vectors> box_log2 <e> | device_ms spread | call_wall_ms spread (read-back "
              "of 16 / 32 / 64 bytes per member and vector included) | bots measured"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def case(name, sim, members, lists, box_log2):
        (s, ss), (c, cs) = yardsticks(sim, members, args.reps)
        say("yard %s %d %d | %.4f %.4f | %.4f %.4f" % (name, members, sim.n, s, ss, c, cs))
        for vectors in lists:
            for kind in KINDS:
                dev, call, measured = time_analyses(sim, members, vectors, box_log2, kind, args.reps)
                say("sk %s %d %d %s %d box_log2 %d | %.4f %.4f | %.4f %.4f | %d"
                    % ((name, members, sim.n, kind, len(vectors), box_log2) + med(dev) + med(call) + (measured,)))

    half = pb.half_plane_vectors(16)
    many = np.random.default_rng(1).integers(-64, 65, (4096, 2)).astype(np.int32)
    sim = benchkit.make_sim(pb, 1000000, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    case("million_arena", sim, 1, (half, many), 9)
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
    case("ensemble_256x1000", ens, members, (half,), 3)
    ens.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
