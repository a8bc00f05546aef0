#!/usr/bin/env python3
"""What the rearrangement analysis costs: one mark (pbSimMarkReference) and one compare (pbSimRearrangementStats)
against the two state copies that a host route would start with (pbSimGetStateOf of pos + rad, once per snapshot), and
against one force step, all in one process on one GPU.

  python tools/dynamics_cost.py [--reps 20] [--gap 0.0019] [--out profiles/dynamics_analysis.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps, and a batch of 256 members of 1000 bots.  Every
repetition, after two untimed ones: one mark, 32 more steps, one compare, two pos + rad copies.  Recorded: device
milliseconds (pbSimGetRearrangementTimes) and wall milliseconds around the call of the mark and of the compare, device
milliseconds of one force step (pbSimStepTimed over the 32 steps), wall milliseconds of the two copies together; medians
and spreads (max - min).  The file starts with the commit, the kernel-source hash and the register counts of the code
objects (tests/test_dynamics_code_objects.py compares those).  --registers-only writes the register table with the
cost rows marked as not measured and needs no GPU; everything else needs one: there is no fallback."""
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


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_dyn_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def copy_pos_rad(sim, member, bufs):
    from particlerobotsimulations_amd import _capi
    _capi.check(_capi.lib().pbSimGetStateOf(sim._h, member, _capi.np_ptr(bufs[0]), None, _capi.np_ptr(bufs[1]), None,
                                            None, None, None), "pbSimGetStateOf")


def measure(sim, members, args):
    bufs = (np.empty((sim.n, 2), np.float32), np.empty(sim.n, np.float32))
    cols = {k: [] for k in ("mark_dev", "mark_wall", "cmp_dev", "cmp_wall", "step", "copy")}
    rows = None
    for r in range(args.reps + 2):
        sim.synchronize()
        t0 = time.perf_counter()
        sim.mark_reference(args.gap)
        t1 = time.perf_counter()
        mark_dev = sim.rearrangement_times()[1]
        done, ms = sim.step_timed(32, dt=0.01, sort_interval=180.0)
        assert done == 32
        sim.synchronize()
        t2 = time.perf_counter()
        rows = sim.rearrangement()
        t3 = time.perf_counter()
        cmp_dev = sim.rearrangement_times()[1]
        t4 = time.perf_counter()
        for snapshot in range(2):  # a host route needs the state twice: then and now
            for m in range(members):
                copy_pos_rad(sim, m, bufs)
        t5 = time.perf_counter()
        if r >= 2:
            for k, v in (("mark_dev", mark_dev), ("mark_wall", (t1 - t0) * 1e3), ("cmp_dev", cmp_dev),
                         ("cmp_wall", (t3 - t2) * 1e3), ("copy", (t5 - t4) * 1e3), ("step", ms / 32.0)):
                cols[k].append(v)
    return {k: np.array(v) for k, v in cols.items()}, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gap", type=float, default=0.0019)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynamics_analysis.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = "# Rearrangement analysis (csrc/pb_dynamics.hip): code-object registers and cost (tools/dynamics_cost.py)."
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_dynamics_code_objects.py compares)")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/dynamics_cost.py (which rewrites this file on a GPU, with the "
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
    lines += ["",
              "# tools/dynamics_cost.py --reps %d --gap %g: milliseconds, median (max - min); per repetition one mark, "
              "32 steps, one compare" % (args.reps, args.gap),
              "# case members bots | mark_device_ms spread | pbSimMarkReference_wall_ms spread | compare_device_ms spread | "
              "pbSimRearrangementStats_wall_ms spread | force_step_device_ms spread | two_pos_rad_copies_wall_ms spread | "
              "bonds marked, now, kept, unchanged bots of member 0 | mark + compare beat the two copies"]
    sp = lambda a: float(a.max() - a.min())

    def case(name, sim, members):
        cols, rows = measure(sim, members, args)
        med = {k: float(np.median(v)) for k, v in cols.items()}
        beats = "yes" if med["mark_wall"] + med["cmp_wall"] < med["copy"] else "NO"
        lines.append("cost %s %d %d | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | "
                     "%d %d %d %d | %s" % (name, members, sim.n, med["mark_dev"], sp(cols["mark_dev"]), med["mark_wall"],
                                           sp(cols["mark_wall"]), med["cmp_dev"], sp(cols["cmp_dev"]), med["cmp_wall"],
                                           sp(cols["cmp_wall"]), med["step"], sp(cols["step"]), med["copy"],
                                           sp(cols["copy"]), rows[0]["bonds_marked"], rows[0]["bonds_now"],
                                           rows[0]["bonds_kept"], rows[0]["bots_unchanged"], beats))
        print(lines[-1], flush=True)

    sim = benchkit.make_sim(pb, 1000000, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    case("million_arena", sim, 1)
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
    case("ensemble_256x1000", ens, members)
    ens.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
