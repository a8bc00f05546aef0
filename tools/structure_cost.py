#!/usr/bin/env python3
"""What the structure analysis costs: the device routes (pbSimRadialCounts, pbSimStructureStats) against the state copy
alone that a host route would need first (pbSimGetStateOf of pos + rad), and against one force step, all in one process
on one GPU.

  python tools/structure_cost.py [--reps 20] [--gap 0.0019] [--rmax 1.175] [--bins 200]
                                 [--out profiles/structure_analysis.txt]

Case: the 10^6-bot arena as bench.py builds it, after 32 steps.  Over --reps repetitions after two untimed ones, the
figures taken alternately: device and wall milliseconds of one radial histogram, device and wall milliseconds of one
hexatic analysis (pbSimGetStructureTimes; wall around the call), device milliseconds of one force step
(pbSimStepTimed over 20 steps), wall milliseconds of the pos + rad copy; medians and spreads (max - min).  The file
starts with the commit, the kernel-source hash and the register counts of the code objects
(tests/test_structure_code_objects.py compares those).  --registers-only writes the register table with the cost rows
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


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_struct_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def copy_pos_rad(sim, bufs):
    from particlerobotsimulations_amd import _capi
    _capi.check(_capi.lib().pbSimGetStateOf(sim._h, 0, _capi.np_ptr(bufs[0]), None, _capi.np_ptr(bufs[1]), None, None,
                                            None, None), "pbSimGetStateOf")


def measure(sim, args):
    bufs = (np.empty((sim.n, 2), np.float32), np.empty(sim.n, np.float32))
    cols = {k: [] for k in ("rdf_dev", "rdf_wall", "hex_dev", "hex_wall", "step", "copy")}
    counts = row = None
    for r in range(args.reps + 2):
        sim.synchronize()
        t0 = time.perf_counter()
        counts = sim.radial_counts(args.rmax, args.bins)
        t1 = time.perf_counter()
        rdf_dev = sim.structure_times()[1]
        t2 = time.perf_counter()
        row = sim.structure(args.gap)
        t3 = time.perf_counter()
        hex_dev = sim.structure_times()[1]
        t4 = time.perf_counter()
        copy_pos_rad(sim, bufs)
        t5 = time.perf_counter()
        done, ms = sim.step_timed(20, dt=0.01, sort_interval=180.0)
        assert done == 20
        if r >= 2:
            for k, v in (("rdf_dev", rdf_dev), ("rdf_wall", (t1 - t0) * 1e3), ("hex_dev", hex_dev),
                         ("hex_wall", (t3 - t2) * 1e3), ("copy", (t5 - t4) * 1e3), ("step", ms / 20.0)):
                cols[k].append(v)
    return {k: np.array(v) for k, v in cols.items()}, counts, row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gap", type=float, default=0.0019)
    ap.add_argument("--rmax", type=float, default=1.175, help="10 x max_radius, the runner's default")
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_analysis.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = "# Structure analysis (csrc/pb_structure.hip): code-object registers and cost (tools/structure_cost.py)."
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_structure_code_objects.py compares)")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/structure_cost.py (which rewrites this file on a GPU, with the "
                 "commit and the build stamp) are not here yet.", regs_head] + register_rows(args.out)
        open(args.out, "w").write("\n".join(lines) + "\n")
        return
    import particlerobotsimulations_amd as pb
    import benchkit
    pb.legacy.cudaInit(0, None)
    stamp = benchkit.loaded_build_stamp() or {}
    lines = [head, "# commit %s (parent of the change when the tree is not committed yet); build stamp %s" %
             (commit, json.dumps(stamp, sort_keys=True)), regs_head]
    lines += register_rows(args.out)
    lines += ["",
              "# tools/structure_cost.py --reps %d --gap %g --rmax %g --bins %d: milliseconds, median (max - min)" %
              (args.reps, args.gap, args.rmax, args.bins),
              "# case bots | radial_device_ms spread | pbSimRadialCounts_wall_ms spread | hexatic_device_ms spread | "
              "pbSimStructureStats_wall_ms spread | force_step_device_ms spread | pos_rad_copy_wall_ms spread | "
              "ordered pairs counted, bonds, |psi6| of member 0 | each device route beats the copy"]
    sim = benchkit.make_sim(pb, 1000000, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    cols, counts, row = measure(sim, args)
    sp = lambda a: float(a.max() - a.min())
    med = {k: float(np.median(v)) for k, v in cols.items()}
    beats = "yes" if max(med["rdf_wall"], med["hex_wall"]) < med["copy"] else "NO"
    lines.append("cost million_arena %d | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | "
                 "%d %d %.6f | %s" % (sim.n, med["rdf_dev"], sp(cols["rdf_dev"]), med["rdf_wall"], sp(cols["rdf_wall"]),
                                      med["hex_dev"], sp(cols["hex_dev"]), med["hex_wall"], sp(cols["hex_wall"]),
                                      med["step"], sp(cols["step"]), med["copy"], sp(cols["copy"]), int(counts.sum()),
                                      row[0]["bonds"], abs(row[0]["psi6"]), beats))
    print(lines[-1], flush=True)
    sim.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
