#!/usr/bin/env python3
"""What the strain analysis costs: one pbSimStrainStats on the device and as a call, and in the same run one
pbSimRearrangementStats, one force step, and the bare `pos` copy a host route would start with (pbSimGetStateOf of pos
alone, every member once), all in one process on one GPU.

  python tools/strain_cost.py [--reps 20] [--gap 0.0019] [--variant original] [--lib PATH] [--out profiles/strain_analysis.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps, and a batch of 256 members of 1000 bots.  One mark, then
every repetition, after two untimed ones: 32 more steps, one strain call, one compare, one pos copy.  Recorded: device
milliseconds (pbSimGetStrainTimes, pbSimGetRearrangementTimes) and wall milliseconds around each call, device
milliseconds of one force step (pbSimStepTimed over the 32 steps), wall milliseconds of the copy; medians and spreads
(max - min).

k_strain_fit deals its lanes to bots in ORIGINAL order; built with EXTRA_DEVFLAGS=-DPB_STRAIN_SORTED_LANES (into another
LIBDIR and BUILD, see csrc/Makefile) it deals them in the current sorted order.  --lib loads such a library instead of
the package's own and --variant names it in the rows; with --append the rows are added to the file instead of replacing
it, so that both variants stand side by side.  --registers-only writes the register table with the cost rows marked as
not measured and needs no GPU; everything else needs one: there is no fallback."""
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

HEAD = "# Strain analysis (csrc/pb_strain.hip): code-object registers and cost (tools/strain_cost.py)."
REGS_HEAD = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects of the shipped variant; "
             "tests/test_strain_code_objects.py compares)")


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_strain_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def copy_pos(sim, member, buf):
    from particlerobotsimulations_amd import _capi
    _capi.check(_capi.lib().pbSimGetStateOf(sim._h, member, _capi.np_ptr(buf), None, None, None, None, None, None),
                "pbSimGetStateOf")


def measure(sim, members, args):
    buf = np.empty((sim.n, 2), np.float32)
    cols = {k: [] for k in ("strain_dev", "strain_wall", "cmp_dev", "cmp_wall", "step", "copy")}
    rows = None
    sim.mark_reference(args.gap)
    for r in range(args.reps + 2):
        done, ms = sim.step_timed(32, dt=0.01, sort_interval=180.0)
        assert done == 32
        sim.synchronize()
        t0 = time.perf_counter()
        rows = sim.strain(args.threshold)
        t1 = time.perf_counter()
        strain_dev = sim.strain_times()[1]
        t2 = time.perf_counter()
        sim.rearrangement()
        t3 = time.perf_counter()
        cmp_dev = sim.rearrangement_times()[1]
        t4 = time.perf_counter()
        for m in range(members):
            copy_pos(sim, m, buf)
        t5 = time.perf_counter()
        if r >= 2:
            for k, v in (("strain_dev", strain_dev), ("strain_wall", (t1 - t0) * 1e3), ("cmp_dev", cmp_dev),
                         ("cmp_wall", (t3 - t2) * 1e3), ("copy", (t5 - t4) * 1e3), ("step", ms / 32.0)):
                cols[k].append(v)
    return {k: np.array(v) for k, v in cols.items()}, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gap", type=float, default=0.0019)
    ap.add_argument("--threshold", type=float, default=0.0001)
    ap.add_argument("--variant", default="original", help="how this library deals lanes to bots: a label for the rows")
    ap.add_argument("--lib", default=None, help="a libparticlebot_hip.so to load instead of the package's own")
    ap.add_argument("--append", action="store_true", help="add the cost rows to --out instead of rewriting it")
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strain_analysis.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    if args.registers_only:
        lines = [HEAD.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/strain_cost.py (which rewrites this file on a GPU, with the "
                 "commit and the build stamp) are not here yet.", REGS_HEAD] + register_rows(args.out)
        open(args.out, "w").write("\n".join(lines) + "\n")
        return
    from particlerobotsimulations_amd import _capi
    if args.lib:
        _capi.HIP_SO = os.path.abspath(args.lib)  # before the first lib(): the package loads this one
    import particlerobotsimulations_amd as pb
    import benchkit
    from helpers import jittered_blob
    pb.legacy.cudaInit(0, None)
    stamp = benchkit.loaded_build_stamp() or {}
    lines = []
    if not args.append:
        lines = [HEAD, "# commit %s (parent of the change when the tree is not committed yet); build stamp %s" %
                 (commit, json.dumps(stamp, sort_keys=True)), REGS_HEAD]
        lines += register_rows(args.out)
        lines += ["",
                  "# tools/strain_cost.py --reps N --gap G: milliseconds, median (max - min); one mark, then per "
                  "repetition 32 steps, one strain call, one compare, one pos copy",
                  "# cost <variant> <case> members bots | strain_device_ms spread | pbSimStrainStats_wall_ms spread | "
                  "compare_device_ms spread | pbSimRearrangementStats_wall_ms spread | force_step_device_ms spread | "
                  "pos_copy_wall_ms spread | fitted, unfitted, above, bonds used, bonds dropped of member 0 | "
                  "the strain call beats the pos copy"]
    sp = lambda a: float(a.max() - a.min())

    def case(name, sim, members):
        cols, rows = measure(sim, members, args)
        med = {k: float(np.median(v)) for k, v in cols.items()}
        beats = "yes" if med["strain_wall"] < med["copy"] else "NO"
        r = rows[0]
        lines.append("cost %s %s %d %d | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | "
                     "%d %d %d %d %d | %s" % (args.variant, name, members, sim.n, med["strain_dev"], sp(cols["strain_dev"]),
                                              med["strain_wall"], sp(cols["strain_wall"]), med["cmp_dev"],
                                              sp(cols["cmp_dev"]), med["cmp_wall"], sp(cols["cmp_wall"]), med["step"],
                                              sp(cols["step"]), med["copy"], sp(cols["copy"]), r["fitted"], r["unfitted"],
                                              r["above"], r["bonds_used"], r["bonds_dropped"], beats))
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
    open(args.out, "a" if args.append else "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
