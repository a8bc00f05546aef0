#!/usr/bin/env python3
"""What the pair correlations cost: the device route (pbSimPairCorrelation) against the radial pair counts on the same
state, rMax and bins (pbSimRadialCounts: the same walk with one LDS atomic per pair instead of five), and against the
state copy alone that a host route starts with (pbSimGetStateOf of pos + vel + rad, before its neighbour search), all in
one process on one GPU.

  python tools/correlation_cost.py [--reps 20] [--rmax 1.175] [--bins 200] [--kind velocity]
                                   [--out profiles/pair_correlation.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps, and 256 members of 1000 bots.  Over --reps repetitions
after two untimed ones, the figures taken alternately: device milliseconds of one correlation analysis (front end,
k_corr_gather and k_corr_sweep: pbSimGetCorrelationTimes) and wall milliseconds of the whole call, the same two of one
radial histogram, wall milliseconds of the copy of every member; medians and spreads (max - min).  The two kernels on
their own are not separated by the library's clock: their durations come from a kernel trace of this tool.  The file
starts with the commit, the kernel-source hash and the register counts of the code objects
(tests/test_correlation_code_objects.py compares those).  --registers-only writes the register table with the cost rows
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
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_corr_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def copy_pos_vel_rad(sim, member, bufs):
    from particlerobotsimulations_amd import _capi
    _capi.check(_capi.lib().pbSimGetStateOf(sim._h, member, _capi.np_ptr(bufs[0]), _capi.np_ptr(bufs[1]),
                                            _capi.np_ptr(bufs[2]), None, None, None, None), "pbSimGetStateOf")


def measure(sim, members, args):
    bufs = (np.empty((sim.n, 2), np.float32), np.empty((sim.n, 2), np.float32), np.empty(sim.n, np.float32))
    cols = {k: [] for k in ("corr_dev", "corr_wall", "rdf_dev", "rdf_wall", "copy")}
    got = counts = None
    for r in range(args.reps + 2):
        sim.synchronize()
        t0 = time.perf_counter()
        got = sim.pair_correlation(args.kind, args.rmax, args.bins)
        t1 = time.perf_counter()
        corr_dev = sim.correlation_times()[1]
        t2 = time.perf_counter()
        counts = sim.radial_counts(args.rmax, args.bins)
        t3 = time.perf_counter()
        rdf_dev = sim.structure_times()[1]
        t4 = time.perf_counter()
        for m in range(members):
            copy_pos_vel_rad(sim, m, bufs)
        t5 = time.perf_counter()
        if r >= 2:
            for k, v in (("corr_dev", corr_dev), ("corr_wall", (t1 - t0) * 1e3), ("rdf_dev", rdf_dev),
                         ("rdf_wall", (t3 - t2) * 1e3), ("copy", (t5 - t4) * 1e3)):
                cols[k].append(v)
    return {k: np.array(v) for k, v in cols.items()}, got, counts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rmax", type=float, default=1.175, help="10 x max_radius, the runner's default")
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--kind", default="velocity", choices=("velocity", "radius"))
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_correlation.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = "# Pair correlations (csrc/pb_correlate.hip): code-object registers and cost (tools/correlation_cost.py)."
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_correlation_code_objects.py compares; the sweep's LDS table is sized at the launch, 40 bytes "
                 "per bin)")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/correlation_cost.py (which rewrites this file on a GPU, with the "
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
              "# tools/correlation_cost.py --reps %d --rmax %g --bins %d --kind %s: milliseconds, median (max - min)" %
              (args.reps, args.rmax, args.bins, args.kind),
              "# case members bots | correlation_device_ms spread | pbSimPairCorrelation_wall_ms spread | "
              "radial_device_ms spread | pbSimRadialCounts_wall_ms spread | pos_vel_rad_copy_wall_ms spread | "
              "ordered pairs of the batch, the same from the radial counts, measured bots of member 0 | "
              "the call beats the copy"]
    sp = lambda a: float(a.max() - a.min())

    def case(name, sim, members):
        cols, (rows, totals), counts = measure(sim, members, args)
        med = {k: float(np.median(v)) for k, v in cols.items()}
        beats = "yes" if med["corr_wall"] < med["copy"] else "NO"
        lines.append("cost %s %d %d | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %d %d %d | %s" %
                     (name, members, sim.n, med["corr_dev"], sp(cols["corr_dev"]), med["corr_wall"], sp(cols["corr_wall"]),
                      med["rdf_dev"], sp(cols["rdf_dev"]), med["rdf_wall"], sp(cols["rdf_wall"]), med["copy"],
                      sp(cols["copy"]), int(rows["pairs"].sum()), int(counts.sum()), totals[0]["measured"], beats))
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
