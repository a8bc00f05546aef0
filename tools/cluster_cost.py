#!/usr/bin/env python3
"""What a cluster analysis costs: the device route (pbSimClusterStats) against the state copy alone that a host route
would need first (pbSimGetStateOf of pos + rad for every member), and against one force step, all in one process on one
GPU.

  python tools/cluster_cost.py [--reps 20] [--gap 0.0019] [--out profiles/cluster_analysis.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps; a 256-member ensemble of examples/example_gap.cfg's
size (1000 bots each, jittered blobs), after 32 steps.  Per case, over --reps repetitions after two untimed ones, the four
figures taken alternately: device milliseconds of one analysis (pbSimGetClusterTimes), wall milliseconds of
pbSimClusterStats, device milliseconds of one force step (pbSimStepTimed over 20 steps), wall milliseconds of the
pos + rad copy; medians and spreads (max - min).  The file starts with the commit, the kernel-source hash and the
register counts of the code objects (tests/test_cluster_api.py compares those).  Needs a GPU: there is no fallback."""
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

def register_rows():
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = []
    for k in sorted(regs):
        if k.startswith("k_cluster_"):  # (the other kernels' table is profiles/cluster_parent_registers.txt)
            rows.append("reg %s %s" % (k, " ".join(str(v) for v in regs[k])))
    return rows


def copy_pos_rad(sim, members, bufs):
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    for k in range(members):
        _capi.check(L.pbSimGetStateOf(sim._h, k, _capi.np_ptr(bufs[0]), None, _capi.np_ptr(bufs[1]), None, None, None,
                                      None), "pbSimGetStateOf")


def measure(sim, members, gap, reps, dt, sort_interval):
    bufs = (np.empty((sim.n, 2), np.float32), np.empty(sim.n, np.float32))
    dev, wall, step, copy = [], [], [], []
    row = None
    for r in range(reps + 2):
        sim.synchronize()
        t0 = time.perf_counter()
        row = sim.clusters(gap)
        t1 = time.perf_counter()
        copy_pos_rad(sim, members, bufs)
        t2 = time.perf_counter()
        done, ms = sim.step_timed(20, dt=dt, sort_interval=sort_interval)
        assert done == 20
        if r >= 2:
            dev.append(sim.cluster_times()[1])
            wall.append((t1 - t0) * 1e3)
            copy.append((t2 - t1) * 1e3)
            step.append(ms / 20.0)
    return [np.array(a) for a in (dev, wall, step, copy)], row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gap", type=float, default=0.0019)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_analysis.txt"))
    args = ap.parse_args()
    import particlerobotsimulations_amd as pb
    import benchkit
    from helpers import jittered_blob
    pb.legacy.cudaInit(0, None)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    stamp = benchkit.loaded_build_stamp() or {}
    lines = ["# Cluster analysis (csrc/pb_cluster.hip): code-object registers and cost (tools/cluster_cost.py).",
             "# commit %s (parent of the change when the tree is not committed yet); build stamp %s" %
             (commit, json.dumps(stamp, sort_keys=True)),
             "# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
             "tests/test_cluster_api.py compares)"]
    lines += register_rows()
    lines += ["",
              "# tools/cluster_cost.py --reps %d --gap %g: milliseconds, median (max - min)" % (args.reps, args.gap),
              "# case members bots | analysis_device_ms spread | pbSimClusterStats_wall_ms spread | force_step_device_ms "
              "spread | pos_rad_copy_wall_ms spread | clusters largest links of member 0 | device route beats the copy"]

    def case(name, sim, members, dt, sort_interval):
        (dev, wall, step, copy), row = measure(sim, members, args.gap, args.reps, dt, sort_interval)
        sp = lambda a: float(a.max() - a.min())
        beats = "yes" if np.median(wall) < np.median(copy) else "NO"
        lines.append("cost %s %d %d | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %d %d %d | %s" % (
            name, members, sim.n, np.median(dev), sp(dev), np.median(wall), sp(wall), np.median(step), sp(step),
            np.median(copy), sp(copy), row[0]["clusters"], row[0]["largest"], row[0]["links"], beats))
        print(lines[-1], flush=True)

    sim = benchkit.make_sim(pb, 1000000, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    case("million_arena", sim, 1, 0.01, 180.0)
    sim.close()

    members, n = 256, 1000
    rng = np.random.default_rng(1)
    plist, keeps = [], []
    for k in range(members):
        sp, keep = benchkit.workload_params(n, seed=k + 1)
        plist.append(sp)
        keeps.append(keep)
    ens = pb.Ensemble(plist, wall_half=240.0, keepalive=keeps)
    for k in range(members):
        pos, vel, rad = jittered_blob(n, 0.2, rng, jitter=0.3)
        ens.set_state_of(k, pos=pos, vel=vel, rad=rad, phase=np.zeros(n, np.float32), dead=np.zeros(n, np.int32))
    assert ens.step(32) == 32
    case("ensemble_256x1000", ens, members, 0.01, 180.0)
    ens.close()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
