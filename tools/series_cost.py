#!/usr/bin/env python3
"""What the time-series recorder costs: one record (pbSimSetSeries; the device time of its two launches from
pbSimGetSeriesTimes) against one force step and against the pos + vel + rad copy that a host route would start with
(pbSimGetStateOf per member), and what a stepping window costs per step with the series at a sparse interval and at
every step against the same window with the series off, all in one process on one GPU.

  python tools/series_cost.py [--reps 20] [--window 64] [--sparse 0.16] [--out profiles/series_recording.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps, and a batch of 256 members of 1000 bots.  Every
repetition, after two untimed ones: a window of --window steps (dt 0.01) with the series off, the same with the series
at --sparse (window * 0.01 / sparse records) and at interval 0 (a record in front of every step, no fused launch), each
timed by pbSimStepTimed; the last record's device time; one copy of pos + vel + rad of every member.  Medians and
spreads (max - min).  The file starts with the commit, the kernel-source hash and the register counts of the code
objects (tests/test_series_code_objects.py compares those).  --registers-only writes the register table with the cost
rows marked as not measured and needs no GPU; everything else needs one: there is no fallback."""
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
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_mom_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def copy_state(sim, member, bufs):
    from particlerobotsimulations_amd import _capi
    _capi.check(_capi.lib().pbSimGetStateOf(sim._h, member, _capi.np_ptr(bufs[0]), _capi.np_ptr(bufs[1]),
                                            _capi.np_ptr(bufs[2]), None, None, None, None), "pbSimGetStateOf")


def measure(sim, members, args):
    bufs = (np.empty((sim.n, 2), np.float32), np.empty((sim.n, 2), np.float32), np.empty(sim.n, np.float32))
    cols = {k: [] for k in ("off", "sparse", "every", "record", "copy")}
    taken = {}
    w = args.window

    def window(interval):
        sim.set_series(interval if interval is not None else 0.0, w if interval is not None else 0)
        sim.synchronize()
        done, ms = sim.step_timed(w, dt=0.01, sort_interval=180.0)
        assert done == w
        return ms / w, sim.series_info()["records"]

    for r in range(args.reps + 2):
        off, none = window(None)
        sparse, taken["sparse"] = window(args.sparse)
        every, taken["every"] = window(0.0)
        assert none == 0 and taken["every"] == w
        record = sim.series_times()[1]
        sim.set_series(0.0, 0)
        sim.synchronize()
        t0 = time.perf_counter()
        for m in range(members):
            copy_state(sim, m, bufs)
        t1 = time.perf_counter()
        if r >= 2:
            for k, v in (("off", off), ("sparse", sparse), ("every", every), ("record", record),
                         ("copy", (t1 - t0) * 1e3)):
                cols[k].append(v)
    return {k: np.array(v) for k, v in cols.items()}, taken


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--sparse", type=float, default=0.16)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "series_recording.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = "# Time-series recorder (csrc/pb_moments.hip): code-object registers and cost (tools/series_cost.py)."
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_series_code_objects.py compares)")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/series_cost.py (which rewrites this file on a GPU, with the "
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
              "# tools/series_cost.py --reps %d --window %d --sparse %g: milliseconds, median (max - min); per repetition "
              "three windows of %d steps (dt 0.01): series off, at interval %g, at interval 0"
              % (args.reps, args.window, args.sparse, args.window, args.sparse),
              "# case members bots | record_device_ms spread | force_step_device_ms (series off) spread | "
              "per_step_device_ms at the sparse interval spread | per_step_device_ms at interval 0 spread | "
              "pos_vel_rad_copy_wall_ms spread | records per window: sparse, every step"]
    sp = lambda a: float(a.max() - a.min())

    def case(name, sim, members):
        cols, taken = measure(sim, members, args)
        med = {k: float(np.median(v)) for k, v in cols.items()}
        lines.append("cost %s %d %d | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %d %d"
                     % (name, members, sim.n, med["record"], sp(cols["record"]), med["off"], sp(cols["off"]),
                        med["sparse"], sp(cols["sparse"]), med["every"], sp(cols["every"]), med["copy"],
                        sp(cols["copy"]), taken["sparse"], taken["every"]))
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
