#!/usr/bin/env python3
"""What the time correlations cost: one record (pbSimTimeCorrelationRecord; the device span of its two launches from
pbSimGetTimeCorrelationTimes, and the wall time of the call, which does not wait) with a full ring of 16 and of 64 lags,
against one force step and against the bare pos + vel copy that a host route would start with (pbSimGetStateOf per
member), and what a stepping window costs per step with a record every 16 steps against the same window with the
correlation off, all in one process on one GPU.

  python tools/timecorr_cost.py [--reps 20] [--window 64] [--sparse 0.16] [--out profiles/time_correlation.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps, and a batch of 256 members of 1000 bots.  Per case, in
this order, each after a warm-up that also fills the ring: --reps windows of --window steps (dt 0.01) with the
correlation off; the same with 16 lags at --sparse (window * 0.01 / sparse records per window), each timed by
pbSimStepTimed; --reps manual records with 16 lags, then with 64; --reps copies of pos + vel of every member, each
followed by one of pos + vel + rad, the yardstick of the series' and the pair correlations' rows.  Medians and spreads
(max - min).  The file starts with the commit, the kernel-source hash and the register counts of the code
objects (tests/test_timecorr_code_objects.py compares those).  --registers-only writes the register table with the cost
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

RADIUS = 0.0775  # the example configurations' min_radius


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_tc_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def copy_pos_vel(sim, member, bufs, rad=False):
    from particlerobotsimulations_amd import _capi
    _capi.check(_capi.lib().pbSimGetStateOf(sim._h, member, _capi.np_ptr(bufs[0]), _capi.np_ptr(bufs[1]),
                                            _capi.np_ptr(bufs[2]) if rad else None, None, None, None, None),
                "pbSimGetStateOf")


def measure(sim, members, args):
    bufs = (np.empty((sim.n, 2), np.float32), np.empty((sim.n, 2), np.float32), np.empty(sim.n, np.float32))
    cols = {k: [] for k in ("off", "sparse", "dev16", "call16", "dev64", "call64", "copy", "copy3")}
    w = args.window

    def window():
        sim.synchronize()
        done, ms = sim.step_timed(w, dt=0.01, sort_interval=180.0)
        assert done == w
        return ms / w

    sim.set_time_correlation(0.0, 0, 0.0)
    for r in range(args.reps + 2):
        v = window()
        if r >= 2:
            cols["off"].append(v)
    sim.set_time_correlation(args.sparse, 16, RADIUS)
    before = None
    for r in range(args.reps + 6):  # six untimed windows: the ring of 16 fills
        if r == 6:
            before = sim.time_correlation_info()["records"]
        v = window()
        if r >= 6:
            cols["sparse"].append(v)
    per_window = (sim.time_correlation_info()["records"] - before) / args.reps
    for lags in (16, 64):
        sim.set_time_correlation(-1.0, lags, RADIUS)
        for r in range(lags + args.reps):  # `lags` untimed records: every lag has its partner
            sim.synchronize()
            t0 = time.perf_counter()
            sim.time_correlation_record()
            t1 = time.perf_counter()
            if r >= lags:
                cols["dev%d" % lags].append(sim.time_correlation_times()[1])
                cols["call%d" % lags].append((t1 - t0) * 1e3)
    sim.set_time_correlation(0.0, 0, 0.0)
    for r in range(args.reps + 2):
        sim.synchronize()
        t0 = time.perf_counter()
        for m in range(members):
            copy_pos_vel(sim, m, bufs)
        t1 = time.perf_counter()
        for m in range(members):  # the series' and the pair correlations' yardstick, in the same run
            copy_pos_vel(sim, m, bufs, rad=True)
        t2 = time.perf_counter()
        if r >= 2:
            cols["copy"].append((t1 - t0) * 1e3)
            cols["copy3"].append((t2 - t1) * 1e3)
    return {k: np.array(v) for k, v in cols.items()}, per_window


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--sparse", type=float, default=0.16)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_correlation.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = "# Time correlations (csrc/pb_timecorr.hip): code-object registers and cost (tools/timecorr_cost.py)."
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_timecorr_code_objects.py compares)")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/timecorr_cost.py (which rewrites this file on a GPU, with the "
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
              "# tools/timecorr_cost.py --reps %d --window %d --sparse %g: milliseconds, median (max - min); windows of %d "
              "steps (dt 0.01) with the correlation off, then with 16 lags at interval %g; then single records into a "
              "full ring of 16 and of 64 lags; then the copy" % (args.reps, args.window, args.sparse, args.window,
                                                                   args.sparse),
              "# case members bots | record_device_ms at 16 lags spread | record_call_ms at 16 lags spread | "
              "record_device_ms at 64 lags spread | record_call_ms at 64 lags spread | force_step_device_ms "
              "(correlation off) spread | per_step_device_ms at the sparse interval, 16 lags spread | "
              "pos_vel_copy_wall_ms spread | pos_vel_rad_copy_wall_ms spread | records per sparse window"]
    sp = lambda a: float(a.max() - a.min())

    def case(name, sim, members):
        cols, per_window = measure(sim, members, args)
        med = {k: float(np.median(v)) for k, v in cols.items()}
        lines.append("cost %s %d %d | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %g"
                     % (name, members, sim.n, med["dev16"], sp(cols["dev16"]), med["call16"], sp(cols["call16"]),
                        med["dev64"], sp(cols["dev64"]), med["call64"], sp(cols["call64"]), med["off"], sp(cols["off"]),
                        med["sparse"], sp(cols["sparse"]), med["copy"], sp(cols["copy"]), med["copy3"],
                        sp(cols["copy3"]), per_window))
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
