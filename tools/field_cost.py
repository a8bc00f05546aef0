#!/usr/bin/env python3
"""What a field map costs (pbSimFieldMap, csrc/pb_field.hip): the device time of its two launches (pbSimGetFieldTimes)
and the time of the whole call, read-back included, against one force step, one pbSimMoments pass (the same read
pattern with one row of atomics per workgroup: the floor) and the pos + vel + rad copy that a host route would start
with (pbSimGetStateOf per member), all in one process on one GPU.

  python tools/field_cost.py [--reps 20] [--form NAME=LIBDIR]... [--out profiles/field_maps.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps, with maps of 64 x 64, 256 x 256 and 1024 x 1024 cells
over the arena (centre 0, 0, half extent 240); and a batch of 256 members of 1000 bots with one 32 x 32 map of every
member.  Every figure is the median of --reps repetitions after two untimed ones, with the spread (max - min).

--form NAME=LIBDIR times the arena's three maps with another build of the libraries, in a child process of its own,
for the wave-level combine against the plain form and for the fallback threshold.  Such a build differs only in
PB_FIELD_ROUNDS, the leader-loop rounds per wave before the per-lane atomics (0: the plain form, eight atomics per
counted bot and no combine):
  make -C particlerobotsimulations_amd/csrc LIBDIR=../lib_field_plain BUILD=build_field_plain EXTRA_DEVFLAGS=-DPB_FIELD_ROUNDS=0

The file starts with the commit, the kernel-source hash and the register counts of the code objects
(tests/test_field_code_objects.py compares those).  --registers-only writes the register table with the cost rows
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

ARENA_HALF = 240.0
ARENA_MAPS = (64, 256, 1024)


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_field_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def med(a):
    a = np.asarray(a, float)
    return float(np.median(a)), float(a.max() - a.min())


def time_maps(sim, members, cells_per_axis, reps, half=ARENA_HALF):
    """(device ms, call ms) lists of one map of every member into a buffer made once."""
    from particlerobotsimulations_amd import _capi
    L = _capi.lib()
    view = _capi.field_view(cells_per_axis, cells_per_axis, (0.0, 0.0), half)
    cells = np.zeros((members, cells_per_axis, cells_per_axis), _capi.FIELD_CELL_DTYPE)
    tot = (_capi.pbFieldTotals * members)()
    dev, call = [], []
    for r in range(reps + 2):
        sim.synchronize()
        t0 = time.perf_counter()
        _capi.check(L.pbSimFieldMap(sim._h, C.byref(view), _capi.np_ptr(cells), tot), "pbSimFieldMap")
        t1 = time.perf_counter()
        if r >= 2:
            dev.append(sim.field_times()[1])
            call.append((t1 - t0) * 1e3)
    assert sum(t.inside + t.outside + t.unmeasured for t in tot) == members * sim.n
    return dev, call, int(sum(t.inside for t in tot)), int((cells["count"] > 0).sum())


def copy_state(sim, member, bufs):
    from particlerobotsimulations_amd import _capi
    _capi.check(_capi.lib().pbSimGetStateOf(sim._h, member, _capi.np_ptr(bufs[0]), _capi.np_ptr(bufs[1]),
                                            _capi.np_ptr(bufs[2]), None, None, None, None), "pbSimGetStateOf")


def yardsticks(sim, members, reps):
    """Medians of one force step, one moments pass and the copy of pos + vel + rad of every member."""
    bufs = (np.empty((sim.n, 2), np.float32), np.empty((sim.n, 2), np.float32), np.empty(sim.n, np.float32))
    step, mom, copy = [], [], []
    for r in range(reps + 2):
        sim.synchronize()
        done, ms = sim.step_timed(64, dt=0.01, sort_interval=180.0)
        assert done == 64
        sim.moments()
        m = sim.series_times()[1]
        sim.synchronize()
        t0 = time.perf_counter()
        for k in range(members):
            copy_state(sim, k, bufs)
        t1 = time.perf_counter()
        if r >= 2:
            step.append(ms / 64), mom.append(m), copy.append((t1 - t0) * 1e3)
    return med(step), med(mom), med(copy)


def arena(pb):
    import benchkit
    sim = benchkit.make_sim(pb, 1000000, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    return sim


def child(libdir, reps):
    """The arena's three maps with the libraries of `libdir`: one JSON line."""
    from particlerobotsimulations_amd import _capi
    _capi.LIB_DIR = os.path.abspath(libdir)
    _capi.HIP_SO = os.path.join(_capi.LIB_DIR, "libparticlebot_hip.so")
    _capi.HOST_SO = os.path.join(_capi.LIB_DIR, "libparticlebot_host.so")
    import particlerobotsimulations_amd as pb
    pb.legacy.cudaInit(0, None)
    sim = arena(pb)
    out = {}
    for c in ARENA_MAPS:
        dev, _, _, _ = time_maps(sim, 1, c, reps)
        out[str(c)] = med(dev)
    sim.close()
    print("FORM " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--form", action="append", default=[], metavar="NAME=LIBDIR")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_maps.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.reps)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = "# Field maps (csrc/pb_field.hip): code-object registers and cost (tools/field_cost.py)."
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_field_code_objects.py compares)")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/field_cost.py (which rewrites this file on a GPU, with the "
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
    lines += ["", "# tools/field_cost.py --reps %d: milliseconds, median (max - min) of %d repetitions after two untimed ones"
              % (args.reps, args.reps),
              "# yard <case> <members> <bots> | force_step_device_ms spread | moments_pass_device_ms spread | "
              "pos_vel_rad_copy_wall_ms spread",
              "# map <case> <members> <bots> <nx>x<ny> | device_ms spread | call_wall_ms spread (read-back of 64 bytes "
              "per cell included) | bots inside | cells that hold bots"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    def case(name, sim, members, maps, half=ARENA_HALF):
        (s, ss), (m, ms), (c, cs) = yardsticks(sim, members, args.reps)
        say("yard %s %d %d | %.4f %.4f | %.4f %.4f | %.4f %.4f" % (name, members, sim.n, s, ss, m, ms, c, cs))
        for cells in maps:
            dev, call, inside, filled = time_maps(sim, members, cells, args.reps, half)
            say("map %s %d %d %dx%d | %.4f %.4f | %.4f %.4f | %d | %d"
                % ((name, members, sim.n, cells, cells) + med(dev) + med(call) + (inside, filled)))

    sim = arena(pb)
    case("million_arena", sim, 1, ARENA_MAPS)
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
    case("ensemble_256x1000", ens, members, (32,), half=4.0)  # the blobs: 1000 bots at spacing 0.2
    ens.close()

    if args.form:
        lines += ["", "# form <name> | device_ms spread of the arena's maps of 64x64, 256x256, 1024x1024 cells, each build in "
                  "a process of its own (PB_FIELD_ROUNDS as the name says; plain = 0: eight atomics per counted bot)"]
    for spec in args.form:
        name, libdir = spec.split("=", 1)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", libdir, "--reps", str(args.reps)],
                           capture_output=True, text=True, timeout=900)
        got = [l for l in r.stdout.splitlines() if l.startswith("FORM ")]
        if r.returncode != 0 or not got:
            say("form %s | NOT MEASURED (exit %d)" % (name, r.returncode))
            sys.stderr.write(r.stderr[-2000:])
            break  # (a build that failed on the device: nothing more is started on it)
        out = json.loads(got[-1][5:])
        say("form %s | %s" % (name, " | ".join("%.4f %.4f" % tuple(out[str(c)]) for c in ARENA_MAPS)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
