#!/usr/bin/env python3
"""What a record of the coherent intermediate scattering function costs (pbSimSetCoherent, csrc/pb_coherent.hip): the
device time of its launches (pbSimGetCoherentTimes) with the ring full, so that a record pairs with every lag, against
one force step, a scattering record with the same list (pbSimGetScatteringTimes), a time-correlation record at the same
lags, one pbSimStructureFactor(PB_SK_DENSITY) call with the same list including its read-back (the host route that the
header used to recommend for F(k, tau): its wall time, and the device time of its launches), and the bare pos copy, all
in one process on one GPU.

  python tools/coherent_cost.py [--reps 20] [--out profiles/coherent_scattering.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps, box 2^9; and a batch of 256 members of 1000 bots, box
2^3.  16 and 64 lags; 8, 24 and 256 wavevectors (the first 8 and all 24 of half_plane_vectors(3), and 256 random ones).
Every figure is the median of --reps repetitions after two untimed ones (records: after the ring has filled), with the
spread (max - min).

The striped lane layout of k_coh_modes is compared with one lane per vector (k_sk_accumulate's layout: the same kernel
with a single stripe) at 8 and 24 vectors, in a child process each, since the layout is chosen when the batch is
created, from PB_COHERENT_STRIPES under PB_ALLOW_ENV_OVERRIDES=1 (one of pbSimCreateBatch's A/B switches).

The file starts with the commit, the build stamp and the register counts of the code objects
(tests/test_coherent_code_objects.py compares those).  --registers-only writes the register table with the cost rows
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

from scatter_cost import kept_rows, med, time_records, yardsticks  # noqa: E402

LAGS = (16, 64)


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_coh_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


def million(pb, benchkit):
    sim = benchkit.make_sim(pb, 1000000, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    return sim, 1, 9


def ensemble(pb, benchkit):
    from helpers import jittered_blob
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
    return ens, members, 3


CASES = {"million_arena": million, "ensemble_256x1000": ensemble}


def vector_lists(pb):
    half = pb.half_plane_vectors(3)
    many = np.random.default_rng(1).integers(-64, 65, (256, 2)).astype(np.int32)
    return half[:8], half, many


def coherent_records(sim, lags, box_log2, vectors, reps):
    sim.set_coherent_scattering(-1.0, lags, box_log2, vectors)
    dev = time_records(sim.coherent_scattering_record, sim.coherent_scattering_times, lags, reps)
    rows = sim.coherent_scattering()
    assert all(r["bots_then"] > 0 and r["origins"] == reps + 3 for r in rows[0][lags - 1])
    sim.set_coherent_scattering(-1.0, 0, 0, None)
    return med(dev)


def layout_child(args):
    """One layout's rows, printed for the parent: `layout <stripes> <case> ...` at 8 and 24 vectors, 16 lags."""
    import particlerobotsimulations_amd as pb
    import benchkit
    pb.legacy.cudaInit(0, None)
    for name, make in CASES.items():
        sim, members, box = make(pb, benchkit)
        for vectors in vector_lists(pb)[:2]:
            print("layout %s %s %d %d lags 16 vectors %d | %.4f %.4f"
                  % ((args.layout_child, name, members, sim.n, len(vectors)) + coherent_records(sim, 16, box, vectors, args.reps)),
                  flush=True)
        sim.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--layout-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coherent_scattering.txt"))
    args = ap.parse_args()
    if args.layout_child:
        return layout_child(args)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = ("# Coherent intermediate scattering (csrc/pb_coherent.hip): code-object registers and cost "
            "(tools/coherent_cost.py).")
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_coherent_code_objects.py compares)")
    notes = kept_rows(args.out, "# note ") + kept_rows(args.out, "bench ")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/coherent_cost.py (which rewrites this file on a GPU, with the "
                 "commit and the build stamp) are not here yet.", regs_head] + register_rows(args.out) + notes
        open(args.out, "w").write("\n".join(lines) + "\n")
        return
    import particlerobotsimulations_amd as pb
    import benchkit
    pb.legacy.cudaInit(0, None)
    stamp = benchkit.loaded_build_stamp() or {}
    lines = [head, "# commit %s (parent of the change when the tree is not committed yet); build stamp %s" %
             (commit, json.dumps(stamp, sort_keys=True)), regs_head]
    lines += register_rows(args.out) + notes
    lines += ["", "# tools/coherent_cost.py --reps %d: milliseconds, median (max - min) of %d repetitions after two untimed ones"
              % (args.reps, args.reps),
              "# yard <case> <members> <bots> | force_step_device_ms spread | pos_copy_wall_ms spread",
              "# tc <case> <members> <bots> lags <lags> | record_device_ms spread   (a time-correlation record, ring full)",
              "# scat <case> <members> <bots> lags <lags> vectors <nvec> box_log2 <e> | record_device_ms spread   "
              "(a scattering record: snapshot + all lags, ring full)",
              "# coh <case> <members> <bots> lags <lags> vectors <nvec> box_log2 <e> | record_device_ms spread   "
              "(a coherent record: the slot's memsets, k_coh_modes, k_coh_correlate, ring full)",
              "# sk <case> <members> <bots> vectors <nvec> box_log2 <e> | call_wall_ms spread | launches_device_ms spread   "
              "(one pbSimStructureFactor(PB_SK_DENSITY) call with its read-back: the host route per sample)",
              "# layout <striped|one_lane_per_vector> <case> <members> <bots> lags 16 vectors <nvec> | record_device_ms spread"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    lists = vector_lists(pb)

    def case(name, sim, members, box_log2):
        (s, ss), (c, cs) = yardsticks(sim, members, args.reps)
        say("yard %s %d %d | %.4f %.4f | %.4f %.4f" % (name, members, sim.n, s, ss, c, cs))
        for vectors in lists:
            wall, dev = [], []
            for r in range(args.reps + 2):
                sim.synchronize()
                t0 = time.perf_counter()
                sim.structure_factor(vectors, box_log2, "density")
                t1 = time.perf_counter()
                if r >= 2:
                    wall.append((t1 - t0) * 1e3), dev.append(sim.structure_factor_times()[1])
            say("sk %s %d %d vectors %d box_log2 %d | %.4f %.4f | %.4f %.4f"
                % ((name, members, sim.n, len(vectors), box_log2) + med(wall) + med(dev)))
        for lags in LAGS:
            sim.set_time_correlation(-1.0, lags, 0.1)
            dev = time_records(sim.time_correlation_record, sim.time_correlation_times, lags, args.reps)
            sim.set_time_correlation(-1.0, 0, 0.0)
            say("tc %s %d %d lags %d | %.4f %.4f" % ((name, members, sim.n, lags) + med(dev)))
            for vectors in lists:
                sim.set_scattering(-1.0, lags, box_log2, vectors)
                dev = time_records(sim.scattering_record, sim.scattering_times, lags, args.reps)
                sim.set_scattering(-1.0, 0, 0, None)
                say("scat %s %d %d lags %d vectors %d box_log2 %d | %.4f %.4f"
                    % ((name, members, sim.n, lags, len(vectors), box_log2) + med(dev)))
                say("coh %s %d %d lags %d vectors %d box_log2 %d | %.4f %.4f"
                    % ((name, members, sim.n, lags, len(vectors), box_log2)
                       + coherent_records(sim, lags, box_log2, vectors, args.reps)))

    for name, make in CASES.items():
        sim, members, box = make(pb, benchkit)
        case(name, sim, members, box)
        sim.close()
    # the two lane layouts, a fresh process each (this one keeps the GPU open meanwhile: two processes at most)
    for layout, stripes in (("striped", "1"), ("one_lane_per_vector", "0")):
        env = dict(os.environ, PB_ALLOW_ENV_OVERRIDES="1", PB_COHERENT_STRIPES=stripes)
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--layout-child", layout, "--reps", str(args.reps)],
                               env=env, capture_output=True, text=True, timeout=600)
        if child.returncode != 0:
            raise SystemExit("the %s layout's child failed (%d):\n%s" % (layout, child.returncode, child.stderr[-2000:]))
        for line in child.stdout.splitlines():
            if line.startswith("layout "):
                say(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
