#!/usr/bin/env python3
"""What a record of the four-point recorder costs (pbSimSetFourPoint, csrc/pb_fourpoint.hip): the device time of its
launches (pbSimGetFourPointTimes) with the ring full, so that a record pairs with every lag, against a scattering record
with the same list and lags (pbSimGetScatteringTimes: the same number of table look-ups, the natural yardstick), one
force step and the bare pos copy a host route would start with, all in one process on one GPU.

  python tools/fourpoint_cost.py [--reps 20] [--out profiles/four_point.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps, box 2^9; and a batch of 256 members of 1000 bots, box
2^3.  16 and 64 lags; 8, 24 and 256 wavevectors (the first 8 and all 24 of half_plane_vectors(3), and 256 random ones).
Between two four-point records every bot takes a step of its own, a multiple of 1/64 within +-1/4 per axis (set from
the host: the time of that copy is not in the device span that is measured), and the overlap radius is 0.2, so that
about half the pairs overlap at lag 1 and ever fewer at longer lags: the `fp` rows end with the fraction that did,
overlap / samples, at lag 1 and at the last lag.  A scattering record costs the same whatever the bots did and is taken
of a still state.  Every figure is the median of --reps records after the ring has filled and two more, with the spread
(max - min).

The staging of k_fp_modes, compacted (ships) or masked, is chosen when the library is built (-DPB_FOURPOINT_COMPACT=0 in
EXTRA_DEVFLAGS for the masked form): --form names the loaded build's in the `fp` rows, and the two builds are run one
after the other; --append adds a run's rows to the file instead of rewriting it.

The file starts with the commit, the build stamp and the register counts of the code objects
(tests/test_fourpoint_code_objects.py compares those).  --registers-only writes the register table with the cost rows
marked as not measured and needs no GPU; everything else needs one: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from coherent_cost import CASES, vector_lists  # noqa: E402
from scatter_cost import kept_rows, med, time_records, yardsticks  # noqa: E402

LAGS = (16, 64)
RADIUS = 0.2  # P(dx^2 + dy^2 < RADIUS^2) is about a half for dx, dy uniform within +-1/4


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_fp_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


class Walk:
    """Every bot of every member stepped on its own between two records, from the positions the batch had at first."""

    def __init__(self, sim, members):
        self.sim, self.members = sim, members
        self.base = [np.array((sim.get_state_of(k) if members > 1 else sim.get_state())["pos"], np.float32)
                     for k in range(members)]

    def restart(self):
        self.pos = [b.copy() for b in self.base]
        self.rng = np.random.default_rng(7)

    def step(self):
        for k, p in enumerate(self.pos):
            p += self.rng.integers(-16, 17, size=p.shape).astype(np.float32) / np.float32(64.0)
            if self.members > 1:
                self.sim.set_state_of(k, pos=p)
            else:
                self.sim.set_state(pos=p)


def four_point_records(sim, walk, lags, box_log2, vectors, reps):
    sim.set_four_point(-1.0, lags, RADIUS, box_log2, vectors)
    walk.restart()

    def step_and_record():
        walk.step()
        sim.four_point_record()
    dev = time_records(step_and_record, sim.four_point_times, lags, reps)
    rows = sim.four_point()[0]
    assert all(r["samples"] > 0 and r["origins"] == reps + 3 for r in rows[lags - 1])
    fractions = tuple(rows[l][0]["overlap"] / rows[l][0]["samples"] for l in (1, lags - 1))
    sim.set_four_point(-1.0, 0, 0.0, 0, None)
    return med(dev) + fractions


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--form", default="compacted", choices=("masked", "compacted"), help="the loaded build's staging")
    ap.add_argument("--append", action="store_true", help="add this build's `fp` rows to --out as it is")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "four_point.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = "# Four-point dynamics (csrc/pb_fourpoint.hip): code-object registers and cost (tools/fourpoint_cost.py)."
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_fourpoint_code_objects.py compares)")
    notes = kept_rows(args.out, "# note ") + kept_rows(args.out, "bench ")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/fourpoint_cost.py (which rewrites this file on a GPU, with the "
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
    lines += ["", "# tools/fourpoint_cost.py --reps %d: milliseconds, median (max - min) of %d repetitions after two untimed ones; "
              "a random step of every bot between two four-point records, overlap radius %g" % (args.reps, args.reps, RADIUS),
              "# yard <case> <members> <bots> | force_step_device_ms spread | pos_copy_wall_ms spread",
              "# scat <case> <members> <bots> lags <lags> vectors <nvec> box_log2 <e> | record_device_ms spread   "
              "(a scattering record: snapshot + all lags, ring full)",
              "# fp <masked|compacted> <case> <members> <bots> lags <lags> vectors <nvec> box_log2 <e> | record_device_ms spread | "
              "overlap/samples at lag 1, at the last lag   (a four-point record: snapshot, the scratch's memsets, k_fp_modes "
              "in that form, k_fp_fold, ring full)"]
    if args.append:  # the other build's rows behind what the file holds
        lines = [l.rstrip("\n") for l in open(args.out)]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    lists = vector_lists(pb)
    for name, make in CASES.items():
        sim, members, box_log2 = make(pb, benchkit)
        if not args.append:
            (s, ss), (c, cs) = yardsticks(sim, members, args.reps)
            say("yard %s %d %d | %.4f %.4f | %.4f %.4f" % (name, members, sim.n, s, ss, c, cs))
        walk = Walk(sim, members)
        for lags in LAGS:
            for vectors in lists:
                if not args.append:
                    sim.set_scattering(-1.0, lags, box_log2, vectors)
                    dev = time_records(sim.scattering_record, sim.scattering_times, lags, args.reps)
                    sim.set_scattering(-1.0, 0, 0, None)
                    say("scat %s %d %d lags %d vectors %d box_log2 %d | %.4f %.4f"
                        % ((name, members, sim.n, lags, len(vectors), box_log2) + med(dev)))
                say("fp %s %s %d %d lags %d vectors %d box_log2 %d | %.4f %.4f | %.3f %.3f"
                    % ((args.form, name, members, sim.n, lags, len(vectors), box_log2)
                       + four_point_records(sim, walk, lags, box_log2, vectors, args.reps)))
        sim.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
