#!/usr/bin/env python3
"""What a record of the bond recorder costs (pbSimSetBondDynamics, csrc/pb_bonds.hip): the device time of its launches
(pbSimGetBondDynamicsTimes) with the ring full, so that a record pairs with every lag, against one force step, a
time-correlation record with the same lags (pbSimGetTimeCorrelationTimes), one pbSimMarkReference plus one
pbSimRearrangementStats (the route a caller had per pair of origins: pbSimGetRearrangementTimes of each) and the bare
pos + rad copy a host route would start with, all in one process on one GPU.

  python tools/bonds_cost.py [--reps 20] [--out profiles/bond_dynamics.txt]

Cases: the 10^6-bot arena as bench.py builds it, after 32 steps; and a batch of 256 members of 1000 bots.  16 and 64
lags.  Between two bond records every bot takes a step of its own, a multiple of 1/256 within +-1/64 per axis (set from
the host: the time of that copy is not in the device span that is measured), so that a share of the bonds breaks per
lag: the `bond` rows end with bonds_kept / bonds_then at lag 1 and at the last lag, the mean degree of a sampled bot and
the crowded fraction.  The link gap is 0.002, the largest radius the state's own largest, the overlap radius 1/128.

THE SNAPSHOT AND THE PAIRING.  A record is the filing (hash, sort, gather, cell starts), k_bond_snapshot and k_bond_pairs
over all paired lags, between two events.  The `bond ... lags 1` rows are a record into a ring of one slot: the filing,
the snapshot and the pairing of the record with itself; the rows at 16 and 64 lags hold the same filing and snapshot and
the pairing with every lag, so their difference to the lags-1 row is the pairing's cost of 15 and 63 more lags.  Every
figure is the median of --reps records after the ring has filled and two more, with the spread (max - min).

The file starts with the commit, the build stamp and the register counts of the code objects
(tests/test_bonds_code_objects.py compares those).  --registers-only writes the register table with the cost rows marked
as not measured and needs no GPU; everything else needs one: there is no fallback."""
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

from coherent_cost import CASES  # noqa: E402
from scatter_cost import kept_rows, med, time_records  # noqa: E402

LAGS = (1, 16, 64)
GAP, OVERLAP = 0.002, 0.0078125


def register_rows(out):
    """The `reg` rows of this build's code objects; where the objects are not at hand (libraries copied without
    csrc/build), the rows the file already holds are kept."""
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    rows = ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_bond_")]
    if not rows and os.path.exists(out):
        rows = [l.rstrip("\n") for l in open(out) if l.startswith("reg ")]
    return rows


class Walk:
    """Every bot of every member stepped on its own between two records, from the positions the batch had at first."""

    def __init__(self, sim, members):
        self.sim, self.members = sim, members
        states = [sim.get_state_of(k) if members > 1 else sim.get_state() for k in range(members)]
        self.base = [np.array(s["pos"], np.float32) for s in states]
        self.max_radius = float(max(np.max(s["rad"]) for s in states))

    def restart(self):
        self.pos = [b.copy() for b in self.base]
        self.rng = np.random.default_rng(7)

    def step(self):
        for k, p in enumerate(self.pos):
            p += self.rng.integers(-4, 5, size=p.shape).astype(np.float32) / np.float32(256.0)
            if self.members > 1:
                self.sim.set_state_of(k, pos=p)
            else:
                self.sim.set_state(pos=p)


def bond_records(sim, walk, lags, reps):
    sim.set_bond_dynamics(-1.0, lags, GAP, walk.max_radius, OVERLAP)
    walk.restart()

    def step_and_record():
        walk.step()
        sim.bond_dynamics_record()
    dev = time_records(step_and_record, sim.bond_dynamics_times, lags, reps)
    rows = sim.bond_dynamics()[0]
    assert rows[lags - 1]["samples"] > 0 and rows[lags - 1]["origins"] == reps + 3
    near, far = rows[min(1, lags - 1)], rows[lags - 1]
    share = lambda r: r["bonds_kept"] / r["bonds_then"] if r["bonds_then"] else float("nan")
    figures = (share(near), share(far), near["bonds_then"] / near["samples"], near["crowded"] / (near["samples"] + near["crowded"]))
    sim.set_bond_dynamics(-1.0, 0, 0.0, 0.0, 0.0)
    return med(dev) + figures


def yardsticks(sim, members, reps):
    """Medians of one force step, of a mark, of a compare, and of the copy of pos and rad of every member."""
    from particlerobotsimulations_amd import _capi
    pos, rad = np.empty((sim.n, 2), np.float32), np.empty(sim.n, np.float32)
    step, mark, compare, copy = [], [], [], []
    for r in range(reps + 2):
        sim.synchronize()
        done, ms = sim.step_timed(64, dt=0.01, sort_interval=180.0)
        assert done == 64
        sim.mark_reference(GAP)
        m = sim.rearrangement_times()[1]
        sim.rearrangement()
        c = sim.rearrangement_times()[1]
        sim.synchronize()
        t0 = time.perf_counter()
        for k in range(members):
            _capi.check(_capi.lib().pbSimGetStateOf(sim._h, k, _capi.np_ptr(pos), None, _capi.np_ptr(rad), None, None, None,
                                                    None), "pbSimGetStateOf")
        t1 = time.perf_counter()
        if r >= 2:
            step.append(ms / 64), mark.append(m), compare.append(c), copy.append((t1 - t0) * 1e3)
    sim.clear_reference()
    return med(step), med(mark), med(compare), med(copy)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--registers-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bond_dynamics.txt"))
    args = ap.parse_args()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    head = "# Bond dynamics (csrc/pb_bonds.hip): code-object registers and cost (tools/bonds_cost.py)."
    regs_head = ("# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
                 "tests/test_bonds_code_objects.py compares)")
    notes = kept_rows(args.out, "# note ") + kept_rows(args.out, "bench ")
    if args.registers_only:
        lines = [head.replace(" and cost", ""),
                 "# NOT MEASURED: the cost rows of tools/bonds_cost.py (which rewrites this file on a GPU, with the "
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
    lines += ["", "# tools/bonds_cost.py --reps %d: milliseconds, median (max - min) of %d repetitions after two untimed ones; "
              "a random step of every bot between two bond records, link gap %g, overlap radius %g"
              % (args.reps, args.reps, GAP, OVERLAP),
              "# yard <case> <members> <bots> | force_step_device_ms spread | mark_device_ms spread | compare_device_ms spread "
              "| pos_rad_copy_wall_ms spread   (mark: pbSimMarkReference; compare: pbSimRearrangementStats)",
              "# tc <case> <members> <bots> lags <lags> | record_device_ms spread   (a time-correlation record, ring full)",
              "# bond <case> <members> <bots> lags <lags> | record_device_ms spread | bonds kept/then at lag 1, at the last "
              "lag | mean degree | crowded fraction   (a bond record: filing, k_bond_snapshot, k_bond_pairs, ring full; lags 1 "
              "is the filing, the snapshot and the self-pair alone)"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for name, make in CASES.items():
        sim, members, _ = make(pb, benchkit)
        (s, ss), (m, ms), (c, cs), (p, ps) = yardsticks(sim, members, args.reps)
        say("yard %s %d %d | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f" % (name, members, sim.n, s, ss, m, ms, c, cs, p, ps))
        walk = Walk(sim, members)
        for lags in LAGS:
            if lags > 1:
                sim.set_time_correlation(-1.0, lags, OVERLAP)
                dev = time_records(sim.time_correlation_record, sim.time_correlation_times, lags, args.reps)
                sim.set_time_correlation(-1.0, 0, 0.0)
                say("tc %s %d %d lags %d | %.4f %.4f" % ((name, members, sim.n, lags) + med(dev)))
            say("bond %s %d %d lags %d | %.4f %.4f | %.3f %.3f | %.2f | %.4f"
                % ((name, members, sim.n, lags) + bond_records(sim, walk, lags, args.reps)))
        sim.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
