#!/usr/bin/env python3
"""What a contact export costs: pbSimContactsOf and pbSimContactVirialOf on the 10^6-bot arena as bench.py builds it,
after 32 steps, at linkGap 0 and 0.0019, in one process on one GPU.

  python tools/contacts_cost.py [--reps 10] [--out profiles/contact_network.txt]

Per gap, over --reps repetitions after two untimed ones: device milliseconds of one export with links
(pbSimGetContactTimes after the fetching call of Sim.contacts: front end, scan, fill, order), wall milliseconds of
Sim.contacts() (the sizing call plus the fetching call and the copies), device milliseconds of one virial export, device
milliseconds of one cluster analysis alone (pbSimGetClusterTimes: the front end's share); medians and spreads
(max - min); the directed entries and the bytes returned (offsets + links).  The file starts with the commit, the
kernel-source hash and the register counts of the code objects (tests/test_contacts_api.py compares those).  Needs a
GPU: there is no fallback."""
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


def register_rows():
    import summarize_profile
    regs = summarize_profile.code_object_registers()
    return ["reg %s %s" % (k, " ".join(str(v) for v in regs[k])) for k in sorted(regs) if k.startswith("k_contact_")]


def measure(sim, gap, reps):
    dev, wall, vir, front = [], [], [], []
    net = None
    for r in range(reps + 2):
        sim.synchronize()
        t0 = time.perf_counter()
        net = sim.contacts(gap)
        t1 = time.perf_counter()
        d = sim.contact_times()[1]
        sim.contact_virial(gap)
        v = sim.contact_times()[1]
        sim.clusters(gap)
        if r >= 2:
            dev.append(d)
            wall.append((t1 - t0) * 1e3)
            vir.append(v)
            front.append(sim.cluster_times()[1])
    return [np.array(a) for a in (dev, wall, vir, front)], net


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bots", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contact_network.txt"))
    args = ap.parse_args()
    import particlerobotsimulations_amd as pb
    import benchkit
    pb.legacy.cudaInit(0, None)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    stamp = benchkit.loaded_build_stamp() or {}
    lines = ["# Contact export (csrc/pb_contacts.hip): code-object registers and cost (tools/contacts_cost.py).",
             "# commit %s (parent of the change when the tree is not committed yet); build stamp %s" %
             (commit, json.dumps(stamp, sort_keys=True)),
             "# reg <kernel> <vgpr> <sgpr> <lds bytes> <scratch bytes>   (from the code objects; "
             "tests/test_contacts_api.py compares)"]
    lines += register_rows()
    lines += ["",
              "# tools/contacts_cost.py --reps %d --bots %d: milliseconds, median (max - min)" % (args.reps, args.bots),
              "# case bots linkGap | export_device_ms spread | contacts_wall_ms spread | virial_export_device_ms spread | "
              "cluster_analysis_device_ms spread | directed entries | bytes returned (offsets + links)"]
    sim = benchkit.make_sim(pb, args.bots, benchkit.LATTICE_PITCH, seed=1)
    assert sim.step(32) == 32
    sp = lambda a: float(a.max() - a.min())
    for gap in (0.0, 0.0019):
        (dev, wall, vir, front), net = measure(sim, gap, args.reps)
        entries = int(net["other"].size)
        lines.append("cost million_arena %d %g | %.4f %.4f | %.4f %.4f | %.4f %.4f | %.4f %.4f | %d | %d" % (
            sim.n, gap, np.median(dev), sp(dev), np.median(wall), sp(wall), np.median(vir), sp(vir), np.median(front),
            sp(front), entries, 4 * (sim.n + 1) + 16 * entries))
        print(lines[-1], flush=True)
    sim.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
