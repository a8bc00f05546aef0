#!/usr/bin/env python3
"""What a frame costs: the host frame writer (state copy + CPU rasteriser + file) against the device rasteriser
(pbSimRenderOf + file), timed alternately in one process on one GPU, both writing to the same temporary directory.

  python tools/frame_cost.py [--reps 20] [--out FILE]

Cases: examples/million_bots.cfg after 32 steps, whole arena and a 64-bot-wide window, at 1024^2 and 2048^2, plain and
reference style; examples/example_gap.cfg after 300 steps at the reference camera (large footprints).  Columns: median
and spread (max - min) of the wall time of each path in milliseconds over --reps alternating repetitions after two
untimed ones, and the median device time of the render launches alone (HIP events on the engine's stream, without the
copy to the host).  Needs a GPU: there is no fallback."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(h, d, size, center, half, style, reps):
    host_p, dev_p = os.path.join(d, "host.ppm"), os.path.join(d, "device.ppm")
    th, td, tk = [], [], []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        h.write_frame(host_p, size=size, center=center, half_extent=half, style=style)
        t1 = time.perf_counter()
        h.write_frame(dev_p, size=size, center=center, half_extent=half, style=style, renderer="device")
        t2 = time.perf_counter()
        if r >= 2:
            th.append((t1 - t0) * 1e3)
            td.append((t2 - t1) * 1e3)
            tk.append(h.render_stats()[1])
    same = open(host_p, "rb").read() == open(dev_p, "rb").read()
    return np.array(th), np.array(td), np.array(tk), same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from particlerobotsimulations_amd import host
    lines = ["# tools/frame_cost.py --reps %d: wall milliseconds per frame, median (max - min); host = writeFramePPM[Reference] "
             "with its state copy, device = writeFramePPMDevice; kernels = device time of the render launches alone" % args.reps,
             "# case size style host_ms host_spread device_ms device_spread kernels_ms same_bytes"]

    def row(case, h, d, size, center, half, style):
        th, td, tk, same = measure(h, d, size, center, half, style, args.reps)
        lines.append("cost %s %dx%d %s %.3f %.3f %.3f %.3f %.4f %s" % (
            case, size, size, style, np.median(th), th.max() - th.min(), np.median(td), td.max() - td.min(),
            np.median(tk), "yes" if same else "NO"))
        print(lines[-1], flush=True)

    with tempfile.TemporaryDirectory() as d:
        h = host.HostSim(os.path.join(ROOT, "examples", "million_bots.cfg"), engine="fused", max_time="1e9")
        assert h.advance(32) == 32
        pos = h.get("pos")
        lo, hi = pos.min(axis=0), pos.max(axis=0)
        c = (float((lo[0] + hi[0]) / 2), float((lo[1] + hi[1]) / 2))
        arena = float(max(hi[0] - lo[0], hi[1] - lo[1]) / 2) * 1.02
        pitch = float(np.sqrt((hi[0] - lo[0]) * (hi[1] - lo[1]) / h.n))
        for size in (1024, 2048):
            for case, half in (("million_arena", arena), ("million_window64", 32.0 * pitch)):
                for style in ("plain", "reference"):
                    row(case, h, d, size, c, half, style)
        del h
        g = host.HostSim(os.path.join(ROOT, "examples", "example_gap.cfg"), engine="fused", max_time="1e9")
        assert g.advance(300) == 300
        for size in (1024, 2048):
            for style in ("plain", "reference"):
                row("example_gap_camera", g, d, size, (0.0, 0.0), 0.0, style)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
